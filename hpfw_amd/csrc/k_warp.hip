// k_warp.hip -- time warp and mix of int16 PCM (DESIGN.md section 16 states the contract, tests/warp_ref.py restates it in
// numpy): output m of a track reads its source at i0 + m + (f0 + m d) 2^-40 through a polyphase windowed sinc of
// P = 4096 fractional delays, T = 32 taps each, in exact integer arithmetic.
//
//   warp_design    host, float64: the [P][T] int16 table, every row summing to exactly 2^14, row 0 the unit impulse
//   warp_kernel    one workgroup = one tile of kWarpTile consecutive outputs of one track.  The tile stages its input span
//                  in LDS with the staging of the sample-rate conversion (16-byte loads over the aligned interior, zeros
//                  outside the source), then lane l computes outputs l, l + 256, ...: T int16 products on v_dot2_i32_i16,
//                  sample pairs realigned with v_alignbit_b32 when the first tap's sample is odd.  The position is one
//                  int64 per tile and per lane; a lane steps it by the uniform 256 d.  The 64 consecutive outputs of a
//                  wave differ in position by 64 d 2^-40 <= 1/16 sample: when they share one table row -- always at d = 0,
//                  mostly at a few ppm -- the row is read once for the wave through the scalar cache, else each lane reads
//                  its own of the few neighbouring rows (256 KB in all: the vector caches).
//   mix_kernel     one workgroup = one tile of the mix: the same per track whose reach (warp_reach, drift_plan.h) meets the
//                  tile, g_k y_k summed in int64 registers; no track is materialised.
#include <cmath>
#include <algorithm>

#include "drift_plan.h"
#include "kernels.h"
#include "resample_dev.h"

namespace hpfw {

namespace {

double warp_bessel_i0(double x)
{
    double sum = 1.0, term = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}

} // namespace

bool warp_design(std::vector<int16_t> &taps)
{
    constexpr int P = kWarpP, H = kWarpH, T = kWarpT;
    const double beta = 8.0, i0b = warp_bessel_i0(beta);
    taps.assign((size_t)P * T, 0);
    std::vector<double> h((size_t)T);
    std::vector<int64_t> q((size_t)T);
    for (int p = 0; p < P; ++p) {
        double sum = 0.0;
        for (int j = 0; j < T; ++j) {
            const double tau = (double)j - H + 1 - (double)p / P, r = tau / H; // cutoff 1: the zeros of the sinc are the samples
            const double px = M_PI * (tau == 0.0 ? 1.0e-20 : tau);
            h[(size_t)j] = (std::sin(px) / px) * warp_bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
            sum += h[(size_t)j];
        }
        int64_t total = 0, l1 = 0;
        for (int j = 0; j < T; ++j) {
            q[(size_t)j] = (int64_t)std::nearbyint(h[(size_t)j] / sum * (double)(1 << kRsShift));
            total += q[(size_t)j];
        }
        q[(size_t)(H - 1)] += ((int64_t)1 << kRsShift) - total; // every row sums to exactly 2^14
        int16_t *row = taps.data() + (size_t)p * T;
        for (int j = 0; j < T; ++j) {
            if (q[(size_t)j] < -32768 || q[(size_t)j] > 32767) return false;
            row[j] = (int16_t)q[(size_t)j];
            l1 += std::abs(q[(size_t)j]);
        }
        if (32768 * l1 >= ((int64_t)1 << 31)) return false; // the int32 accumulator cannot overflow
    }
    return true;
}

namespace {

constexpr int kWarpTile = kRsTile;                                       // outputs per workgroup
constexpr int kWarpChunks = kWarpT / 8;                                  // 16-byte chunks of a table row
constexpr int kWarpSlide = (int)(((int64_t)kWarpTile * kWarpDMax) >> kWarpFrac) + 2; // what a tile's span can gain or lose by d
constexpr int kWarpSpan = (kWarpTile + kWarpSlide + kWarpT + 2 + 7) / 8 * 8;         // int16 slots of the staged span
static_assert(kWarpT % 8 == 0, "a table row is whole 16-byte chunks");

// (sum + 2^13) >> 14 of one output, not clamped: the staged samples as words sw, the first tap's sample k (an odd k: each
// pair straddles two words), the row's 16-byte chunks of taps
__device__ __forceinline__ int warp_value(const uint32_t *sw, uint32_t k, const int4 *row)
{
    const uint32_t *xs = sw + (k >> 1);
    const uint32_t sh = (k & 1) * 16;
    int acc = 0;
    uint32_t prev = xs[0];
#pragma unroll
    for (int c = 0; c < kWarpChunks; ++c) {
        const int4 tv = row[c];
        const uint32_t w1 = xs[4 * c + 1], w2 = xs[4 * c + 2], w3 = xs[4 * c + 3], w4 = xs[4 * c + 4];
        acc = dot2(__builtin_amdgcn_alignbit(w1, prev, sh), (uint32_t)tv.x, acc);
        acc = dot2(__builtin_amdgcn_alignbit(w2, w1, sh), (uint32_t)tv.y, acc);
        acc = dot2(__builtin_amdgcn_alignbit(w3, w2, sh), (uint32_t)tv.z, acc);
        acc = dot2(__builtin_amdgcn_alignbit(w4, w3, sh), (uint32_t)tv.w, acc);
        prev = w4;
    }
    return (acc + (1 << (kRsShift - 1))) >> kRsShift;
}

__device__ __forceinline__ int clamp16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// The outputs [mb, me) of track t (me - mb <= kWarpTile): stages the span in s and hands every output of this lane, in the
// order r = 0, 1, ..., to emit(r, m, value).  Called by the whole workgroup.
template <class Emit>
__device__ __forceinline__ void warp_tile(const WarpTrack &t, const int16_t *__restrict__ pcm, const int4 *__restrict__ tab, int64_t mb,
                                          int64_t me, int16_t *s, Emit emit)
{
    const int64_t ub = t.f0 + mb * t.d, hb = ub >> kWarpFrac;             // |mb d| < 2^61
    const int64_t ipb = t.i0 + mb + hb;                                   // the first output's centre sample: the smallest
    const int64_t ul = t.f0 + (me - 1) * t.d;
    const int span = (int)((me - 1 - mb) + ((ul >> kWarpFrac) - hb)) + kWarpT + 2; // <= kWarpSpan
    __syncthreads(); // (the previous track is done with s)
    stage_span(pcm + t.src_off, t.src_len, ipb - kWarpH + 1, span, s);
    __syncthreads();
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(s);
    const int64_t step = (int64_t)kRsThreads * t.d;
    int64_t u = ub + (int64_t)threadIdx.x * t.d;
#pragma unroll
    for (int r = 0; r < kRsPerLane; ++r, u += step) {
        const int64_t m = mb + threadIdx.x + (int64_t)r * kRsThreads;
        // (lanes past the end compute inside the staged buffer and emit nothing: the wave stays whole for the ballot)
        const bool live = m < me;
        const int64_t uu = live ? u : ub;
        const uint32_t k = live ? (uint32_t)((int)threadIdx.x + r * kRsThreads + (int)((uu >> kWarpFrac) - hb)) : 0u;
        const uint32_t p = (uint32_t)((uu & (((int64_t)1 << kWarpFrac) - 1)) >> (kWarpFrac - kWarpPB));
        const uint32_t p0 = __builtin_amdgcn_readfirstlane(p);
        int v;
        if (__builtin_amdgcn_ballot_w64(p != p0) == 0)
            v = warp_value(sw, k, tab + (size_t)p0 * kWarpChunks); // one row for the wave
        else
            v = warp_value(sw, k, tab + (size_t)p * kWarpChunks);
        if (live) emit(r, m, v);
    }
}

struct WarpArgs {
    const int16_t *pcm;
    const WarpTrack *tracks;
    const int4 *tab; // [P][kWarpChunks]
    int16_t *out;
    int64_t m0, n_out;
    int32_t n_tracks;
};

__global__ __launch_bounds__(kRsThreads) void warp_kernel(WarpArgs a)
{
    __shared__ __align__(16) int16_t s[kWarpSpan];
    const WarpTrack t = a.tracks[blockIdx.y];
    const int64_t o0 = (int64_t)blockIdx.x * kWarpTile, o1 = o0 + kWarpTile < a.n_out ? o0 + kWarpTile : a.n_out;
    int16_t *y = a.out + (int64_t)blockIdx.y * a.n_out;
    const int64_t mb = a.m0 + o0, me = a.m0 + o1;
    if (t.m_hi < mb || t.m_lo >= me) { // no tap of the tile reaches the source
        for (int64_t o = o0 + threadIdx.x; o < o1; o += kRsThreads) y[o] = 0;
        return;
    }
    const bool neg = t.gain < 0;
    warp_tile(t, a.pcm, a.tab, mb, me, s, [&](int, int64_t m, int v) { y[m - a.m0] = (int16_t)clamp16(neg ? -v : v); });
}

__global__ __launch_bounds__(kRsThreads) void mix_kernel(WarpArgs a)
{
    __shared__ __align__(16) int16_t s[kWarpSpan];
    const int64_t o0 = (int64_t)blockIdx.x * kWarpTile, o1 = o0 + kWarpTile < a.n_out ? o0 + kWarpTile : a.n_out;
    const int64_t mb = a.m0 + o0, me = a.m0 + o1;
    int64_t sum[kRsPerLane];
#pragma unroll
    for (int r = 0; r < kRsPerLane; ++r) sum[r] = 0;
    for (int i = 0; i < a.n_tracks; ++i) {
        const WarpTrack t = a.tracks[i];
        if (t.m_hi < mb || t.m_lo >= me || t.gain == 0) continue; // (uniform over the workgroup)
        const int64_t g = t.gain;
        warp_tile(t, a.pcm, a.tab, mb, me, s, [&](int r, int64_t, int v) { sum[r] += g * clamp16(v); });
    }
#pragma unroll
    for (int r = 0; r < kRsPerLane; ++r) {
        const int64_t o = o0 + threadIdx.x + (int64_t)r * kRsThreads;
        if (o < o1) {
            const int64_t v = (sum[r] + (1 << 14)) >> 15;
            a.out[o] = (int16_t)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v));
        }
    }
}

} // namespace

// d_tracks [n_tracks] with their reach filled in, d_tab: resample_device_table's image of warp_design's table.
// mix: d_out [n_out], else [n_tracks][n_out]
void launch_warp(const int16_t *d_pcm, const WarpTrack *d_tracks, int64_t n_tracks, const int32_t *d_tab, int64_t m0, int64_t n_out, bool mix,
                 int16_t *d_out, hipStream_t s)
{
    if (n_out <= 0 || (!mix && n_tracks <= 0)) return;
    WarpArgs a;
    a.pcm = d_pcm;
    a.tab = reinterpret_cast<const int4 *>(d_tab);
    a.m0 = m0;
    a.n_out = n_out;
    const unsigned gx = (unsigned)((n_out + kWarpTile - 1) / kWarpTile); // <= 2^20
    if (mix) {
        a.tracks = d_tracks;
        a.out = d_out;
        a.n_tracks = (int32_t)n_tracks;
        hipLaunchKernelGGL(mix_kernel, dim3(gx), dim3(kRsThreads), 0, s, a);
        return;
    }
    for (int64_t c0 = 0; c0 < n_tracks; c0 += 65535) {
        const unsigned gy = (unsigned)std::min<int64_t>(65535, n_tracks - c0);
        a.tracks = d_tracks + c0;
        a.out = d_out + c0 * n_out;
        a.n_tracks = (int32_t)gy;
        hipLaunchKernelGGL(warp_kernel, dim3(gx, gy), dim3(kRsThreads), 0, s, a);
    }
}

} // namespace hpfw
