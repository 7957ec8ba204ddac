// k_xcorr.hip -- exact windowed cross-correlation of int16 PCM: for a job (xcorr_plan.h) and
// every lag index t in [0, 2 radius]
//     r[t] = sum over n in [0, len) of a[w + t + n] b[n]        (a read as 0 outside its operand)
// in int64, integer work only: no rounding, no summation order, so the parts of a job are added with 64-bit integer
// atomics and the result is the same bits whatever the order.
//
//   xcorr_init_kernel   r = the bias term of the digit split for the lags of the matrix-core parts, 0 for the others
//   xcorr_mfma_kernel   a part = 1024 lags x up to 16 384 samples on v_mfma_i32_32x32x32_i8, as a Toeplitz product
//   xcorr_valu_kernel   a part = 256 lags x up to 4096 samples, one lag per thread, 64-bit accumulation: the
//                       independent cross-check and the fallback (HPFW_XCORR=valu)
//   xcorr_peak_kernel   per job the lag of the largest |r| (ties: the smaller |lag|, then the negative lag) and the two energies
//
// The Toeplitz product.  With A[i][k] = a_d[base + i + k] (32 rows of one digit plane, each shifted by one sample) and
// B[k][j] = b_d[n0 + k - 32 j] (32 columns, each shifted by 32 samples) element (i, j) of A B is
// sum_k a_d[base + i + k] b_d[n0 + k - 32 j]: with base = w + t0 + n0 the terms n = n0 + k - 32 j of lag t0 + i + 32 j.  One
// accumulator tile holds the 1024 lags t0 + i + 32 j; stepping n0 by 32 from the first sample of the part to 31 steps past
// its last one, with b_d read as 0 outside the part, gives every lag every sample of the part once.  (Which k a lane's
// sixteen bytes stand for does not matter: both operands are laid out by the same rule.)
//
// Digits: x = 256 hi + lo + 128 with hi = x >> 8 and lo = (x & 255) - 128, both in [-128, 127] (k_forward.hip), for both
// operands; a sample of a outside its operand is the digits of 0.  With x' = x - 128 = 256 hi + lo:
//     sum a b = sum a' b' + 128 (sum_n a[w + t + n] + sum_n b[n] - 128 len)
// and the second term -- a sliding sum of a, the sum of b, a constant -- is what xcorr_init_kernel writes before the parts
// add theirs.  lo lo goes to accumulator 0, lo hi and hi lo share accumulator 1, hi hi goes to accumulator 2:
// sum a' b' = acc0 + 2^8 acc1 + 2^16 acc2.  |acc1| <= 2 . 16 384 . 2^14 = 2^29 over a part (kXcChunk): the int32 accumulators
// are flushed to int64 at the end of every part, never later.
//
// A workgroup = 4 waves = one part.  The digits of the part lie in LDS: a as two byte planes of the window
// [w + t0 + m0, + 32 steps + 64), b as two planes of 16-byte units with the even and the odd units apart, so that the 32
// lanes of a half wave -- units n0 / 16 + h - 2 j -- read consecutive units (ds_read_b128, aligned).  The A fragment starts
// at any byte: five aligned dwords and four v_alignbyte_b32.  The waves take the steps in turn (s = wave, wave + 4, ...),
// nothing is exchanged in the loop; at the end the four tiles are added through LDS and go out as 1024 atomics.  72 KB of
// LDS: two workgroups per CU, one staging under the other's matrix instructions.
#include "kernels.h"

namespace hpfw {

extern __shared__ __align__(16) unsigned char xc_smem[];

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef short xc_s8 __attribute__((ext_vector_type(8)));
typedef xc_s8 xc_s8u __attribute__((aligned(2))); // eight samples wherever they start

constexpr int kXcThreads = 256;
constexpr int kXcSteps = kXcChunk / 32 + 31;          // 543 matrix-instruction steps of a full part
constexpr int kXcABytes = kXcSteps * 32 + 64;         // 17 440: a plane of a (the last fragment ends 34 bytes past the steps)
constexpr int kXcBUnits = kXcSteps + 31;              // 574 pairs of 16-byte units: 31 steps of zeros on either side
constexpr int kXcBHalf = kXcBUnits * 16;              // the even (or odd) units of a plane of b
constexpr int kXcLds = 2 * kXcABytes + 4 * kXcBHalf;  // 71 616
constexpr int kXcRedStride = 33 * 32;                 // a wave's tile in the final sum: [j][33] int64
static_assert(kXcABytes % 16 == 0 && kXcBHalf % 16 == 0, "planes start on 16-byte boundaries");
static_assert(4 * kXcRedStride * 8 <= kXcLds, "the four tiles of the final sum fit the planes' memory");

__device__ __forceinline__ int xc_a(const int16_t *__restrict__ pcm, const XcJob &j, int64_t i)
{
    return (i >= 0 && i < j.a_len) ? (int)pcm[j.a0 + i] : 0;
}

// sum of v over the workgroup, in every thread (red [kXcThreads])
__device__ __forceinline__ long long xc_block_sum(long long v, long long *red)
{
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int o = kXcThreads / 2; o >= 1; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

// this thread's share of the sum (SQ: of the squares) of x[0 .. n): eight samples per load
template <bool SQ>
__device__ __forceinline__ long long xc_span_sum(const int16_t *__restrict__ x, int64_t n)
{
    const int tid = threadIdx.x;
    const int64_t n8 = n >> 3;
    long long s = 0;
#pragma unroll 2
    for (int64_t k = tid; k < n8; k += kXcThreads) {
        const xc_s8u v = *reinterpret_cast<const xc_s8u *>(x + 8 * k);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += SQ ? (long long)((int)v[e] * (int)v[e]) : (long long)v[e];
    }
    for (int64_t i = 8 * n8 + tid; i < n; i += kXcThreads) s += SQ ? (long long)((int)x[i] * (int)x[i]) : (long long)x[i];
    return s;
}

// the same over a[w .. w + len), 0 outside the operand
template <bool SQ>
__device__ __forceinline__ long long xc_window_sum(const int16_t *__restrict__ pcm, const XcJob &j, int64_t w)
{
    const int64_t lo = w > 0 ? w : 0, hi = w + j.len < j.a_len ? w + j.len : j.a_len;
    return hi > lo ? xc_span_sum<SQ>(pcm + j.a0 + lo, hi - lo) : 0;
}

// one workgroup per job
__global__ __launch_bounds__(kXcThreads) void xcorr_init_kernel(const int16_t *__restrict__ pcm, const XcJob *__restrict__ jobs,
                                                                long long *__restrict__ r)
{
    __shared__ long long red[kXcThreads];
    const XcJob j = jobs[blockIdx.x];
    const int tid = threadIdx.x;
    long long *rj = r + j.r_off;
    for (int t = j.n_mfma + tid; t < j.n_lags; t += kXcThreads) rj[t] = 0;
    if (j.n_mfma == 0) return;
    // s0 = sum_n a[w + n] + sum_n b[n]: the sliding sum of lag index 0, and the sum of b
    const long long s0 = xc_block_sum(xc_window_sum<false>(pcm, j, j.w) + xc_span_sum<false>(pcm + j.b0, j.len), red);
    // the sliding sum moves by a[w + u + len] - a[w + u] from lag index u to u + 1: every thread a run of lags, the runs'
    // totals scanned over the workgroup
    const int run = (j.n_mfma + kXcThreads - 1) / kXcThreads;
    const int ta = min(tid * run, j.n_mfma), tb = min(ta + run, j.n_mfma);
    long long d = 0;
    for (int u = ta; u < tb; ++u) d += xc_a(pcm, j, j.w + u + j.len) - xc_a(pcm, j, j.w + u);
    __syncthreads();
    red[tid] = d;
    __syncthreads();
    for (int o = 1; o < kXcThreads; o <<= 1) { // inclusive scan
        const long long v = tid >= o ? red[tid - o] : 0;
        __syncthreads();
        red[tid] += v;
        __syncthreads();
    }
    long long sa = s0 + red[tid] - d;
    for (int t = ta; t < tb; ++t) {
        rj[t] = 128 * (sa - 128 * j.len);
        sa += xc_a(pcm, j, j.w + t + j.len) - xc_a(pcm, j, j.w + t);
    }
}

// sample e of four -> byte e of a dword of each digit plane
__device__ __forceinline__ void xc_digits(int v, int e, unsigned &lo, unsigned &hi)
{
    lo |= (((unsigned)v & 255u) ^ 128u) << (8 * e);
    hi |= (((unsigned)v >> 8) & 255u) << (8 * e);
}

// one workgroup per part (items[blockIdx.x])
__global__ __launch_bounds__(kXcThreads, 2) void xcorr_mfma_kernel(const int16_t *__restrict__ pcm, const XcJob *__restrict__ jobs,
                                                                   const XcItem *__restrict__ items, unsigned long long *__restrict__ r)
{
    unsigned char *a_lo = xc_smem, *a_hi = a_lo + kXcABytes, *b_lo = a_hi + kXcABytes, *b_hi = b_lo + 2 * kXcBHalf;
    const XcItem it = items[blockIdx.x];
    const XcJob j = jobs[it.job];
    const int tid = threadIdx.x;
    const int mc = j.len - it.m0 < kXcChunk ? (int)(j.len - it.m0) : kXcChunk; // samples of the part
    const int steps = (mc + 31) / 32 + 31;
    // the window of a: plane byte x is sample w + t0 + m0 + x (the digits of 0 outside the operand)
    const int64_t wa = j.w + it.t0 + it.m0;
#pragma unroll 2
    for (int x = 8 * tid; x < steps * 32 + 64; x += 8 * kXcThreads) {
        const int64_t i0 = wa + x;
        unsigned lo[2] = {0, 0}, hi[2] = {0, 0};
        if (i0 >= 0 && i0 + 8 <= j.a_len) { // eight samples in one load (any 2-byte boundary)
            const xc_s8u v = *reinterpret_cast<const xc_s8u *>(pcm + j.a0 + i0);
#pragma unroll
            for (int e = 0; e < 8; ++e) xc_digits((int)v[e], e & 3, lo[e >> 2], hi[e >> 2]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) xc_digits(xc_a(pcm, j, i0 + e), e & 3, lo[e >> 2], hi[e >> 2]);
        }
        *reinterpret_cast<uint2 *>(a_lo + x) = make_uint2(lo[0], lo[1]);
        *reinterpret_cast<uint2 *>(a_hi + x) = make_uint2(hi[0], hi[1]);
    }
    // b: position y is sample m0 + y - 992 of the segment, zero DIGITS outside the part; 32 positions = an even and an odd unit
    const int16_t *b = pcm + j.b0 + it.m0;
#pragma unroll 2
    for (int y = 8 * tid; y < (steps + 31) * 32; y += 8 * kXcThreads) {
        const int m0 = y - 992;
        unsigned lo[2] = {0, 0}, hi[2] = {0, 0};
        if (m0 >= 0 && m0 + 8 <= mc) {
            const xc_s8u v = *reinterpret_cast<const xc_s8u *>(b + m0);
#pragma unroll
            for (int e = 0; e < 8; ++e) xc_digits((int)v[e], e & 3, lo[e >> 2], hi[e >> 2]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (m0 + e >= 0 && m0 + e < mc) xc_digits((int)b[m0 + e], e & 3, lo[e >> 2], hi[e >> 2]);
        }
        const int ad = ((y >> 4) & 1) * kXcBHalf + (y >> 5) * 16 + (y & 15);
        *reinterpret_cast<uint2 *>(b_lo + ad) = make_uint2(lo[0], lo[1]);
        *reinterpret_cast<uint2 *>(b_hi + ad) = make_uint2(hi[0], hi[1]);
    }
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6, li = lane & 31, h = lane >> 5;
    const unsigned sh = (unsigned)(li & 3);
    v16i acc0 = v16i{0}, acc1 = v16i{0}, acc2 = v16i{0};
    for (int s = wave; s < steps; s += 4) {
        // A: row li, sixteen bytes from plane byte 32 s + li + 16 h
        const int xa = (s * 32 + li + 16 * h) & ~3;
        const unsigned *pl = reinterpret_cast<const unsigned *>(a_lo + xa), *ph = reinterpret_cast<const unsigned *>(a_hi + xa);
        const unsigned l0 = pl[0], l1 = pl[1], l2 = pl[2], l3 = pl[3], l4 = pl[4];
        const unsigned h0 = ph[0], h1 = ph[1], h2 = ph[2], h3 = ph[3], h4 = ph[4];
        v4i al, ah;
        al[0] = (int)__builtin_amdgcn_alignbyte(l1, l0, sh);
        al[1] = (int)__builtin_amdgcn_alignbyte(l2, l1, sh);
        al[2] = (int)__builtin_amdgcn_alignbyte(l3, l2, sh);
        al[3] = (int)__builtin_amdgcn_alignbyte(l4, l3, sh);
        ah[0] = (int)__builtin_amdgcn_alignbyte(h1, h0, sh);
        ah[1] = (int)__builtin_amdgcn_alignbyte(h2, h1, sh);
        ah[2] = (int)__builtin_amdgcn_alignbyte(h3, h2, sh);
        ah[3] = (int)__builtin_amdgcn_alignbyte(h4, h3, sh);
        // B: column li, the unit of parity h of pair s - li (+ 31: the zeros in front)
        const int bi = h * kXcBHalf + (s - li + 31) * 16;
        const v4i bl = *reinterpret_cast<const v4i *>(b_lo + bi), bh = *reinterpret_cast<const v4i *>(b_hi + bi);
        acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(al, bl, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(al, bh, acc1, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(ah, bl, acc1, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(ah, bh, acc2, 0, 0, 0);
    }
    // the flush: the four waves' tiles in int64 through LDS (the planes are done with), one atomic per lag
    __syncthreads();
    long long *red = reinterpret_cast<long long *>(xc_smem);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int i = (reg & 3) + 8 * (reg >> 2) + 4 * h; // row of the tile; the lane's column is li
        red[wave * kXcRedStride + li * 33 + i] = (long long)acc0[reg] + 256ll * acc1[reg] + 65536ll * acc2[reg];
    }
    __syncthreads();
    for (int t = tid; t < kXcTile; t += kXcThreads) {
        const int at = (t >> 5) * 33 + (t & 31);
        const long long v = red[at] + red[kXcRedStride + at] + red[2 * kXcRedStride + at] + red[3 * kXcRedStride + at];
        if (it.t0 + t < j.n_lags) atomicAdd(r + j.r_off + it.t0 + t, (unsigned long long)v);
    }
}

// one workgroup per part: thread = lag index t0 + tid
__global__ __launch_bounds__(kXcValuLags) void xcorr_valu_kernel(const int16_t *__restrict__ pcm, const XcJob *__restrict__ jobs,
                                                                  const XcItem *__restrict__ items, unsigned long long *__restrict__ r)
{
    __shared__ int16_t a_s[kXcValuChunk + kXcValuLags], b_s[kXcValuChunk];
    const XcItem it = items[blockIdx.x];
    const XcJob j = jobs[it.job];
    const int tid = threadIdx.x;
    const int mc = j.len - it.m0 < kXcValuChunk ? (int)(j.len - it.m0) : kXcValuChunk;
    const int64_t wa = j.w + it.t0 + it.m0;
    for (int x = tid; x < mc + kXcValuLags - 1; x += kXcValuLags) a_s[x] = (int16_t)xc_a(pcm, j, wa + x);
    for (int x = tid; x < mc; x += kXcValuLags) b_s[x] = pcm[j.b0 + it.m0 + x];
    __syncthreads();
    long long acc = 0;
    for (int m = 0; m < mc; ++m) acc += (long long)((int)a_s[tid + m] * (int)b_s[m]); // |product| <= 2^30
    if (it.t0 + tid < j.n_lags) atomicAdd(r + j.r_off + it.t0 + tid, (unsigned long long)acc);
}

// (|r|, lag) a better peak than (|r|', lag')
__device__ __forceinline__ bool xc_better(unsigned long long m, int l, unsigned long long m2, int l2)
{
    if (m != m2) return m > m2;
    const int al = l < 0 ? -l : l, al2 = l2 < 0 ? -l2 : l2;
    if (al != al2) return al < al2;
    return l < l2;
}

// one workgroup per job
__global__ __launch_bounds__(kXcThreads) void xcorr_peak_kernel(const int16_t *__restrict__ pcm, const XcJob *__restrict__ jobs,
                                                                const long long *__restrict__ r, hpfw_xcorr_peak *__restrict__ peaks)
{
    __shared__ long long red[kXcThreads];
    __shared__ unsigned long long best_m[kXcThreads];
    __shared__ int best_l[kXcThreads];
    const XcJob j = jobs[blockIdx.x];
    const int tid = threadIdx.x, radius = (j.n_lags - 1) / 2;
    const long long *rj = r + j.r_off;
    unsigned long long bm = 0;
    int bl = 1 << 30; // (no lag: loses every tie)
    for (int t = tid; t < j.n_lags; t += kXcThreads) {
        const long long v = rj[t];
        const unsigned long long m = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
        if (xc_better(m, t - radius, bm, bl)) {
            bm = m;
            bl = t - radius;
        }
    }
    best_m[tid] = bm;
    best_l[tid] = bl;
    __syncthreads();
    for (int o = kXcThreads / 2; o >= 1; o >>= 1) {
        if (tid < o && xc_better(best_m[tid + o], best_l[tid + o], best_m[tid], best_l[tid])) {
            best_m[tid] = best_m[tid + o];
            best_l[tid] = best_l[tid + o];
        }
        __syncthreads();
    }
    const int lag = best_l[0];
    const long long ea = xc_block_sum(xc_window_sum<true>(pcm, j, j.w + radius + lag), red);
    const long long eb = xc_block_sum(xc_span_sum<true>(pcm + j.b0, j.len), red);
    if (tid == 0) peaks[blockIdx.x] = hpfw_xcorr_peak{rj[lag + radius], ea, eb, lag, 0};
}

} // namespace

void launch_xcorr(const int16_t *d_pcm, const XcJob *d_jobs, int64_t n_jobs, const XcItem *d_mfma, int64_t n_mfma,
                  const XcItem *d_valu, int64_t n_valu, int64_t *d_r, hpfw_xcorr_peak *d_peaks, hipStream_t s)
{
    if (n_jobs < 1) return;
    static PerDeviceOnce attr_set;
    if (attr_set.need()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(xcorr_mfma_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kXcLds);
        attr_set.mark();
    }
    hipLaunchKernelGGL(xcorr_init_kernel, dim3((unsigned)n_jobs), dim3(kXcThreads), 0, s, d_pcm, d_jobs, (long long *)d_r);
    if (n_mfma > 0)
        hipLaunchKernelGGL(xcorr_mfma_kernel, dim3((unsigned)n_mfma), dim3(kXcThreads), kXcLds, s, d_pcm, d_jobs, d_mfma,
                           (unsigned long long *)d_r);
    if (n_valu > 0)
        hipLaunchKernelGGL(xcorr_valu_kernel, dim3((unsigned)n_valu), dim3(kXcValuLags), 0, s, d_pcm, d_jobs, d_valu,
                           (unsigned long long *)d_r);
    if (d_peaks)
        hipLaunchKernelGGL(xcorr_peak_kernel, dim3((unsigned)n_jobs), dim3(kXcThreads), 0, s, d_pcm, d_jobs, (const long long *)d_r,
                           d_peaks);
}

} // namespace hpfw
