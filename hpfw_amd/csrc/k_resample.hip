// k_resample.hip -- sample-rate conversion of int16 PCM from an integer rate fs in [8 000, 192 000] to 44 100 Hz
// (essentia MonoLoader's resampling, reference include/hpfw/spectrum/cqt.h:45-47, mel.h:42-44, as an exact integer
// polyphase filter; DESIGN.md section 10 states the contract, tests/resample_ref.py restates it in numpy).
//
//   resample_design     host, float64: the [L][T] int16 table, every phase summing to exactly 2^14
//   resample_kernel     one workgroup = up to kPasses passes of kTile consecutive outputs of one clip.  A pass stages
//                       its input span in LDS (16-byte loads where the span is aligned, zeros outside the clip), then
//                       lane l computes outputs l, l + 256, ... of the pass: T int16 products per output on
//                       v_dot2_i32_i16, sample pairs realigned with v_alignbit_b32 when the first tap's sample is odd.
//                       The taps live in LDS when they fit beside the samples (staged once per workgroup), else they
//                       are read from device memory.  What it shares with the kernel of live feeds (the staging, one
//                       output's products) is in resample_dev.h.
#include <cmath>
#include <algorithm>
#include <numeric>

#include "kernels.h"
#include "resample_dev.h"

namespace hpfw {

namespace {

double bessel_i0(double x)
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

bool resample_ratio(int rate, int32_t *L, int32_t *M, int32_t *H)
{
    if (rate < kRsRateMin || rate > kRsRateMax) return false;
    const int g = std::gcd(kRsRateOut, rate);
    *L = kRsRateOut / g;
    *M = rate / g;
    *H = (int32_t)((10ll * 16 * std::max(*L, *M) + 9ll * *L - 1) / (9ll * *L)); // ceil(Z max(1, M / L) / rho), rho = 9 / 10
    return true;
}

int64_t resample_out_length(int64_t n_in, int32_t L, int32_t M) { return (n_in * L + M - 1) / M; }

bool resample_design(int rate, std::vector<int16_t> &taps, int32_t *L_out, int32_t *M_out, int32_t *T_out)
{
    int32_t L, M, H;
    if (!resample_ratio(rate, &L, &M, &H)) return false;
    const int T = 2 * H;
    const double fc = 0.9 * std::min(1.0, (double)L / M), beta = 8.0, i0b = bessel_i0(beta);
    taps.assign((size_t)L * T, 0);
    std::vector<double> h((size_t)T);
    for (int p = 0; p < L; ++p) {
        double sum = 0.0;
        for (int j = 0; j < T; ++j) {
            const double tau = (double)j - H + 1 - (double)p / L, r = tau / H;
            const double x = fc * tau, px = M_PI * (x == 0.0 ? 1.0e-20 : x);
            h[(size_t)j] = fc * (std::sin(px) / px) * bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
            sum += h[(size_t)j];
        }
        int64_t total = 0, l1 = 0;
        int16_t *row = taps.data() + (size_t)p * T;
        std::vector<int64_t> q((size_t)T);
        for (int j = 0; j < T; ++j) {
            q[(size_t)j] = (int64_t)std::nearbyint(h[(size_t)j] / sum * (double)(1 << kRsShift));
            total += q[(size_t)j];
        }
        q[(size_t)(H - 1)] += ((int64_t)1 << kRsShift) - total; // every phase sums to exactly 2^14
        for (int j = 0; j < T; ++j) {
            if (q[(size_t)j] < -32768 || q[(size_t)j] > 32767) return false;
            row[j] = (int16_t)q[(size_t)j];
            l1 += std::abs(q[(size_t)j]);
        }
        if (32768 * l1 >= ((int64_t)1 << 31)) return false; // the int32 accumulator cannot overflow
    }
    *L_out = L;
    *M_out = M;
    *T_out = T;
    return true;
}

int resample_row_words(int T) { return (T + 7) / 8 * 4; } // a row padded with zero taps to whole 16-byte chunks

// device image of the table: [L][resample_row_words(T)] words, two taps per word (tap 2i in the low half)
std::vector<int32_t> resample_device_table(const std::vector<int16_t> &taps, int32_t L, int32_t T)
{
    const int rw = resample_row_words(T);
    std::vector<int32_t> img((size_t)L * rw, 0);
    for (int32_t p = 0; p < L; ++p)
        for (int32_t j = 0; j < T; ++j) {
            const uint32_t v = (uint16_t)taps[(size_t)p * T + j];
            img[(size_t)p * rw + j / 2] |= (int32_t)(v << (16 * (j & 1)));
        }
    return img;
}

namespace {

struct RsArgs {
    const int16_t *in;
    int16_t *out;
    const int4 *taps; // [L][rw / 4]
    int64_t n_in, n_out;
    uint32_t L, M, H, rw;  // rw: words per table row (multiple of 4)
    uint32_t step_q, step_r; // (256 M) / L, (256 M) % L: one lane's step from output d to d + 256
    uint32_t span_cap;     // int16 slots of the sample buffer in LDS
};

template <bool kTabLds>
__global__ __launch_bounds__(kRsThreads) void resample_kernel(RsArgs a)
{
    extern __shared__ __align__(16) unsigned char rs_smem[];
    const int64_t clip = blockIdx.y;
    const int16_t *x = a.in + clip * a.n_in;
    int16_t *y = a.out + clip * a.n_out;
    const int tab_words = kTabLds ? (int)(a.L * a.rw) : 0;
    const int4 *tab = a.taps;
    if (kTabLds) {
        int4 *t = reinterpret_cast<int4 *>(rs_smem);
        for (int i = threadIdx.x; i < tab_words / 4; i += kRsThreads) t[i] = a.taps[i];
        tab = t;
    }
    int16_t *s = reinterpret_cast<int16_t *>(rs_smem + (size_t)tab_words * 4);
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(s);
    const int chunks = (int)(a.rw / 4);
    for (int pass = 0; pass < kRsPasses; ++pass) {
        const int64_t m0 = ((int64_t)blockIdx.x * kRsPasses + pass) * kRsTile;
        if (m0 >= a.n_out) break;
        // 64-bit tile base: m M passes 2^32 for long clips at rates with a large M
        const uint64_t q0 = (uint64_t)m0 * a.M;
        const int64_t i0b = (int64_t)(q0 / a.L);
        const uint32_t pb = (uint32_t)(q0 % a.L);
        const int64_t m_last = (m0 + kRsTile < a.n_out ? m0 + kRsTile : a.n_out) - 1;
        const int span = (int)((uint64_t)m_last * a.M / a.L - i0b) + (int)a.rw * 2 + 2;
        __syncthreads(); // (the previous pass is done with s)
        stage_span(x, a.n_in, i0b - (int64_t)a.H + 1, span, s);
        __syncthreads();
        // output d = lane + 256 r of the pass: first tap's sample k = i0 - i0b, phase p, in 32-bit steps
        const uint32_t t0 = pb + (uint32_t)threadIdx.x * a.M; // < 2^32: lane < 256, M < 2^24, pb < L
        uint32_t k = t0 / a.L, p = t0 - k * a.L;
        for (int r = 0; r < kRsPerLane; ++r) {
            const int64_t m = m0 + threadIdx.x + (int64_t)r * kRsThreads;
            if (m < a.n_out) y[m] = rs_output(sw, k, tab + (size_t)p * chunks, chunks);
            k += a.step_q;
            p += a.step_r;
            if (p >= a.L) {
                p -= a.L;
                ++k;
            }
        }
    }
}

} // namespace

// d_taps: resample_device_table's image on the device.  Returns false when the launch configuration is impossible.
bool launch_resample(const int16_t *d_in, int64_t n_in, int64_t n_clips, int32_t L, int32_t M, int32_t T, const int32_t *d_taps,
                     int16_t *d_out, hipStream_t s)
{
    const int64_t n_out = resample_out_length(n_in, L, M);
    if (n_clips <= 0 || n_out <= 0) return true;
    RsArgs a;
    a.in = d_in;
    a.out = d_out;
    a.taps = reinterpret_cast<const int4 *>(d_taps);
    a.n_in = n_in;
    a.n_out = n_out;
    a.L = (uint32_t)L;
    a.M = (uint32_t)M;
    a.H = (uint32_t)(T / 2);
    a.rw = (uint32_t)resample_row_words(T);
    const uint64_t step = (uint64_t)kRsThreads * (uint64_t)M;
    a.step_q = (uint32_t)(step / (uint64_t)L);
    a.step_r = (uint32_t)(step % (uint64_t)L);
    a.span_cap = rs_span_cap(L, M, a.rw);
    const size_t sample_bytes = (size_t)a.span_cap * 2, tab_bytes = (size_t)L * a.rw * 4;
    const bool tab_lds = tab_bytes + sample_bytes <= kRsLdsMax;
    const size_t lds = sample_bytes + (tab_lds ? tab_bytes : 0);
    if (lds > 160 * 1024) return false;
    static PerDeviceOnce attr_set;
    if (attr_set.need()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(resample_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  160 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(resample_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  160 * 1024);
        attr_set.mark();
    }
    const int64_t per_block = (int64_t)kRsTile * kRsPasses;
    const unsigned gx = (unsigned)((n_out + per_block - 1) / per_block);
    for (int64_t c0 = 0; c0 < n_clips; c0 += 65535) {
        const unsigned gy = (unsigned)std::min<int64_t>(65535, n_clips - c0);
        RsArgs b = a;
        b.in = d_in + c0 * n_in;
        b.out = d_out + c0 * n_out;
        if (tab_lds)
            hipLaunchKernelGGL(resample_kernel<true>, dim3(gx, gy), dim3(kRsThreads), lds, s, b);
        else
            hipLaunchKernelGGL(resample_kernel<false>, dim3(gx, gy), dim3(kRsThreads), lds, s, b);
    }
    return true;
}

} // namespace hpfw
