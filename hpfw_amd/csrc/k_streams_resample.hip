// k_streams_resample.hip -- live feeds at another rate than 44.1 kHz: the chunks of one push go through
// the polyphase filter of k_resample.hip on their way into the rings.  A feed that has received n input samples has been
// given the outputs y[0 .. emitted(n)) of the offline conversion of everything pushed to it (streams_plan.h): output m reads
// inputs floor(m M / L) - H + 1 .. floor(m M / L) + H, so the outputs a push completes read the chunk and at most the T - 1
// samples in front of it, which the feed keeps as its history.
//
//   ring_resample_append_kernel   every feed of one push that is at one rate.  blockIdx.y is the feed's run (RingRsRun),
//                                 blockIdx.x a group of kRsPasses passes of kRsTile outputs counted from the run's first.  A pass
//                                 stages its input span from the run's virtual source -- zeros in front of the feed's first
//                                 sample and behind the chunk, the history, the chunk -- and then is resample_kernel's pass:
//                                 the same table image, the same products (rs_output).  Output m goes to ring position
//                                 m mod capacity.  Workgroup 0 of a run also writes the feed's next history, the last T - 1
//                                 samples of (history, chunk), into the feed's other history buffer: nothing of this launch
//                                 reads what it writes, and a run that completes no output still has that workgroup.
#include <algorithm>

#include "kernels.h"
#include "resample_dev.h"

namespace hpfw {

namespace {

struct RingRsArgs {
    const RingRsRun *runs;
    const int16_t *src; // the staged chunks
    int16_t *slab;
    int16_t *hist;
    const int4 *taps;        // [L][rw / 4]
    uint32_t L, M, H, rw;    // rw: words per table row (multiple of 4)
    uint32_t step_q, step_r; // (256 M) / L, (256 M) % L: one lane's step from output d to d + 256
};

// input sample g of the feed as this push sees it; t1 = T - 1
__device__ __forceinline__ int16_t feed_sample(const RingRsRun &r, const int16_t *__restrict__ hist, const int16_t *__restrict__ chunk,
                                               int64_t t1, int64_t g)
{
    if (g < 0 || g >= r.n_old + r.count) return 0;
    if (g >= r.n_old) return chunk[g - r.n_old];
    const int64_t j = g - (r.n_old - t1);
    return j >= 0 ? hist[j] : 0;
}

template <bool kTabLds>
__global__ __launch_bounds__(kRsThreads) void ring_resample_append_kernel(RingRsArgs a)
{
    extern __shared__ __align__(16) unsigned char ring_rs_smem[];
    const RingRsRun r = a.runs[blockIdx.y];
    const int64_t tile0 = (int64_t)blockIdx.x * kRsPasses * kRsTile; // the group's first output, counted from m0
    if (blockIdx.x && tile0 >= r.m1 - r.m0) return;
    const int16_t *chunk = a.src + r.src, *hist = a.hist + r.hist_rd;
    const int64_t t1 = 2 * (int64_t)a.H - 1;
    if (blockIdx.x == 0) {
        int16_t *next = a.hist + r.hist_wr;
        for (int j = threadIdx.x; j < (int)t1; j += kRsThreads) next[j] = feed_sample(r, hist, chunk, t1, r.n_old + r.count - t1 + j);
    }
    const int tab_words = kTabLds ? (int)(a.L * a.rw) : 0;
    const int4 *tab = a.taps;
    if (kTabLds) {
        int4 *t = reinterpret_cast<int4 *>(ring_rs_smem);
        for (int i = threadIdx.x; i < tab_words / 4; i += kRsThreads) t[i] = a.taps[i];
        tab = t;
    }
    int16_t *s = reinterpret_cast<int16_t *>(ring_rs_smem + (size_t)tab_words * 4);
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(s);
    const int chunks = (int)(a.rw / 4);
    const int64_t h0 = r.n_old - t1 < 0 ? 0 : r.n_old - t1; // the history holds inputs [h0, n_old)
    for (int pass = 0; pass < kRsPasses; ++pass) {
        const int64_t m0 = r.m0 + tile0 + (int64_t)pass * kRsTile;
        if (m0 >= r.m1) break;
        // 64-bit absolute positions: a feed runs for days
        const uint64_t q0 = (uint64_t)m0 * a.M;
        const int64_t i0b = (int64_t)(q0 / a.L);
        const uint32_t pb = (uint32_t)(q0 % a.L);
        const int64_t m_last = (m0 + kRsTile < r.m1 ? m0 + kRsTile : r.m1) - 1;
        const int span = (int)((uint64_t)m_last * a.M / a.L - i0b) + (int)a.rw * 2 + 2;
        const int64_t lo = i0b - (int64_t)a.H + 1;
        __syncthreads(); // (the previous pass is done with s)
        stage_span(chunk, r.count, lo - r.n_old, span, s); // the chunk, zeros around it
        // ... and the history over the zeros in front of it (slot j is written by lane j mod 256 both times)
        const int64_t j0 = h0 - lo, j1 = r.n_old - lo < span ? r.n_old - lo : span;
        for (int64_t j = threadIdx.x; j < j1; j += kRsThreads)
            if (j >= j0) s[j] = hist[lo + j - (r.n_old - t1)];
        __syncthreads();
        // output d = lane + 256 i of the pass: first tap's sample k = i0 - i0b, phase p, in 32-bit steps
        const uint32_t t0 = pb + (uint32_t)threadIdx.x * a.M; // < 2^32: lane < 256, M < 2^24, pb < L
        uint32_t k = t0 / a.L, p = t0 - k * a.L;
        for (int i = 0; i < kRsPerLane; ++i) {
            const int64_t m = m0 + threadIdx.x + (int64_t)i * kRsThreads;
            if (m < r.m1) {
                const int64_t j = m - r.m0;
                a.slab[r.base + (j < r.first ? r.pos0 + j : j - r.first)] = rs_output(sw, k, tab + (size_t)p * chunks, chunks);
            }
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

// runs [n_runs] (device): the feeds of one push at the rate of (L, M, T); most: the most outputs of one run.  d_taps:
// resample_device_table's image.  Returns false when the launch configuration is impossible.
bool launch_ring_resample_append(const RingRsRun *d_runs, int n_runs, int64_t most, const int16_t *d_src, int16_t *d_slab, int16_t *d_hist,
                                 int32_t L, int32_t M, int32_t T, const int32_t *d_taps, hipStream_t s)
{
    if (n_runs == 0) return true;
    RingRsArgs a;
    a.runs = d_runs;
    a.src = d_src;
    a.slab = d_slab;
    a.hist = d_hist;
    a.taps = reinterpret_cast<const int4 *>(d_taps);
    a.L = (uint32_t)L;
    a.M = (uint32_t)M;
    a.H = (uint32_t)(T / 2);
    a.rw = (uint32_t)resample_row_words(T);
    const uint64_t step = (uint64_t)kRsThreads * (uint64_t)M;
    a.step_q = (uint32_t)(step / (uint64_t)L);
    a.step_r = (uint32_t)(step % (uint64_t)L);
    const size_t sample_bytes = (size_t)rs_span_cap(L, M, a.rw) * 2, tab_bytes = (size_t)L * a.rw * 4;
    const bool tab_lds = tab_bytes + sample_bytes <= kRsLdsMax;
    const size_t lds = sample_bytes + (tab_lds ? tab_bytes : 0);
    if (lds > kRsLdsMax) return false;
    const int64_t per_block = (int64_t)kRsTile * kRsPasses;
    const dim3 grid((unsigned)std::max<int64_t>(1, (most + per_block - 1) / per_block), (unsigned)n_runs);
    if (tab_lds)
        hipLaunchKernelGGL(ring_resample_append_kernel<true>, grid, dim3(kRsThreads), lds, s, a);
    else
        hipLaunchKernelGGL(ring_resample_append_kernel<false>, grid, dim3(kRsThreads), lds, s, a);
    return true;
}

} // namespace hpfw
