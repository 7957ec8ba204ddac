// k_stats.hip -- the scored searches' second readers of the (query, clip) tables: dist_stats_kernel for the plain search
// (DESIGN.md section 13), overlap_stats_kernel for the overlap search (section 18, above its launch below).
//
// The scan leaves best[q][clip] = dist << 32 | offset; the top-k kernels pick the winners.  dist_stats_kernel reads the
// same table once more and writes, per query row, the integer moments n, sum d, sum d^2 of the per-clip best distances
// over the COUNTED clips: those at least as long as the query (a shorter clip is compared over fewer hashprints,
// storage.h:37-39, so its distance is on another scale).  Integer sums do not depend on their order: the result is bitwise
// deterministic however the row is split.  d <= 64 * 16000 < 2^20; the host refuses calls whose sum of squares could
// pass 2^64 (search.hip).  No floating point.
//
// Grid (n_q, slices): slice g of row q takes clips [g per, (g + 1) per).  Lanes stride the slice (coalesced 8-byte loads of
// the table, 8-byte loads of db_off served by the cache: neighbouring lanes share all but one word), the three sums are
// reduced over the wave by shuffles, over the workgroup through LDS, and thread 0 adds the slice to the row with vector
// atomics on the 64-bit words (the row is zeroed by the host before the launch).
#include "kernels.h"
#include "overlap_rule.h"

namespace hpfw {

struct DistStatsDev {
    unsigned long long sum, sum_sq;
    uint32_t n, pad;
};

constexpr int kStThreads = 256;

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// the threads' moments summed over the workgroup (wave shuffles, then LDS) and added to row q by thread 0
__device__ __forceinline__ void add_moments(unsigned long long n, unsigned long long sum, unsigned long long sum_sq, DistStatsDev *stats, int q)
{
    __shared__ unsigned long long red[3][kStThreads / 64];
    const int tid = threadIdx.x;
    n = wave_sum_u64(n);
    sum = wave_sum_u64(sum);
    sum_sq = wave_sum_u64(sum_sq);
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = n;
        red[1][tid >> 6] = sum;
        red[2][tid >> 6] = sum_sq;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kStThreads / 64; ++w) {
            n += red[0][w];
            sum += red[1][w];
            sum_sq += red[2][w];
        }
        if (n) {
            atomicAdd(&stats[q].sum, sum);
            atomicAdd(&stats[q].sum_sq, sum_sq);
            atomicAdd(&stats[q].n, (uint32_t)n);
        }
    }
}

// SET: column c of the table is slot set[c] of db_off (search within a set)
template <bool SET>
__global__ __launch_bounds__(kStThreads) void dist_stats_kernel(const uint64_t *__restrict__ best, const int64_t *__restrict__ db_off,
                                                                const int64_t *__restrict__ q_off, int n_clips, int per,
                                                                const int32_t *__restrict__ set, DistStatsDev *__restrict__ stats)
{
    const int tid = threadIdx.x, q = blockIdx.x;
    const int64_t kq = q_off[q + 1] - q_off[q];
    if (kq < 1) return; // an empty query counts nothing (uniform over the workgroup)
    const int c0 = blockIdx.y * per, c1 = min(n_clips, c0 + per);
    const uint64_t *row = best + (int64_t)q * n_clips;
    unsigned long long n = 0, sum = 0, sum_sq = 0;
    for (int c = c0 + tid; c < c1; c += kStThreads) {
        int len;
        (void)clip_span<SET>(db_off, set, c, len);
        if (len < kq) continue;
        const unsigned long long d = row[c] >> 32;
        n += 1;
        sum += d;
        sum_sq += d * d;
    }
    add_moments(n, sum, sum_sq, stats, q);
}

// The scored overlap search's second reader: the table of k_search_overlap.hip after
// overlap_select_kernel has folded a clip's splits into its first entry {dist, L, lag, 0}.  Per query row the moments of
// rate = floor(dist 2^10 / L) over the clips that have a candidate and are not the row's excluded clip.  dist <= 64 L and
// L <= 16000: the numerator is below 2^30 (one 32-bit division), rate <= 2^16, and the sum of squares of fewer than 2^31
// clips stays below 2^63 -- nothing can wrap.  Grid and reduction as dist_stats_kernel's.
__global__ __launch_bounds__(kStThreads) void overlap_stats_kernel(const uint4 *__restrict__ tab, int n_clips, int splits,
                                                                   const int32_t *__restrict__ exclude, int per,
                                                                   DistStatsDev *__restrict__ stats)
{
    const int tid = threadIdx.x, q = blockIdx.x;
    const int c0 = blockIdx.y * per, c1 = min(n_clips, c0 + per);
    const uint4 *row = tab + (int64_t)q * n_clips * splits;
    const int ex = exclude ? exclude[q] : -1;
    unsigned long long n = 0, sum = 0, sum_sq = 0;
    for (int c = c0 + tid; c < c1; c += kStThreads) {
        const uint4 e = row[(int64_t)c * splits];
        if (overlap_no_entry(e) || c == ex) continue; // no candidate, or left out
        const unsigned long long r = (e.x << kOverlapRateBits) / e.y;
        n += 1;
        sum += r;
        sum_sq += r * r;
    }
    add_moments(n, sum, sum_sq, stats, q);
}

void launch_overlap_stats(const void *d_tab, int n_q, int n_clips, int splits, const int32_t *d_exclude, void *d_stats, hipStream_t s)
{
    const int slices = overlap_stats_slices(n_clips);
    const int per = (n_clips + slices - 1) / slices;
    hipLaunchKernelGGL(overlap_stats_kernel, dim3(n_q, slices), dim3(kStThreads), 0, s, static_cast<const uint4 *>(d_tab), n_clips, splits,
                       d_exclude, per, static_cast<DistStatsDev *>(d_stats));
}

void launch_dist_stats(const uint64_t *d_best, const int64_t *d_db_off, const int64_t *d_q_off, int n_q, int n_clips, void *d_stats,
                       hipStream_t s, const int32_t *d_set)
{
    // a slice of at least 4096 clips per workgroup (16 loads per lane); at most 64 slices, as the two-step top-k cuts a row
    const int slices = std::max(1, std::min(64, n_clips / 4096));
    const int per = (n_clips + slices - 1) / slices;
    if (d_set)
        hipLaunchKernelGGL(dist_stats_kernel<true>, dim3(n_q, slices), dim3(kStThreads), 0, s, d_best, d_db_off, d_q_off, n_clips, per,
                           d_set, static_cast<DistStatsDev *>(d_stats));
    else
        hipLaunchKernelGGL(dist_stats_kernel<false>, dim3(n_q, slices), dim3(kStThreads), 0, s, d_best, d_db_off, d_q_off, n_clips, per,
                           d_set, static_cast<DistStatsDev *>(d_stats));
}

} // namespace hpfw
