// k_within.hip -- search within sets: what regroups a call's queries by set and puts the results back.
//
// The scans, the top-k and the moments of a set are the SET instantiations of the kernels of k_search.hip, k_search_mfma.hip
// and k_stats.hip (kernels.h clip_span).  They take the queries of one set as a dense range, so the host orders the call's
// queries by set (stable), within_gather_kernel copies their hashprints into that order, and within_scatter_kernel writes
// the rows of hits and of moments back to the caller's order.  Pure copies: every destination word has one writer.
#include "kernels.h"

namespace hpfw {

// one workgroup per query i: dst[dst_off[i] + j] = src[src_off[i] + j], j < dst_off[i + 1] - dst_off[i]
__global__ __launch_bounds__(256) void within_gather_kernel(const uint64_t *__restrict__ src, const int64_t *__restrict__ src_off,
                                                            const int64_t *__restrict__ dst_off, uint64_t *__restrict__ dst)
{
    const int64_t i = blockIdx.x;
    const int64_t d0 = dst_off[i], len = dst_off[i + 1] - d0, s0 = src_off[i];
    for (int64_t j = threadIdx.x; j < len; j += 256) dst[d0 + j] = src[s0 + j];
}

// rows of `words` words: out[perm[r]][w] = in[r][w]; thread = one word of the n * words
__global__ __launch_bounds__(256) void within_scatter_kernel(const uint64_t *__restrict__ in, const int64_t *__restrict__ perm,
                                                             int64_t total, int words, uint64_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t r = i / words;
    out[perm[r] * words + (i - r * words)] = in[i];
}

void launch_within_gather(const uint64_t *d_src, const int64_t *d_src_off, const int64_t *d_dst_off, int64_t n, uint64_t *d_dst, hipStream_t s)
{
    if (n > 0) hipLaunchKernelGGL(within_gather_kernel, dim3((unsigned)n), dim3(256), 0, s, d_src, d_src_off, d_dst_off, d_dst);
}

void launch_within_scatter(const uint64_t *d_in, const int64_t *d_perm, int64_t n, int words, uint64_t *d_out, hipStream_t s)
{
    const int64_t total = n * words;
    if (total > 0)
        hipLaunchKernelGGL(within_scatter_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d_in, d_perm, total, words, d_out);
}

} // namespace hpfw
