// k_merge.hip -- what a sharded search does with the gathered per-shard results: the device twins of
// hpfw_gpu_merge_topk and of the sum of the scored search's moments, and the merge of the voting search's per-shard neighbour
// lists (knn_merge_shards_kernel).
//
// topk_merge_shards_kernel: one workgroup per query.  Its n = n_shards k <= 4096 candidates in[shard][q][k] are 16-byte
// records with the key (dist, clip) in their first two words; the other two words are payload (hpfw_hit: offset, pad;
// hpfw_shift_hit: offset, shift_index) and travel with the record.  The candidates are sorted in LDS as 64-bit keys
// dist << 44 | clip << 12 | candidate index (dist < 2^20: queries of at most 16 000 hashprints; a larger word, which only
// the padding record dist = clip = 0xffffffff holds, saturates to 0xfffff), and output t is a 16-byte copy of the record
// key t names.  The candidate index i = shard k + rank is the position std::stable_sort starts from, so records of equal
// (dist, clip) -- the padding records -- come out in the order the host merge leaves them in, payload as found.  Integer
// work, vector loads and stores, no atomics.
//
// sum_stats_kernel: one thread per row, out[r] = sum over the shards of in[shard][r] (sum, sum_sq mod 2^64, n mod 2^32), pad 0.
#include "kernels.h"

namespace hpfw {

constexpr int kMsThreads = 256;
constexpr int kMsMax = 64 * 64;

static __device__ void merge_sort_lds(uint64_t *key, int np, int tid)
{
    for (int size = 2; size <= np; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < np; i += kMsThreads) {
                const int j = i ^ stride;
                if (j > i) {
                    const uint64_t a = key[i], b = key[j];
                    if ((a > b) == ((i & size) == 0)) {
                        key[i] = b;
                        key[j] = a;
                    }
                }
            }
            __syncthreads();
        }
}

__global__ __launch_bounds__(kMsThreads) void topk_merge_shards_kernel(const uint4 *__restrict__ in, int n_shards, long long n_q, int k,
                                                                       uint4 *__restrict__ out)
{
    __shared__ uint64_t key[kMsMax];
    const int tid = threadIdx.x, n = n_shards * k;
    const long long q = blockIdx.x;
    int np = 1;
    while (np < n) np <<= 1;
    for (int i = tid; i < np; i += kMsThreads) {
        uint64_t v = ~0ull; // the filler up to the power of two: behind every candidate
        if (i < n) {
            const int s = i / k, t = i - s * k;
            const uint4 r = in[((long long)s * n_q + q) * k + t];
            const uint64_t d = r.x < 0xfffffu ? r.x : 0xfffffu;
            v = (d << 44) | ((uint64_t)r.y << 12) | (uint64_t)i;
        }
        key[i] = v;
    }
    __syncthreads();
    merge_sort_lds(key, np, tid);
    for (int t = tid; t < k; t += kMsThreads) { // k <= n <= np: key[t] is a candidate
        const int i = (int)(key[t] & 4095), s = i / k;
        out[q * k + t] = in[((long long)s * n_q + q) * k + (i - s * k)];
    }
}

struct MergeStatsDev {
    unsigned long long sum, sum_sq;
    uint32_t n, pad;
};

__global__ __launch_bounds__(kMsThreads) void sum_stats_kernel(const MergeStatsDev *__restrict__ in, int n_shards, long long rows,
                                                               MergeStatsDev *__restrict__ out)
{
    const long long r = (long long)blockIdx.x * kMsThreads + threadIdx.x;
    if (r >= rows) return;
    MergeStatsDev acc{0, 0, 0, 0};
    for (int s = 0; s < n_shards; ++s) {
        const MergeStatsDev v = in[(long long)s * rows + r];
        acc.sum += v.sum;
        acc.sum_sq += v.sum_sq;
        acc.n += v.n;
    }
    out[r] = acc;
}

// the per-shard neighbour lists of the voting search: one thread per window.  Shards are contiguous blocks of clips, so a key
// with its shard's first position added is the key of the unsharded index, and the 5 smallest of the 5 n_shards keys, ties
// included, are the unsharded list.
struct KnnPosBase {
    long long v[64];
};

__global__ __launch_bounds__(kMsThreads) void knn_merge_shards_kernel(const uint64_t *__restrict__ in, KnnPosBase base, int n_shards,
                                                                      long long n_win, uint64_t *__restrict__ out)
{
    const long long w = (long long)blockIdx.x * kMsThreads + threadIdx.x;
    if (w >= n_win) return;
    uint64_t b0 = ~0ull, b1 = ~0ull, b2 = ~0ull, b3 = ~0ull, b4 = ~0ull;
    for (int s = 0; s < n_shards; ++s) {
        const uint64_t *row = in + ((long long)s * n_win + w) * 5;
        const uint64_t add = (uint64_t)base.v[s];
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            uint64_t c = row[r], t;
            if (c != ~0ull) c += add; // (the position field: below 2^40 with the base added)
            if (c < b0) { t = b0; b0 = c; c = t; }
            if (c < b1) { t = b1; b1 = c; c = t; }
            if (c < b2) { t = b2; b2 = c; c = t; }
            if (c < b3) { t = b3; b3 = c; c = t; }
            if (c < b4) b4 = c;
        }
    }
    uint64_t *o = out + w * 5;
    o[0] = b0;
    o[1] = b1;
    o[2] = b2;
    o[3] = b3;
    o[4] = b4;
}

void launch_knn_merge_shards(const uint64_t *d_in, const int64_t *pos_base, int n_shards, int64_t n_win, uint64_t *d_out, hipStream_t s)
{
    KnnPosBase base = {};
    for (int i = 0; i < n_shards && i < 64; ++i) base.v[i] = pos_base[i];
    hipLaunchKernelGGL(knn_merge_shards_kernel, dim3((unsigned)((n_win + kMsThreads - 1) / kMsThreads)), dim3(kMsThreads), 0, s, d_in, base,
                       n_shards, (long long)n_win, d_out);
}

void launch_topk_merge_shards(const void *d_in, int n_shards, int64_t n_q, int k, void *d_out, hipStream_t s)
{
    hipLaunchKernelGGL(topk_merge_shards_kernel, dim3((unsigned)n_q), dim3(kMsThreads), 0, s, static_cast<const uint4 *>(d_in), n_shards,
                       (long long)n_q, k, static_cast<uint4 *>(d_out));
}

void launch_sum_stats(const void *d_in, int n_shards, int64_t rows, void *d_out, hipStream_t s)
{
    hipLaunchKernelGGL(sum_stats_kernel, dim3((unsigned)((rows + kMsThreads - 1) / kMsThreads)), dim3(kMsThreads), 0, s,
                       static_cast<const MergeStatsDev *>(d_in), n_shards, (long long)rows, static_cast<MergeStatsDev *>(d_out));
}

} // namespace hpfw
