// k_votes.hip -- the tally of the voting search on the device (the rule: annoy_storage.h:41-63 of the
// reference, restated in include/hpfw_gpu.h).
//
// The events of a query are its real neighbour keys in stream order (window i ascending, rank r ascending).  An event at
// database position pos of clip c votes for bucket (c, off = i - (pos - db_off[c])).  Positions within a window are distinct,
// so a bucket's value is a sequential chain over its own events in window order, and because every vote is positive the
// running maximum of the literal loop is the prefix maximum of the post-event values: the winner is the event earliest in
// stream order whose post-event value is the largest of the query.
//
//   window_starts_kernel  one thread per window: where its 64 hashprints begin in the query array
//   sort_knn_slots_kernel one thread per window: the 5 keys knn_windows_kernel left unsorted in 8 slots -> [n_win][5] ascending
//   vote_events_kernel    one thread per event: sort key = query << ubits | u, with u = pos - i + stride (clip + 1) one number
//                         per bucket (stride = the most windows any query of the call has, so stride > every i and the
//                         ranges of consecutive clips do not meet); value = the event's stream index.  Padding keys sort behind a query's buckets (u = all ones).
//   (hipcub radix sort of the pairs: stable, so a bucket's events stay in window order)
//   vote_chain_kernel     one thread per run of equal sort keys: cnt = (float)((double)cnt + 1.0 / (double)(float)(d + 1))
//                         event by event, written to post[stream index]
//   vote_pick_kernel      one workgroup per query: arg-max of (post descending, stream index ascending) -> one hpfw_vote
//
// Integer work plus the chain arithmetic (a double add, a correctly rounded double division, a round to float: no fast-math
// flag reaches this file); vector loads and stores; no atomics, so nothing depends on scheduling.
#include <hipcub/hipcub.hpp>

#include "kernels.h"

namespace hpfw {

namespace {

constexpr int kVtThreads = 256;
constexpr uint64_t kNoKey = ~0ull;
constexpr uint64_t kPosMask = ((uint64_t)1 << 40) - 1;

// c into the ascending b0..b4, the largest of the six dropped (registers only)
__device__ __forceinline__ void insert5(uint64_t c, uint64_t &b0, uint64_t &b1, uint64_t &b2, uint64_t &b3, uint64_t &b4)
{
    uint64_t t;
    if (c < b0) { t = b0; b0 = c; c = t; }
    if (c < b1) { t = b1; b1 = c; c = t; }
    if (c < b2) { t = b2; b2 = c; c = t; }
    if (c < b3) { t = b3; b3 = c; c = t; }
    if (c < b4) b4 = c;
}

// the last index t in [0, n] with tab[t] <= v (tab ascending, tab[0] <= v)
__device__ __forceinline__ int64_t last_not_above(const int64_t *__restrict__ tab, int64_t n, int64_t v)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (tab[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kVtThreads) void window_starts_kernel(const int64_t *__restrict__ w_first, const int64_t *__restrict__ q_off,
                                                                    int n_q, int64_t w_base, int64_t n_win, int64_t *__restrict__ w_start)
{
    const int64_t w = (int64_t)blockIdx.x * kVtThreads + threadIdx.x;
    if (w >= n_win) return;
    const int64_t q = last_not_above(w_first, n_q - 1, w_base + w); // (queries without a window repeat a value: the last one holds w)
    w_start[w] = q_off[q] + (w_base + w - w_first[q]);
}

__global__ __launch_bounds__(kVtThreads) void sort_knn_slots_kernel(const ulonglong2 *__restrict__ slots, int64_t n_win,
                                                                     uint64_t *__restrict__ keys)
{
    const int64_t w = (int64_t)blockIdx.x * kVtThreads + threadIdx.x;
    if (w >= n_win) return;
    const ulonglong2 a = slots[w * 4], b = slots[w * 4 + 1], c = slots[w * 4 + 2]; // (slots 5..7 are never written)
    uint64_t b0 = kNoKey, b1 = kNoKey, b2 = kNoKey, b3 = kNoKey, b4 = kNoKey;
    insert5(a.x, b0, b1, b2, b3, b4);
    insert5(a.y, b0, b1, b2, b3, b4);
    insert5(b.x, b0, b1, b2, b3, b4);
    insert5(b.y, b0, b1, b2, b3, b4);
    insert5(c.x, b0, b1, b2, b3, b4);
    uint64_t *o = keys + w * 5;
    o[0] = b0;
    o[1] = b1;
    o[2] = b2;
    o[3] = b3;
    o[4] = b4;
}

__global__ __launch_bounds__(kVtThreads) void vote_events_kernel(VoteTallyArgs a)
{
    const int64_t e = (int64_t)blockIdx.x * kVtThreads + threadIdx.x;
    if (e >= a.n_win * 5) return;
    const int64_t w = a.w_base + e / 5;
    const int64_t q = last_not_above(a.w_first, a.n_q - 1, w);
    const uint64_t key = a.keys[e];
    const uint64_t u_pad = ((uint64_t)1 << a.ubits) - 1;
    uint64_t u = u_pad;
    if (key != kNoKey) {
        const int64_t pos = (int64_t)(key & kPosMask), i = w - a.w_first[q];
        const int64_t clip = last_not_above(a.db_off, a.n_clips - 1, pos);
        u = (uint64_t)(pos - i + a.stride * (clip + 1));
        u = u < u_pad ? u : u_pad - 1; // (a position outside the index: kept inside the query's field)
    }
    a.sort_keys[e] = ((uint64_t)q << a.ubits) | u;
    a.sort_vals[e] = (uint32_t)e;
    a.post[e] = 0.0f;
}

__global__ __launch_bounds__(kVtThreads) void vote_chain_kernel(const uint64_t *__restrict__ sorted_keys, const uint32_t *__restrict__ sorted_vals,
                                                                 int64_t n_ev, int ubits, const uint64_t *__restrict__ keys,
                                                                 float *__restrict__ post)
{
    const int64_t t = (int64_t)blockIdx.x * kVtThreads + threadIdx.x;
    if (t >= n_ev) return;
    const uint64_t mine = sorted_keys[t];
    if (t > 0 && sorted_keys[t - 1] == mine) return; // not the head of its run
    const uint64_t u_pad = ((uint64_t)1 << ubits) - 1;
    if ((mine & u_pad) == u_pad) return; // padding keys are not events
    float cnt = 0.0f;
    for (int64_t j = t; j < n_ev && sorted_keys[j] == mine; ++j) {
        const uint32_t idx = sorted_vals[j];
        const uint64_t d = keys[idx] >> 40;
        cnt = (float)((double)cnt + 1.0 / (double)(float)(d + 1)); // annoy_storage.h:53
        post[idx] = cnt;
    }
}

__global__ __launch_bounds__(kVtThreads) void vote_pick_kernel(VoteTallyArgs a)
{
    __shared__ uint64_t part[kVtThreads / 64];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int64_t w0 = a.w_first[q], w1 = a.w_first[q + 1];
    const int64_t e0 = (w0 - a.w_base) * 5, n = (w1 - w0) * 5;
    // (value, stream index) as one word: positive floats order as their bits, the earlier event is the larger low half
    uint64_t best = 0;
    for (int64_t e = tid; e < n; e += kVtThreads) {
        const uint64_t cand = ((uint64_t)__float_as_uint(a.post[e0 + e]) << 32) | (uint64_t)(0xffffffffu - (uint32_t)e);
        best = cand > best ? cand : best;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)best, s);
        best = o > best ? o : best;
    }
    if ((tid & 63) == 0) part[tid >> 6] = best;
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int i = 1; i < kVtThreads / 64; ++i) best = part[i] > best ? part[i] : best;
    hpfw_vote v = {0xffffffffu, 0, 0, 0.0f, 0.0f}; // annoy_storage.h:43
    if ((best >> 32) != 0) { // (a real event leaves a value above 0; padding leaves 0)
        const int64_t e = (int64_t)(0xffffffffu - (uint32_t)best);
        const uint64_t key = a.keys[e0 + e];
        const int64_t pos = (int64_t)(key & kPosMask), i = e / 5;
        const int64_t clip = last_not_above(a.db_off, a.n_clips - 1, pos);
        v.clip = a.clip_base + (uint32_t)clip;
        v.offset = i - (pos - a.db_off[clip]);
        v.cnt = __uint_as_float((uint32_t)(best >> 32));
    }
    a.out[q] = v;
}

} // namespace

void launch_window_starts(const int64_t *d_w_first, const int64_t *d_q_off, int n_q, int64_t w_base, int64_t n_win, int64_t *d_w_start,
                          hipStream_t s)
{
    hipLaunchKernelGGL(window_starts_kernel, dim3((unsigned)((n_win + kVtThreads - 1) / kVtThreads)), dim3(kVtThreads), 0, s, d_w_first, d_q_off,
                       n_q, w_base, n_win, d_w_start);
}

void launch_sort_knn_slots(const void *d_slots, int64_t n_win, uint64_t *d_keys, hipStream_t s)
{
    hipLaunchKernelGGL(sort_knn_slots_kernel, dim3((unsigned)((n_win + kVtThreads - 1) / kVtThreads)), dim3(kVtThreads), 0, s,
                       static_cast<const ulonglong2 *>(d_slots), n_win, d_keys);
}

size_t vote_sort_temp_bytes(int64_t n_ev, int bits)
{
    size_t tb = 0;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr,
                                           (uint32_t *)nullptr, (int)n_ev, 0, bits, nullptr) != hipSuccess)
        return 0;
    return std::max<size_t>(tb, 256);
}

hipError_t launch_vote_tally(const VoteTallyArgs &a, void *d_temp, size_t temp_bytes, hipStream_t s)
{
    const int64_t n_ev = a.n_win * 5;
    if (n_ev > 0 && a.n_clips > 0) {
        const unsigned grid = (unsigned)((n_ev + kVtThreads - 1) / kVtThreads);
        hipLaunchKernelGGL(vote_events_kernel, dim3(grid), dim3(kVtThreads), 0, s, a);
        const hipError_t e = hipcub::DeviceRadixSort::SortPairs(d_temp, temp_bytes, (const uint64_t *)a.sort_keys, a.sorted_keys,
                                                                (const uint32_t *)a.sort_vals, a.sorted_vals, (int)n_ev, 0, a.ubits + a.qbits, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(vote_chain_kernel, dim3(grid), dim3(kVtThreads), 0, s, (const uint64_t *)a.sorted_keys, (const uint32_t *)a.sorted_vals,
                           n_ev, a.ubits, a.keys, a.post);
    } else if (n_ev > 0) { // nothing indexed: no key is an event
        const hipError_t e = hipMemsetAsync(a.post, 0, (size_t)n_ev * 4, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(vote_pick_kernel, dim3((unsigned)a.n_q), dim3(kVtThreads), 0, s, a);
    return hipSuccess;
}

} // namespace hpfw
