/*
 * hpfw_gpu_multi_search.h -- the key, tempo and scored searches and the windows of one recording over a sharded index
 * (libhpfw_gpu_multi.so).
 *
 * Kept beside include/hpfw_gpu_multi.h rather than in it: that header's symbol set is fixed (tests/test_library.py
 * checks it against hpfw_amd.multi.EXPORTS), and this is an addition to it (hpfw_amd.multi.SEARCH_EXPORTS).
 *
 * Every search here equals the one-handle function of the same name (include/hpfw_gpu.h) on the unsharded index, field
 * for field, at any number of shards: clips are disjoint across the shards, a shard's transposed search already took each
 * of its clips' minimum over the variant sets before its top-k, so the global top-k by (dist, clip) is the merge of the
 * per-shard lists, shift_index included; and a row of moments is the sum of the shards' rows (exact integers).
 * Replicated queries -> per-shard search -> ONE ncclAllGather of the per-shard hits and moments -> merge and sum on
 * device 0 (hpfw_gpu_merge_topk_device, hpfw_gpu_sum_stats_device) -> one copy of n_q k hits and the rows of moments back.
 * All pointers are HOST pointers.  Bad k, bad n_shifts and null stats are refused with the statuses and messages of the
 * one-handle functions before any device is touched.
 */
#ifndef HPFW_GPU_MULTI_SEARCH_H
#define HPFW_GPU_MULTI_SEARCH_H

#include "hpfw_gpu_multi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hpfw_gpu_search_topk_scored: out [n_q][k], stats [n_q].  The bound n_clips * k_max^2 * 4096 < 2^64 is checked with the
 * GROUP's clip count (HPFW_E_UNSUPPORTED): the sum over the shards must not wrap either. */
int hpfw_gpu_group_search_topk_scored(hpfw_gpu_group *g, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int k,
                                      hpfw_hit *out, hpfw_dist_stats *stats);
/* hpfw_gpu_search_topk_transposed: q_off [n_q * n_shifts + 1], out [n_q][k] */
int hpfw_gpu_group_search_topk_transposed(hpfw_gpu_group *g, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q,
                                          int n_shifts, int k, hpfw_shift_hit *out);
/* hpfw_gpu_search_topk_transposed_scored: stats [n_q][n_shifts] */
int hpfw_gpu_group_search_topk_transposed_scored(hpfw_gpu_group *g, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q,
                                                 int n_shifts, int k, hpfw_shift_hit *out, hpfw_dist_stats *stats);
/* hpfw_gpu_extract_windows_pcm16_host with the windows sharded contiguously (hpfw_gpu_shard_range over the window count):
 * shard s extracts its windows [lo, hi) from the samples [lo hop, (hi - 1) hop + win) and writes its rows of hp; no
 * collective.  hp as the one-handle call gives it, bit for bit; its argument checks and its requirement of projection
 * mode 1 for tempos and shifts are made once up front, on shard 0's handle. */
int hpfw_gpu_group_extract_windows_pcm16(hpfw_gpu_group *g, const int16_t *pcm, int64_t n_total, int64_t win, int64_t hop,
                                         const float *tempos, int n_tempos, const int32_t *shifts, int n_shifts, uint64_t *hp);

#ifdef __cplusplus
}
#endif
#endif
