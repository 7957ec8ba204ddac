/*
 * hpfw_gpu_multi_votes.h -- the voting search (AnnStorage::find with exact neighbours, include/hpfw_gpu.h) over a sharded
 * index (libhpfw_gpu_multi.so; DESIGN.md sections 6.1 and 19).
 *
 * Kept beside include/hpfw_gpu_multi.h and include/hpfw_gpu_multi_search.h rather than in them: their symbol sets are fixed
 * (tests/test_library.py, tests/test_multi_search_host.py), and this is an addition (hpfw_amd.multi.VOTES_EXPORTS).
 *
 * The result equals hpfw_gpu_search_votes_device on the unsharded index, field for field, at any number of shards, a shard
 * without a clip of 64 hashprints included: shards are contiguous blocks of clips, so a shard's neighbour key with the
 * hashprints of the earlier shards added to its position is the unsharded key, and the 5 smallest of the shards' 5 n_shards
 * keys of a window are the unsharded 5, ties included.
 * Replicated queries -> per-shard hpfw_gpu_knn_windows_device -> ONE ncclAllGather of the per-shard key lists -> on device 0
 * hpfw_gpu_merge_knn_device and hpfw_gpu_vote_windows_device against the offsets of the whole index (kept on device 0,
 * uploaded by the first voting search after a build) -> one copy of n_q votes back.
 * The tally reads the offsets hpfw_gpu_group_index_build recorded and hpfw_gpu_group_index_remove
 * (include/hpfw_gpu_multi_index.h) keeps up to date: the index has to be built through the one and maintained through the
 * other.  Clips added to or removed from a shard's own handle (hpfw_gpu_group_handle) are not known to the group, and the
 * votes would be counted against stale offsets without an error.  A group holds at most 64 shards (hpfw_gpu_group_create), which is also
 * what hpfw_gpu_merge_knn_device takes.
 * All pointers are HOST pointers.
 */
#ifndef HPFW_GPU_MULTI_VOTES_H
#define HPFW_GPU_MULTI_VOTES_H

#include "hpfw_gpu_multi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hpfw_gpu_search_votes: out [n_q]; clip ids are global */
int hpfw_gpu_group_search_votes(hpfw_gpu_group *g, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, hpfw_vote *out);

#ifdef __cplusplus
}
#endif
#endif
