/*
 * hpfw_gpu_multi_index.h -- maintenance of a sharded index (libhpfw_gpu_multi.so; DESIGN.md sections 6.1 and 21).
 *
 * Kept beside include/hpfw_gpu_multi.h rather than in it: its symbol set is fixed (tests/test_library.py), and this is an
 * addition (hpfw_amd.multi.INDEX_EXPORTS).
 *
 * Removal keeps every id, as hpfw_gpu_index_remove does on one handle: the clips named become empty, the others' hashprints
 * close up in place on the shard that holds them, and every shard keeps its range of ids (hpfw_gpu_shard_range) and its clip
 * base.  Every hpfw_gpu_group_search_* afterwards equals its one-handle namesake after the same removal, field for field.
 * The ids are checked against the group's clip count before any shard is touched (HPFW_E_INVALID: an id outside
 * [0, hpfw_gpu_group_index_size), n < 0, a null list with n > 0; every shard is then as it was), routed to the shard whose range
 * holds them, and removed there by hpfw_gpu_index_remove with local ids, every shard on its own stream and host thread.  The
 * group's own offsets, which the voting search's tally reads, follow the same rule.  No collective is needed.  A repeated id
 * and an id of an empty clip are no-ops; the list need not be sorted.  A shard that fails for want of memory (its staging
 * buffer) fails the call; the other shards have then removed their clips, and the group's offsets are unchanged: rebuild.
 *
 * Adding to a sharded index is out of scope: shards are contiguous ranges of ids, so new ids would all fall to the last
 * shard's range.  A catalogue that grows is rebuilt with hpfw_gpu_group_index_build.
 * All pointers are HOST pointers.
 */
#ifndef HPFW_GPU_MULTI_INDEX_H
#define HPFW_GPU_MULTI_INDEX_H

#include "hpfw_gpu_multi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* clips [n]: global ids, in any order */
int hpfw_gpu_group_index_remove(hpfw_gpu_group *g, const int64_t *clips, int64_t n);

#ifdef __cplusplus
}
#endif
#endif
