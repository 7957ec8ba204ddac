// join_plan.h -- the host side of the joins' passes (selfjoin.hip, localjoin.hip; DESIGN.md sections 22, 23 and 26): how many
// workgroups share a pair's chunks, how many row groups a pass takes so that its table fits the budget, and the numbering of
// every pass's pairs.  Plain C++ (no HIP): tests/emu/join_plan_check.cpp builds it alone.
//
// The rows of a join come in groups of 32; group g has group_pairs(g) pairs (row group, b), one per clip b it is scanned
// against.  A pass takes pass_groups consecutive groups and a table of [32 pass_groups][n_cols][splits] entries; every pass
// numbers its pairs from 0, and pair_first [pass_groups + 1] of a pass is the running sum over its groups (groups past the
// last count nothing).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace hpfw {

// Overlap search and joins (overlap_rule.h): a pair's lags come in chunks of 1024; with few pairs the chunks of a pair go
// to `splits` workgroups, each with a table entry of its own -- enough for some 2048 workgroups, at most 64 a pair.
// forced > 0: that many instead (at most 64), for tests of either shape.  pairs > 0
inline int64_t overlap_splits(int64_t chunks, int64_t pairs, int64_t forced)
{
    if (forced > 0) return std::min<int64_t>(forced, 64);
    return std::min<int64_t>({chunks, (2048 + pairs - 1) / pairs, 64});
}

// the pairs of row group g in the join of n_index clips with n_x recordings that are not among them: pair i of group g is
// b = max(n_index, 32 g + 1) + i, and rows at or above n_index are scanned only among_new
inline int64_t join_group_pairs(int64_t n_index, int64_t n_x, int among_new, int64_t g)
{
    if (32 * g >= (among_new ? n_index + n_x : n_index)) return 0; // (no row of the group is launched)
    return std::max<int64_t>(n_index + n_x - std::max(n_index, 32 * g + 1), 0);
}
// and in a self-join of n_clips: b above the group's first row
inline int64_t selfjoin_group_pairs(int64_t n_clips, int64_t g) { return std::max<int64_t>(n_clips - 32 * g - 1, 0); }

// pair_first [n + 1]: the running sum of group_pairs over the n row groups from group0 on, from 0.  false: a sum above 2^32 - 1
template <class GroupPairs>
bool join_pair_first(int64_t group0, int64_t n, GroupPairs group_pairs, uint32_t *pair_first)
{
    pair_first[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t next = (int64_t)pair_first[i] + group_pairs(group0 + i);
        if (next > (int64_t)UINT32_MAX) return false;
        pair_first[i + 1] = (uint32_t)next;
    }
    return true;
}

struct JoinPlan {
    int64_t pairs = 0;                // of all row groups; 0: nothing to scan, and nothing else here is set
    int64_t splits = 0;               // workgroups per pair, 1..64
    int64_t pass_groups = 0;          // row groups per pass, >= 1
    int64_t n_passes = 0;
    std::vector<uint32_t> pair_first; // [n_passes][pass_groups + 1]
    const uint32_t *pass(int64_t p) const { return pair_first.data() + p * (pass_groups + 1); }
};

// n_groups row groups with group_pairs(g) pairs each; a table of n_cols >= 1 columns and entries of entry_bytes; n_max: the
// longest recording, min_overlap: the shortest overlap of a lag that is scanned (the lags of a pair: 2 n_max - 2 min_overlap
// at most, in chunks of `chunk` lags: kernels.h, kSelfjoinChunk).  The table holds 2^26 entries at most; table_kb >= 0:
// that many KiB at most, and at least one row group's, for tests of more than one pass.  forced_splits: as overlap_splits
// takes it.
template <class GroupPairs>
JoinPlan join_plan(int64_t n_groups, GroupPairs group_pairs, int64_t n_cols, int64_t n_max, int64_t min_overlap, int64_t chunk, int64_t entry_bytes,
                   int64_t forced_splits, int64_t table_kb)
{
    JoinPlan pl;
    for (int64_t g = 0; g < n_groups; ++g) pl.pairs += group_pairs(g);
    if (pl.pairs == 0) return pl;
    const int64_t chunks = (2 * n_max - 2 * min_overlap) / chunk + 1;
    int64_t budget = (int64_t)1 << 26;
    if (table_kb >= 0) budget = std::min(std::max<int64_t>(table_kb * 1024 / entry_bytes, 32 * n_cols), budget);
    pl.splits = std::min(overlap_splits(chunks, pl.pairs, forced_splits), budget / (32 * n_cols));
    pl.pass_groups = std::min(n_groups, budget / (32 * n_cols * pl.splits));
    pl.n_passes = (n_groups + pl.pass_groups - 1) / pl.pass_groups;
    pl.pair_first.assign((size_t)(pl.n_passes * (pl.pass_groups + 1)), 0);
    // (a pass has at most pass_groups n_cols pairs, a 32nd of its table's entries: the sums cannot overflow)
    for (int64_t p = 0; p < pl.n_passes; ++p)
        join_pair_first(
            p * pl.pass_groups, pl.pass_groups, [&](int64_t g) { return g < n_groups ? group_pairs(g) : 0; },
            pl.pair_first.data() + p * (pl.pass_groups + 1));
    return pl;
}

} // namespace hpfw
