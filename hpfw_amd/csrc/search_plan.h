// search_plan.h -- the host side of the searches' query groups (search.hip, local.hip): which
// scan a call takes, how many queries share a pass so that its (query, clip) table fits the budget, and the lengths that the
// matrix-core scans are told per group of 32 queries.  Plain C++ (no HIP): tests/emu/search_plan_check.cpp builds it alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace hpfw {

// entries of a pass's table: the plain search's 8-byte keys stay below 1 GiB, the overlap search's 16-byte entries below
// 1 GiB, the local search's 8-byte keys below 512 MiB
constexpr int64_t kSearchTableEntries = (int64_t)1 << 27;
constexpr int64_t kOverlapTableEntries = (int64_t)1 << 26;
constexpr int64_t kLocalTableEntries = (int64_t)1 << 26;
// queries along gridDim.y: the plain scans put groups of 8 or 32 there, the popcount kernels of the other two one query
constexpr int64_t kSearchGridQueries = (int64_t)65535 * 8 / 32 * 32; // 524 256
constexpr int64_t kPopcGridQueries = 65504;

// The queries of one pass, a multiple of 32: as many as `budget` entries hold rows of row_entries (n_clips, or n_clips x
// splits) for, at least 32, no more than the call has and than grid_queries.  table_kb >= 0: that many KiB of entry_bytes
// at most, and at least 32 queries' rows, for tests of more than one pass (join_plan.h takes it the same way).
inline int64_t search_group_queries(int64_t n_q, int64_t row_entries, int64_t budget, int64_t grid_queries, int64_t entry_bytes, int64_t table_kb)
{
    // (a table_kb at or above the budget changes nothing, and is not multiplied: no overflow for any value)
    if (table_kb >= 0 && table_kb < budget) budget = std::min(std::max(table_kb * 1024 / entry_bytes, 32 * row_entries), budget);
    int64_t qgroup = std::max<int64_t>(32, budget / row_entries / 32 * 32);
    qgroup = std::min(qgroup, (n_q + 31) / 32 * 32);
    return std::min(qgroup, grid_queries);
}

// The scan runs on the matrix cores (query_scan.h) unless the window of the longest query does not fit the LDS (queries of
// several thousand hashprints) or the call's switch asks for the xor/popcount kernel.
constexpr size_t kScanLdsLimit = 160 * 1024;
inline bool search_on_matrix_cores(bool popc_asked, size_t scan_lds_bytes) { return !popc_asked && scan_lds_bytes <= kScanLdsLimit; }

// gk [2 per group of 32 queries]: the group's longest query and its shortest non-empty one (0: it has none)
inline std::vector<int> search_group_lengths(const int64_t *q_off, int64_t n_q)
{
    std::vector<int> gk((size_t)(n_q + 31) / 32 * 2, 0);
    for (int64_t i = 0; i < n_q; ++i) {
        const int kq = (int)(q_off[i + 1] - q_off[i]);
        int &mx = gk[(size_t)i / 32 * 2], &mn = gk[(size_t)i / 32 * 2 + 1];
        mx = std::max(mx, kq);
        if (kq > 0) mn = mn == 0 ? kq : std::min(mn, kq);
    }
    return gk;
}
// the shortest non-empty query of groups [g_begin, g_end) of gk (0: none)
inline int search_shortest_query(const std::vector<int> &gk, int64_t g_begin, int64_t g_end)
{
    int mn = 0;
    for (int64_t g = g_begin; g < g_end; ++g)
        if (gk[(size_t)g * 2 + 1] > 0) mn = mn == 0 ? gk[(size_t)g * 2 + 1] : std::min(mn, gk[(size_t)g * 2 + 1]);
    return mn;
}

} // namespace hpfw
