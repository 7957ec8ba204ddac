// plan_cache.h -- the plain arithmetic of the per-length table cache (plans.hip): which plans an
// incoming plan evicts, and how the constant-Q stage finds the forward bins (the CqPlanDev x-fields and the rows-order
// band tables with their two magic divisors).  Plain C++ (no HIP): tests/emu/plan_cache_check.cpp builds it alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "plan.h"

namespace hpfw {

// a row of n2 complex values has to fit the LDS beside what else the kernels of the stages keep there
constexpr size_t kRowLdsLimit = 150 * 1024;
inline bool row_fits_lds(int n2) { return (size_t)n2 * sizeof(HostCf) <= kRowLdsLimit; }

// ---- eviction --------------------------------------------------------------------------------------------------------
struct CachedPlan {
    int64_t length;
    uint64_t last_use;
    size_t bytes;
};
struct Evictions {
    std::vector<int64_t> victims; // lengths, in the order they go
    int wait_before = -1;         // the victim before which the device-wide wait falls (-1: every victim is known idle)
};
// The cache holds `held` bytes in `plans` (in the order of their lengths) and is to take `incoming` more within `budget`.
// The least recently used go first.  Plans known to be idle (last_use <= idle_clock) go one at a time, as many as the new
// one needs: their blocks pass through the pool to the next length's tables (sizes of neighbouring lengths recur), no
// hipMalloc, no hipFree.  A plan that queued work may still read costs a device-wide wait first, once a call (after it every
// plan is idle): then room for a quarter of the budget is made at once, so that a corpus of distinct lengths larger than the
// cache does not pay that wait with every file.
inline Evictions choose_evictions(std::vector<CachedPlan> plans, size_t held, size_t incoming, size_t budget, uint64_t idle_clock)
{
    Evictions ev;
    std::stable_sort(plans.begin(), plans.end(), [](const CachedPlan &a, const CachedPlan &b) { return a.last_use < b.last_use; });
    size_t goal = budget;
    for (const CachedPlan &p : plans) {
        if (held + incoming <= goal) break;
        if (ev.wait_before < 0 && p.last_use > idle_clock) {
            ev.wait_before = (int)ev.victims.size();
            goal = budget - budget / 4;
        }
        held -= p.bytes;
        ev.victims.push_back(p.length);
    }
    return ev;
}

// ---- where the constant-Q stage finds the forward bins ---------------------------------------------------------------
// kernels.h XsView (the CqPlanDev x-fields): natural order from kmin on after the chirp-z forward transform, else
// x[k mod n1][k / n1 - q2lo] in rows of q2w, with magic = ceil(2^40 / n1): k / n1 = (k magic) >> 40 for every k < kmax
struct CqXLayout {
    int xn1, xw, xq0;
    int64_t xclip; // elements per clip
    unsigned long long xmagic;
};
inline CqXLayout cq_x_layout(const HostPlan &p)
{
    if (p.bluestein) return {1, 0, p.kmin, (int64_t)(p.kmax - p.kmin), 0};
    return {p.n1, p.q2w, p.q2lo, (int64_t)p.n1 * p.q2w, ((1ull << 40) + (unsigned long long)p.n1 - 1) / (unsigned long long)p.n1};
}

// kernels.h XsBandRows (7-smooth lengths): band j covers the q2 = q2a[j] .. q2a[j] + nq2[j] - 1 of every row, its
// n1 * nq2[j] window entries lie at g2_off[j], and magic[j] = ceil(2^32 / nq2[j]) (0 when nq2[j] = 1: not used) gives
// t / nq2[j] = (t magic[j]) >> 32 for every t < n1 * nq2[j] < 2^19
struct CqRowsLayout {
    std::vector<int> q2a, nq2;
    std::vector<unsigned> magic;
    std::vector<int64_t> g2_off;
    int64_t total = 0;   // entries of g2
    int max_entries = 0; // the largest n1 * nq2[j]
};
inline CqRowsLayout cq_rows_layout(const HostPlan &p)
{
    CqRowsLayout r;
    r.q2a.resize(121);
    r.nq2.resize(121);
    r.magic.resize(121);
    r.g2_off.resize(121);
    for (int j = 0; j < 121; ++j) {
        r.q2a[j] = p.start[j] / p.n1;
        r.nq2[j] = (p.start[j] + p.lg[j] - 1) / p.n1 - r.q2a[j] + 1;
        r.magic[j] = r.nq2[j] >= 2 ? (unsigned)(((1ull << 32) + (unsigned)r.nq2[j] - 1) / (unsigned)r.nq2[j]) : 0u;
        r.g2_off[j] = r.total;
        r.total += (int64_t)p.n1 * r.nq2[j];
        r.max_entries = std::max(r.max_entries, p.n1 * r.nq2[j]);
    }
    return r;
}

} // namespace hpfw
