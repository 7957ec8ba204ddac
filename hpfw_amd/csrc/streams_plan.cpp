// streams_plan.cpp -- the planning of one push to a set of live feeds (streams_plan.h)
#include "streams_plan.h"

#include <algorithm>

namespace hpfw {

int64_t ring_emitted(int64_t n, int32_t L, int32_t M, int32_t H)
{
    if (n <= H) return 0;
    return (int64_t)(((__int128)(n - H) * L + M - 1) / M);
}

int64_t ring_room(const RingFeed &f, int64_t hop, int64_t capacity)
{
    const __int128 x = (__int128)f.e * hop + capacity; // the ring may hold outputs up to here
    return f.H + (int64_t)(x * f.M / f.L) - f.n;
}

int ring_plan_push(const std::vector<RingFeed> &feeds, const int64_t *counts, int64_t hop, int64_t capacity, RingPushPlan *plan)
{
    for (size_t i = 0; i < feeds.size(); ++i)
        if (counts[i] > ring_room(feeds[i], hop, capacity)) return (int)i;
    *plan = RingPushPlan();
    std::vector<std::vector<RingRsRun>> by_rate; // (a set has few distinct rates)
    int64_t src = 0;
    for (size_t i = 0; i < feeds.size(); ++i) {
        const RingFeed &f = feeds[i];
        const int64_t cnt = counts[i], base = (int64_t)i * capacity;
        if (cnt == 0) continue;
        if (f.H == 0) { // 44.1 kHz: the chunk as it is
            const int64_t at = f.n % capacity, first = std::min(cnt, capacity - at);
            plan->copy.push_back({src, base + at, first});
            if (cnt > first) plan->copy.push_back({src + first, base, cnt - first});
            plan->copy_longest = std::max(plan->copy_longest, std::max(first, cnt - first));
        } else {
            RingRsRun r;
            r.src = src;
            r.n_old = f.n;
            r.count = cnt;
            r.m0 = ring_emitted(f.n, f.L, f.M, f.H);
            r.m1 = ring_emitted(f.n + cnt, f.L, f.M, f.H);
            r.base = base;
            r.pos0 = r.m0 % capacity;
            r.first = std::min(r.m1 - r.m0, capacity - r.pos0);
            r.hist_rd = f.hist + (f.cur ? f.hist_len : 0);
            r.hist_wr = f.hist + (f.cur ? 0 : f.hist_len);
            size_t g = 0;
            while (g < plan->groups.size() && plan->groups[g].rate != f.rate) ++g;
            if (g == plan->groups.size()) {
                plan->groups.push_back({f.rate, 0, 0, 0});
                by_rate.emplace_back();
            }
            plan->groups[g].most = std::max(plan->groups[g].most, r.m1 - r.m0);
            by_rate[g].push_back(r);
        }
        src += cnt;
    }
    for (size_t g = 0; g < by_rate.size(); ++g) {
        plan->groups[g].first = (int32_t)plan->rs.size();
        plan->groups[g].n = (int32_t)by_rate[g].size();
        plan->rs.insert(plan->rs.end(), by_rate[g].begin(), by_rate[g].end());
    }
    plan->total = src;
    return -1;
}

} // namespace hpfw
