// plan_cache_check.cpp -- the plain arithmetic of the table cache (hpfw_amd/csrc/plan_cache.h) in a program of its own, for
// ASan and UBSan.  Eviction: a few thousand random caches against the loop as it stood in get_plan, written out here, and
// the properties of the choice.  Layout: the two magic divisors, the band tables of the rows order and the 2^19 that
// kernels.h states, for the first clip length of every n1 the planner chooses (every 7-smooth length from the first that
// yields a hashprint to 8192 x 6826 is planned), the lengths given as arguments, four named ones and the longest accepted.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../hpfw_amd/csrc/plan_cache.h"

#define CHECK(c)                                                                                            \
    do {                                                                                                    \
        if (!(c)) {                                                                                         \
            std::printf("plan_cache_check: line %d: %s (case %ld, %s)\n", __LINE__, #c, (long)id, note.c_str()); \
            return 1;                                                                                       \
        }                                                                                                   \
    } while (0)

namespace {
unsigned g_state = 2024;
unsigned rnd(unsigned n) // 0 .. n - 1
{
    g_state = g_state * 1664525u + 1013904223u;
    return (g_state >> 8) % n;
}

// get_plan's eviction as it stood before the choice had a header: the cache as a map by length, the wait as a count
struct OldRun {
    std::vector<int64_t> victims;
    int waits = 0, wait_before = -1;
    size_t goal = 0, held = 0;
    bool emptied = false;
};
OldRun old_evict(const std::vector<hpfw::CachedPlan> &cache, size_t plan_bytes, size_t incoming, size_t budget, uint64_t idle_clock,
                 uint64_t plan_clock)
{
    std::map<int64_t, hpfw::CachedPlan> plans;
    for (const hpfw::CachedPlan &p : cache) plans[p.length] = p;
    OldRun r;
    r.goal = budget;
    if (plan_bytes + incoming > budget && !plans.empty()) {
        size_t goal = budget;
        while (plan_bytes + incoming > goal && !plans.empty()) {
            auto lru = plans.begin();
            for (auto q = plans.begin(); q != plans.end(); ++q)
                if (q->second.last_use < lru->second.last_use) lru = q;
            if (lru->second.last_use > idle_clock) {
                ++r.waits; // hipDeviceSynchronize
                r.wait_before = (int)r.victims.size();
                idle_clock = plan_clock;
                goal = budget - budget / 4;
            }
            plan_bytes -= lru->second.bytes;
            r.victims.push_back(lru->first);
            plans.erase(lru);
        }
        r.goal = goal;
    }
    r.held = plan_bytes;
    r.emptied = plans.empty();
    return r;
}

int check_evictions(long &n_cases, long &n_evicting, long &n_waits, long &n_emptied)
{
    std::string note;
    for (long id = 0; id < 6000; ++id) {
        const int n_plans = id % 50 == 0 ? 0 : (int)rnd(13);
        std::vector<hpfw::CachedPlan> cache;
        std::set<int64_t> lengths;
        while ((int)lengths.size() < n_plans) lengths.insert(54243 + (int64_t)rnd(100000));
        // last_use: the cache's clock at each plan's last use, all different (get_plan) -- or, every fifth case, with ties
        std::vector<uint64_t> uses;
        for (int i = 0; i < n_plans; ++i) uses.push_back(id % 5 == 4 ? 1 + rnd(4) : (uint64_t)(i + 1) * 3);
        for (int i = n_plans - 1; i > 0; --i) std::swap(uses[(size_t)i], uses[rnd((unsigned)i + 1)]);
        size_t held = 0;
        uint64_t plan_clock = 0;
        for (int64_t n : lengths) { // (in the order of the lengths, as the cache's map has them)
            const size_t bytes = rnd(7) == 0 ? 0 : 1 + rnd(1000);
            cache.push_back({n, uses[cache.size()], bytes});
            held += bytes;
            plan_clock = std::max(plan_clock, cache.back().last_use);
        }
        ++plan_clock; // the incoming plan's own use
        size_t budget, incoming = rnd(1200);
        switch (id % 6) {
        case 0: budget = 0; break;
        case 1: budget = incoming > 0 ? rnd((unsigned)incoming) : 0; break;    // the incoming plan alone is larger
        case 2: budget = held + incoming; break;                                // fits exactly
        case 3: budget = held + incoming > 0 ? held + incoming - 1 : 0; break;  // one byte short
        default: budget = rnd((unsigned)(held + incoming + 100)); break;
        }
        const uint64_t idle_clock = id % 4 == 0 ? 0 : id % 4 == 1 ? plan_clock : rnd((unsigned)plan_clock + 1); // none, all, some idle
        note = "plans " + std::to_string(n_plans) + ", held " + std::to_string(held) + ", incoming " + std::to_string(incoming) +
               ", budget " + std::to_string(budget) + ", idle_clock " + std::to_string(idle_clock);

        const OldRun old = old_evict(cache, held, incoming, budget, idle_clock, plan_clock);
        const hpfw::Evictions ev = hpfw::choose_evictions(cache, held, incoming, budget, idle_clock);
        ++n_cases;
        CHECK(ev.victims == old.victims);       // the same victims in the same order
        CHECK(ev.wait_before == old.wait_before); // a wait before the same victim
        CHECK(old.waits <= 1 && (old.waits == 1) == (ev.wait_before >= 0));
        CHECK(ev.wait_before < (int)ev.victims.size());
        if (ev.wait_before >= 0) CHECK(old.goal == budget - budget / 4);
        // the choice by its properties alone: the victims are the least recently used; the wait falls before the first
        // victim that is not known idle; the walk ends as soon as the goal is met, else with the cache empty
        std::vector<hpfw::CachedPlan> by_use = cache;
        std::stable_sort(by_use.begin(), by_use.end(), [](const hpfw::CachedPlan &a, const hpfw::CachedPlan &b) { return a.last_use < b.last_use; });
        size_t left = held;
        int first_busy = -1;
        for (size_t i = 0; i < ev.victims.size(); ++i) {
            CHECK(ev.victims[i] == by_use[i].length);
            if (first_busy < 0 && by_use[i].last_use > idle_clock) first_busy = (int)i;
            const size_t goal = first_busy >= 0 ? budget - budget / 4 : budget;
            CHECK(left + incoming > goal); // this victim had to go
            left -= by_use[i].bytes;
        }
        CHECK(first_busy == ev.wait_before && left == old.held);
        const size_t goal = ev.wait_before >= 0 ? budget - budget / 4 : budget;
        CHECK(left + incoming <= goal || ev.victims.size() == cache.size());
        if (incoming > goal) CHECK(ev.victims.size() == cache.size() && old.emptied);
        if (!ev.victims.empty()) ++n_evicting;
        if (ev.wait_before >= 0) ++n_waits;
        if (!cache.empty() && ev.victims.size() == cache.size()) ++n_emptied;
    }
    long id = -1;
    CHECK(n_evicting > 1000 && n_waits > 500 && n_emptied > 500 && n_evicting - n_waits > 300);
    return 0;
}

// every 7-smooth n in [lo, hi]
std::vector<int64_t> smooth_lengths(int64_t lo, int64_t hi)
{
    std::vector<int64_t> out;
    for (int64_t p7 = 1; p7 <= hi; p7 *= 7)
        for (int64_t p5 = p7; p5 <= hi; p5 *= 5)
            for (int64_t p3 = p5; p3 <= hi; p3 *= 3)
                for (int64_t p2 = p3; p2 <= hi; p2 *= 2)
                    if (p2 >= lo) out.push_back(p2);
    std::sort(out.begin(), out.end());
    return out;
}

// the sizes of a 7-smooth length's plan with q2lo and q2w as the full plan sets them (plan.cpp: not among the sizes alone)
bool sizes(int64_t n, hpfw::HostPlan &p)
{
    std::string why;
    if (!hpfw::build_plan(n, p, why, true)) return false;
    p.q2lo = p.kmin / p.n1;
    p.q2w = (p.kmax - 1) / p.n1 - p.q2lo + 1;
    return true;
}

struct LayoutCounts {
    long lengths = 0, every_k = 0, ks = 0, bands = 0, ts = 0, largest_band = 0;
    std::set<int> n1s;
};

// every_k: every k < kmax; else every k within 2 of a multiple of n1 (the quotient is monotonic in k: right at both ends of a
// run of n1 is right throughout) and every 997th
int check_layout(const hpfw::HostPlan &p, bool every_k, LayoutCounts &cnt)
{
    const long id = (long)p.n;
    std::string note = "n1 " + std::to_string(p.n1);
    CHECK(!p.bluestein && p.n1 >= 1 && p.n1 <= 8192 && p.kmax < (1 << 27));
    const hpfw::CqXLayout x = hpfw::cq_x_layout(p);
    CHECK(x.xn1 == p.n1 && x.xw == p.q2w && x.xq0 == p.q2lo && x.xclip == (int64_t)p.n1 * p.q2w);
    CHECK((unsigned long long)(p.kmax - 1) <= ~0ull / x.xmagic); // the product fits 64 bits
    const auto quotient_ok = [&](int64_t k) { return (int64_t)(((unsigned long long)(unsigned)k * x.xmagic) >> 40) == k / p.n1; };
    if (every_k) {
        for (int64_t k = 0; k < p.kmax; ++k) CHECK(quotient_ok(k));
        cnt.ks += p.kmax;
        ++cnt.every_k;
    } else {
        for (int64_t m = 0; m <= p.kmax; m += p.n1)
            for (int64_t k = std::max<int64_t>(m - 2, 0); k <= m + 2 && k < p.kmax; ++k, ++cnt.ks) CHECK(quotient_ok(k));
        for (int64_t k = 0; k < p.kmax; k += 997, ++cnt.ks) CHECK(quotient_ok(k));
    }
    // every bin the stage reads lies in the rows the forward transform stores
    CHECK(p.q2lo * p.n1 <= p.kmin && (int64_t)(p.q2lo + p.q2w) * p.n1 >= p.kmax);

    const hpfw::CqRowsLayout r = hpfw::cq_rows_layout(p);
    CHECK(r.q2a.size() == 121 && r.nq2.size() == 121 && r.magic.size() == 121 && r.g2_off.size() == 121);
    int64_t sum = 0;
    int largest = 0;
    for (int j = 0; j < 121; ++j) {
        note = "n1 " + std::to_string(p.n1) + ", band " + std::to_string(j);
        const int q2a = r.q2a[(size_t)j], nq2 = r.nq2[(size_t)j];
        const unsigned magic = r.magic[(size_t)j];
        // rows q2a .. q2a + nq2 - 1 are those that hold the band's bins, and the forward transform stores them
        CHECK(nq2 >= 1 && q2a == p.start[j] / p.n1 && q2a + nq2 - 1 == (p.start[j] + p.lg[j] - 1) / p.n1);
        CHECK(q2a >= p.q2lo && q2a + nq2 <= p.q2lo + p.q2w);
        const int64_t entries = (int64_t)p.n1 * nq2;
        CHECK(entries < (1 << 19)); // kernels.h XsBandRows
        CHECK(r.g2_off[(size_t)j] == sum);
        sum += entries;
        largest = std::max(largest, (int)entries);
        if (nq2 == 1) {
            CHECK(magic == 0);
        } else {
            for (int64_t t = 0; t < entries; ++t) CHECK((int64_t)(((unsigned long long)(unsigned)t * magic) >> 32) == t / nq2);
            cnt.ts += entries;
        }
        ++cnt.bands;
    }
    CHECK(r.total == sum && r.max_entries == largest);
    cnt.largest_band = std::max<long>(cnt.largest_band, largest);
    ++cnt.lengths;
    cnt.n1s.insert(p.n1);
    return 0;
}
} // namespace

int main(int argc, char **argv)
{
    long id = 0;
    std::string note;
    long n_cases = 0, n_evicting = 0, n_waits = 0, n_emptied = 0;
    if (check_evictions(n_cases, n_evicting, n_waits, n_emptied)) return 1;
    std::printf("plan_cache_check evictions ok: %ld caches, %ld evict, %ld of them behind a device-wide wait, %ld empty the cache\n", n_cases,
                n_evicting, n_waits, n_emptied);

    // the chirp-z forward transform keeps the bins in natural order: no divisor
    {
        hpfw::HostPlan p;
        std::string why;
        note = "132301";
        CHECK(hpfw::build_plan(132301, p, why, true) && p.bluestein);
        const hpfw::CqXLayout x = hpfw::cq_x_layout(p);
        CHECK(x.xn1 == 1 && x.xw == 0 && x.xq0 == p.kmin && x.xclip == p.kmax - p.kmin && x.xmagic == 0);
    }
    // q2lo and q2w of sizes() are the full plan's
    for (int64_t n : {88200, 132300, 1323000}) {
        hpfw::HostPlan full, p;
        std::string why;
        id = (long)n;
        note = "full plan";
        CHECK(hpfw::build_plan(n, full, why, false, false, 0, false) && sizes(n, p));
        CHECK(full.n1 == p.n1 && full.q2lo == p.q2lo && full.q2w == p.q2w && full.kmin == p.kmin && full.kmax == p.kmax);
    }

    // the first length of every n1, and the longest length accepted
    const int64_t first_length = 54243, n1_max = 8192, n2_max = 6826;
    std::map<int, int64_t> first_of_n1;
    int64_t longest = 0;
    long planned = 0;
    for (int64_t n : smooth_lengths(first_length, n1_max * n2_max)) {
        hpfw::HostPlan p;
        if (!sizes(n, p)) continue;
        ++planned;
        longest = n;
        first_of_n1.emplace(p.n1, n);
    }
    std::set<int64_t> lengths = {88200, 132300, 1323000, longest};
    for (const auto &kv : first_of_n1) lengths.insert(kv.second);
    for (int i = 1; i < argc; ++i) lengths.insert(std::atoll(argv[i]));
    id = (long)longest;
    note = "the longest length accepted";
    {
        // tests/test_cq_host.py::test_length_limit: 54 190 080 is accepted, 55 125 000 = 8750 x 6300 refused for its n1
        hpfw::HostPlan p;
        CHECK(longest >= 54190080 && sizes(54190080, p) && !sizes(55125000, p));
    }

    LayoutCounts cnt;
    for (int64_t n : lengths) {
        hpfw::HostPlan p;
        id = (long)n;
        note = "not planned";
        CHECK(sizes(n, p));
        if (check_layout(p, p.kmax <= (1 << 21) || n == longest, cnt)) return 1;
    }
    id = 0;
    note = "coverage";
    CHECK(cnt.n1s.size() == first_of_n1.size());
    std::printf("plan_cache_check layout ok: %ld lengths (of %ld planned; the longest %ld) with %zu values of n1 up to %d; k / n1 for %ld k: every "
                "k < kmax at %ld lengths, the longest among them, at the others every k within 2 of a multiple of n1 and every 997th; "
                "t / nq2 for every t of %ld bands, %ld t, the largest band %ld < 2^19\n",
                cnt.lengths, planned, (long)longest, cnt.n1s.size(), *cnt.n1s.rbegin(), cnt.ks, cnt.every_k, cnt.bands, cnt.ts, cnt.largest_band);
    return 0;
}
