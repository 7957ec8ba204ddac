// streams_plan_check.cpp -- the planning of a push to live feeds (hpfw_amd/csrc/streams_plan.cpp) under the
// host sanitizers: a stand-alone program, no GPU and no HIP.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I hpfw_amd/csrc \
//       tools/streams_plan_check.cpp hpfw_amd/csrc/streams_plan.cpp -o streams_plan_check && ./streams_plan_check
//
// Random sets of feeds at random rates (44.1 kHz among them), positions up to 2^40 and beyond, counts from 0 to the feed's
// room and one past it, and ring geometries down to capacity = win.  For every accepted push it checks that
//   - m0 = emitted(n_old), m1 = emitted(n_old + count) by an independent statement of the formula, m1 - m0 <= capacity;
//   - the two pieces of a run cover [m0, m1) exactly once, lie inside the feed's ring, output m at ring position m mod capacity,
//     and the run is split only at the ring's end;
//   - the runs of a 44.1 kHz feed do the same for its chunk, and src walks the staged chunks back to back;
//   - every feed that takes part is in exactly one group, the groups are by rate, and `most` is the largest run of each;
//   - history buffers alternate and lie inside the feed's own two buffers;
//   - a refused push names the first feed whose count exceeds its room, and the room is the inverse of emitted:
//     emitted(n + room) - e hop <= capacity < emitted(n + room + 1) - e hop.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>

#include "streams_plan.h"

using namespace hpfw;

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::fprintf(stderr, "line %d: %s (trial %d)\n", __LINE__, #c, trial); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

// emitted(n) stated on its own: the outputs m with floor(m M / L) + H <= n - 1
static int64_t emitted_ref(int64_t n, int64_t L, int64_t M, int64_t H)
{
    if (n <= H) return 0;
    __int128 m = ((__int128)(n - H) * L) / M; // about there; walk to the first m that is not final
    while (m > 0 && (m - 1) * M / L + H > n - 1) --m;
    while (m * M / L + H <= n - 1) ++m;
    return (int64_t)m;
}

int main()
{
    std::mt19937_64 rng(20250);
    const int rates_some[] = {8000, 11025, 22050, 32000, 37800, 44056, 44100, 48000, 88200, 96000, 192000};
    int64_t pushes = 0, refused = 0, split = 0, runs = 0;
    for (int trial = 0; trial < 20000; ++trial) {
        const int n_feeds = 1 + (int)(rng() % 9);
        const int64_t win = 1 + (int64_t)(rng() % 300000), hop = 1 + (int64_t)(rng() % win);
        const int64_t capacity = win + (int64_t)(rng() % 3 == 0 ? 0 : rng() % (2 * win + 7));
        std::vector<RingFeed> feeds((size_t)n_feeds);
        int64_t hist = 0;
        for (RingFeed &f : feeds) {
            const int rate = rng() % 4 ? rates_some[rng() % 11] : 8000 + (int)(rng() % 184001);
            if (rate != 44100) {
                const int g = std::gcd(44100, rate);
                f.rate = rate;
                f.L = 44100 / g;
                f.M = rate / g;
                f.H = (int32_t)((160ll * std::max(f.L, f.M) + 9ll * f.L - 1) / (9ll * f.L));
                f.hist = hist;
                f.hist_len = (2 * (int64_t)f.H - 1 + 7) & ~(int64_t)7;
                hist += 2 * f.hist_len;
                f.cur = (int32_t)(rng() % 2);
            }
            // a state a feed can be in: e windows handed out, the ring holding between 0 and capacity outputs behind e hop
            const int kind = (int)(rng() % 4);
            const int64_t e = kind == 0 ? 0 : kind == 1 ? (int64_t)(rng() % 50) : (((int64_t)1 << 40) + (int64_t)(rng() % 1000000)) / hop;
            const int64_t held = (int64_t)(rng() % (uint64_t)(capacity + 1)); // emitted - e hop
            // the largest n with emitted(n) <= e hop + held (for e = 0 and held = 0 any n <= H)
            f.e = e;
            f.n = 0;
            RingFeed probe = f;
            f.n = ring_room(probe, hop, held); // H + floor((e hop + held) M / L)
            int64_t em = ring_emitted(f.n, f.L, f.M, f.H);
            if (em < e * hop) em = ring_emitted(++f.n, f.L, f.M, f.H); // (L > M: the outputs come several at a time)
            if (em < e * hop || em - e * hop > capacity || (e == 0 && held == 0)) {
                f.e = 0;
                f.n = (int64_t)(rng() % (uint64_t)(f.H + 1)); // a feed that has emitted nothing yet
            }
        }
        std::vector<int64_t> counts((size_t)n_feeds);
        int want_bad = -1;
        for (int i = 0; i < n_feeds; ++i) {
            const RingFeed &f = feeds[(size_t)i];
            const int64_t room = ring_room(f, hop, capacity);
            CHECK(room >= 0);
            // the room is the inverse of emitted
            CHECK(emitted_ref(f.n + room, f.L, f.M, f.H) - f.e * hop <= capacity);
            CHECK(emitted_ref(f.n + room + 1, f.L, f.M, f.H) - f.e * hop > capacity);
            CHECK(emitted_ref(f.n, f.L, f.M, f.H) == ring_emitted(f.n, f.L, f.M, f.H));
            const int k = (int)(rng() % 8);
            counts[(size_t)i] = k == 0 ? 0 : k == 1 ? std::min<int64_t>(1, room) : k == 2 ? room : k == 3 && trial % 5 == 0 ? room + 1
                                                                                                : (int64_t)(rng() % (uint64_t)(room + 1));
            if (counts[(size_t)i] > room && want_bad < 0) want_bad = i;
        }
        RingPushPlan plan;
        const int bad = ring_plan_push(feeds, counts.data(), hop, capacity, &plan);
        CHECK(bad == want_bad);
        if (bad >= 0) {
            ++refused;
            continue;
        }
        ++pushes;
        int64_t src = 0;
        size_t at_copy = 0;
        std::vector<int> seen(plan.rs.size(), 0);
        for (int i = 0; i < n_feeds; ++i) {
            const RingFeed &f = feeds[(size_t)i];
            const int64_t cnt = counts[(size_t)i], base = (int64_t)i * capacity;
            if (cnt == 0) continue;
            if (f.H == 0) {
                int64_t done = 0;
                while (done < cnt) {
                    CHECK(at_copy < plan.copy.size());
                    const RingRun &r = plan.copy[at_copy++];
                    CHECK(r.src == src + done && r.count > 0 && r.count <= plan.copy_longest);
                    CHECK(r.dst == base + (f.n + done) % capacity && r.dst + r.count <= base + capacity);
                    CHECK(done + r.count == cnt || r.dst + r.count == base + capacity); // split only at the ring's end
                    done += r.count;
                }
                CHECK(done == cnt);
            } else {
                size_t j = 0;
                while (j < plan.rs.size() && !(plan.rs[j].base == base)) ++j;
                CHECK(j < plan.rs.size() && !seen[j]);
                seen[j] = 1;
                const RingRsRun &r = plan.rs[j];
                ++runs;
                CHECK(r.src == src && r.n_old == f.n && r.count == cnt);
                CHECK(r.m0 == emitted_ref(f.n, f.L, f.M, f.H) && r.m1 == emitted_ref(f.n + cnt, f.L, f.M, f.H));
                const int64_t n_out = r.m1 - r.m0;
                CHECK(n_out >= 0 && n_out <= capacity && r.m0 >= f.e * hop && r.m1 - f.e * hop <= capacity);
                CHECK(r.pos0 == r.m0 % capacity && r.first >= 0 && r.first <= n_out && r.pos0 + r.first <= capacity);
                CHECK(r.first == n_out || r.pos0 + r.first == capacity); // split only at the ring's end
                CHECK(n_out - r.first <= r.pos0);                        // the piece behind the end stays in front of the first
                split += r.first < n_out;
                for (int t = 0; t < 6 && n_out; ++t) { // where the kernel puts output m0 + jj
                    const int64_t jj = t == 0 ? 0 : t == 1 ? n_out - 1 : t == 2 ? std::min(r.first, n_out - 1) : t == 3 ? std::max<int64_t>(r.first - 1, 0)
                                                                                                                    : (int64_t)(rng() % (uint64_t)n_out);
                    const int64_t pos = jj < r.first ? r.pos0 + jj : jj - r.first;
                    CHECK(pos >= 0 && pos < capacity && pos == (r.m0 + jj) % capacity);
                }
                const int64_t rd = f.hist + (f.cur ? f.hist_len : 0), wr = f.hist + (f.cur ? 0 : f.hist_len);
                CHECK(r.hist_rd == rd && r.hist_wr == wr && 2 * f.H - 1 <= f.hist_len);
                // the oldest input an output of this push reads is in the history or the chunk
                CHECK(n_out == 0 || (int64_t)((__int128)r.m0 * f.M / f.L) - f.H + 1 >= f.n - (2 * f.H - 1));
                CHECK(n_out == 0 || (int64_t)((__int128)(r.m1 - 1) * f.M / f.L) + f.H <= f.n + cnt - 1);
            }
            src += cnt;
        }
        CHECK(at_copy == plan.copy.size() && src == plan.total);
        for (int v : seen) CHECK(v == 1);
        size_t covered = 0;
        for (size_t g = 0; g < plan.groups.size(); ++g) {
            const RingPushPlan::Group &gr = plan.groups[g];
            CHECK((size_t)gr.first == covered && gr.n > 0);
            for (size_t g2 = 0; g2 < g; ++g2) CHECK(plan.groups[g2].rate != gr.rate);
            int64_t most = 0;
            for (int j = gr.first; j < gr.first + gr.n; ++j) {
                CHECK(feeds[(size_t)(plan.rs[(size_t)j].base / capacity)].rate == gr.rate);
                most = std::max(most, plan.rs[(size_t)j].m1 - plan.rs[(size_t)j].m0);
            }
            CHECK(most == gr.most);
            covered += (size_t)gr.n;
        }
        CHECK(covered == plan.rs.size());
    }
    std::printf("streams_plan_check ok: %" PRId64 " pushes planned (%" PRId64 " resampled runs, %" PRId64 " across the ring's end), %" PRId64
                " refused\n",
                pushes, runs, split, refused);
    return pushes > 10000 && refused > 100 && split > 100 ? 0 : 1;
}
