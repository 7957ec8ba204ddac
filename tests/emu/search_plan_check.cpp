// search_plan_check.cpp -- the query groups of the searches (hpfw_amd/csrc/search_plan.h) in a program of its own, for ASan and
// UBSan: the group size of the plain, overlap and local searches for a sweep of queries, clips and splits against the
// formulas the three searches had before the plan had a header of its own, written out here; with a table of a few KiB, its
// properties; and the groups' lengths against a walk of the queries.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../hpfw_amd/csrc/search_plan.h"

#define CHECK(c)                                                                                                                          \
    do {                                                                                                                                  \
        if (!(c)) {                                                                                                                       \
            std::printf("search_plan_check: line %d: %s (n_q %ld, n_clips %ld, splits %ld, kb %ld)\n", __LINE__, #c, (long)n_q, (long)n_clips, \
                        (long)splits, (long)kb);                                                                                          \
            return 1;                                                                                                                     \
        }                                                                                                                                 \
    } while (0)

int main()
{
    long cases = 0, many = 0, floor32 = 0;
    const int64_t n_qs[] = {1, 7, 31, 32, 33, 64, 70, 1000, 65504, 65505, 100000, 524256, 524257, 3000000};
    const int64_t n_clipss[] = {1, 2, 5, 31, 33, 1000, 4095, 4096, 4097, 16384, 100000, 2097151, 2097152, 2097153, 4194304, 4194305, 50000000, 300000000};
    const int64_t splitss[] = {1, 2, 3, 64};
    const int64_t kbs[] = {-1, 0, 1, 4, 5, 50, 1000, (int64_t)1 << 21, (int64_t)1 << 40, (int64_t)1 << 62, INT64_MAX};
    for (int64_t n_q : n_qs)
        for (int64_t n_clips : n_clipss)
            for (int64_t splits : splitss)
                for (int64_t kb : kbs) {
                    // the formulas as they stood in search.hip (the plain and the overlap search) and in local.hip
                    int64_t plain = std::max<int64_t>(32, ((int64_t)1 << 27) / n_clips / 32 * 32);
                    plain = std::min<int64_t>(plain, (n_q + 31) / 32 * 32);
                    plain = std::min<int64_t>(plain, (int64_t)65535 * 8 / 32 * 32);
                    int64_t overlap = std::max<int64_t>(32, ((int64_t)1 << 26) / (n_clips * splits) / 32 * 32);
                    overlap = std::min<int64_t>(overlap, (n_q + 31) / 32 * 32);
                    overlap = std::min<int64_t>(overlap, 65504);
                    int64_t local = std::max<int64_t>(32, ((int64_t)1 << 26) / n_clips / 32 * 32);
                    local = std::min<int64_t>(local, (n_q + 31) / 32 * 32);
                    local = std::min<int64_t>(local, 65504);
                    struct {
                        int64_t row, budget, grid, entry, old;
                    } const searches[] = {{n_clips, hpfw::kSearchTableEntries, hpfw::kSearchGridQueries, 8, plain},
                                          {n_clips * splits, hpfw::kOverlapTableEntries, hpfw::kPopcGridQueries, 16, overlap},
                                          {n_clips, hpfw::kLocalTableEntries, hpfw::kPopcGridQueries, 8, local}};
                    for (const auto &sr : searches) {
                        const int64_t q = hpfw::search_group_queries(n_q, sr.row, sr.budget, sr.grid, sr.entry, kb);
                        ++cases;
                        if (kb < 0 || kb >= ((int64_t)1 << 50)) { // unset, or a table no budget reaches (kb * 1024 would not fit 64 bits)
                            CHECK(q == sr.old);
                            continue;
                        }
                        CHECK(q >= 32 && q % 32 == 0 && q <= sr.old);
                        const int64_t asked = kb * 1024 / sr.entry;                  // entries
                        CHECK(q * sr.row <= std::max(asked, 32 * sr.row));          // within the table asked for, or 32 queries' rows
                        if (q * sr.row > asked) ++floor32;
                        if (q < n_q) ++many;
                        // and no smaller than it has to be: another 32 queries would not fit, or the call, the grid or the default ends it
                        CHECK(q == sr.old || (q + 32) * sr.row > asked);
                    }
                }
    int64_t n_q = 0, n_clips = 0, splits = 0, kb = 0;
    CHECK(many > 500 && floor32 > 500);

    // the groups' lengths: 0 to 100 queries of lengths 0..9 from a generator of its own
    unsigned state = 12345;
    for (n_q = 0; n_q <= 100; ++n_q) {
        std::vector<int64_t> q_off((size_t)n_q + 1, 0);
        for (int64_t i = 0; i < n_q; ++i) {
            state = state * 1664525u + 1013904223u;
            q_off[(size_t)i + 1] = q_off[(size_t)i] + ((state >> 16) % 4 == 0 ? 0 : (state >> 20) % 10);
        }
        const std::vector<int> gk = hpfw::search_group_lengths(q_off.data(), n_q);
        CHECK((int64_t)gk.size() == (n_q + 31) / 32 * 2);
        for (int64_t g = 0; g < (n_q + 31) / 32; ++g) {
            int mx = 0, mn = 0;
            for (int64_t i = 32 * g; i < std::min(n_q, 32 * g + 32); ++i) {
                const int k = (int)(q_off[(size_t)i + 1] - q_off[(size_t)i]);
                mx = std::max(mx, k);
                if (k > 0 && (mn == 0 || k < mn)) mn = k;
            }
            CHECK(gk[(size_t)g * 2] == mx && gk[(size_t)g * 2 + 1] == mn);
        }
        for (int64_t a = 0; a <= (n_q + 31) / 32; ++a)
            for (int64_t b = a; b <= (n_q + 31) / 32; ++b) {
                int mn = 0;
                for (int64_t i = 32 * a; i < std::min(n_q, 32 * b); ++i) {
                    const int k = (int)(q_off[(size_t)i + 1] - q_off[(size_t)i]);
                    if (k > 0 && (mn == 0 || k < mn)) mn = k;
                }
                CHECK(hpfw::search_shortest_query(gk, a, b) == mn);
            }
    }
    CHECK(hpfw::search_on_matrix_cores(false, 160 * 1024) && !hpfw::search_on_matrix_cores(false, 160 * 1024 + 1) &&
          !hpfw::search_on_matrix_cores(true, 1000));
    std::printf("search_plan_check ok: %ld group sizes, %ld of more than one group, %ld at the floor of 32 queries\n", cases, many, floor32);
    return 0;
}
