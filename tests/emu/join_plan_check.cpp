// join_plan_check.cpp -- the pass plan of the joins (hpfw_amd/csrc/join_plan.h) in a program of its own, for ASan and UBSan:
// the catalogue and local self-joins of 0 to 70 clips and the join of 0 to 70 clips with 0 to 70 recordings (among_new 0
// and 1), entries of 8 and 16 bytes, the default table and tables of a few KiB that force 2, 3 and many passes, the default
// and forced splits.  The plan's properties, and splits, pass_groups and n_passes against the formulas the joins used
// before the plan had a header of its own, written out here.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "../../hpfw_amd/csrc/join_plan.h"

#define CHECK(c)                                                                                                                \
    do {                                                                                                                        \
        if (!(c)) {                                                                                                             \
            std::printf("join_plan_check: line %d: %s (kind %d, n_index %d, n_x %d, entry %d, kb %d, forced %d, n_max %d)\n", __LINE__, #c, \
                        kind, n_index, n_x, (int)entry, (int)kb, (int)forced, (int)n_max);                                      \
            return 1;                                                                                                           \
        }                                                                                                                       \
    } while (0)

int main()
{
    long cases = 0, seen_passes[5] = {0, 0, 0, 0, 0}; // [min(n_passes, 4)]
    long one_group_over_budget = 0;
    const int64_t kbs[] = {-1, 0, 1, 3, 8, 20, 50, 130};
    const int64_t forceds[] = {0, 1, 3, 64};
    const int64_t lens[][2] = {{100, 1}, {262143, 300}}; // (longest recording, shortest overlap): 1 chunk a pair, and 512
    // kind 0: the self-joins (n_index clips); 1: the join, among_new = 0; 2: the join, among_new = 1
    for (int kind = 0; kind < 3; ++kind)
        for (int n_index = 0; n_index <= 70; ++n_index)
            for (int n_x = 0; n_x <= (kind ? 70 : 0); ++n_x) {
                const int64_t rows = kind == 2 ? n_index + n_x : n_index;
                const int64_t n_groups = (rows + 31) / 32, n_cols = kind ? n_x : n_index;
                // what the plan is given, and what its pair_first must sum
                std::function<int64_t(int64_t)> given, group_pairs;
                if (kind) {
                    given = group_pairs = [&](int64_t g) { return hpfw::join_group_pairs(n_index, n_x, kind == 2, g); };
                } else {
                    given = [&](int64_t g) { return hpfw::selfjoin_group_pairs(n_index, g); };
                    group_pairs = [&](int64_t g) { return std::max<int64_t>(n_index - 32 * g - 1, 0); };
                }
                int64_t pairs = 0;
                for (int64_t g = 0; g < n_groups; ++g) pairs += group_pairs(g);
                for (int64_t entry : {(int64_t)8, (int64_t)16})
                    for (int64_t kb : kbs)
                        for (int64_t forced : forceds)
                            for (const auto &len : lens) {
                                const int64_t n_max = len[0], min_overlap = len[1];
                                const hpfw::JoinPlan pl = hpfw::join_plan(n_groups, given, n_cols, n_max, min_overlap, 1024, entry, forced, kb);
                                ++cases;
                                CHECK(pl.pairs == pairs);
                                if (pairs == 0) { // (the joins returned before they planned anything)
                                    CHECK(pl.n_passes == 0 && pl.pair_first.empty());
                                    continue;
                                }
                                // the formulas of the joins' passes as they stood in selfjoin.hip (* 64) and localjoin.hip (* 128)
                                const int64_t chunks = (2 * n_max - 2 * min_overlap) / 1024 + 1;
                                int64_t splits =
                                    forced ? std::min<int64_t>(std::max<int64_t>(forced, 1), 64) : std::min<int64_t>({chunks, (2048 + pairs - 1) / pairs, 64});
                                int64_t budget = (int64_t)1 << 26;
                                if (kb >= 0) budget = std::min(std::max<int64_t>(kb * (entry == 16 ? 64 : 128), 32 * n_cols), budget);
                                splits = std::min(splits, budget / (32 * n_cols));
                                const int64_t pass_groups = std::min(n_groups, budget / (32 * n_cols * splits));
                                const int64_t n_passes = (n_groups + pass_groups - 1) / pass_groups;
                                CHECK(pl.splits == splits && pl.pass_groups == pass_groups && pl.n_passes == n_passes);
                                // the properties
                                CHECK(pl.pass_groups >= 1 && pl.splits >= 1 && pl.splits <= 64);
                                const int64_t asked = kb >= 0 ? std::min<int64_t>(kb * 1024 / entry, (int64_t)1 << 26) : (int64_t)1 << 26;
                                const int64_t table = 32 * pl.pass_groups * n_cols * pl.splits; // entries
                                if (table > asked) {
                                    CHECK(pl.pass_groups == 1 && pl.splits == 1); // exactly one row group's
                                    ++one_group_over_budget;
                                }
                                // every row group in exactly one pass: pass p takes groups p pass_groups .. and the last pass is not empty
                                CHECK(pl.n_passes * pl.pass_groups >= n_groups && (pl.n_passes - 1) * pl.pass_groups < n_groups);
                                CHECK((int64_t)pl.pair_first.size() == pl.n_passes * (pl.pass_groups + 1));
                                int64_t total = 0;
                                for (int64_t p = 0; p < pl.n_passes; ++p) {
                                    const uint32_t *pf = pl.pass(p);
                                    int64_t sum = 0;
                                    CHECK(pf[0] == 0);
                                    for (int64_t i = 0; i < pl.pass_groups; ++i) {
                                        const int64_t g = p * pl.pass_groups + i;
                                        sum += g < n_groups ? group_pairs(g) : 0;
                                        CHECK(pf[i + 1] == sum);
                                    }
                                    total += sum;
                                }
                                CHECK(total == pairs);
                                ++seen_passes[std::min<int64_t>(pl.n_passes, 4)];
                            }
            }
    int kind = -1, n_index = 0, n_x = 0;
    int64_t entry = 0, kb = 0, forced = 0, n_max = 0;
    CHECK(seen_passes[1] > 1000 && seen_passes[2] > 1000 && seen_passes[3] > 1000 && seen_passes[4] > 1000 && one_group_over_budget > 1000);
    std::printf("join_plan_check ok: %ld plans, %ld/%ld/%ld/%ld of 1/2/3/more passes\n", cases, seen_passes[1], seen_passes[2], seen_passes[3],
                seen_passes[4]);
    return 0;
}
