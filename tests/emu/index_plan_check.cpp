// index_plan_check.cpp -- the plan of a removal from the index (hpfw_amd/csrc/index_plan.h) in a program of its own, for
// ASan and UBSan: every subset of the clips of every ragged index of at most 6 clips of 0 to 3 hashprints, at chunk sizes
// 1, 2, 3 and 7, executed pessimistically (a staged chunk read whole and then written, a direct chunk element by element
// from its last to its first after checking that it may) and compared with a plain loop.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../hpfw_amd/csrc/index_plan.h"

#define CHECK(c)                                                                     \
    do {                                                                             \
        if (!(c)) {                                                                  \
            std::printf("index_plan_check: line %d: %s\n", __LINE__, #c);            \
            return 1;                                                                \
        }                                                                            \
    } while (0)

int main()
{
    long cases = 0;
    const int64_t chunks[4] = {1, 2, 3, 7};
    for (int n_clips = 0; n_clips <= 6; ++n_clips) {
        int shapes = 1;
        for (int c = 0; c < n_clips; ++c) shapes *= 4;
        for (int shape = 0; shape < shapes; ++shape) {
            std::vector<int64_t> off(1, 0);
            for (int c = 0, v = shape; c < n_clips; ++c, v /= 4) off.push_back(off.back() + v % 4);
            const int64_t total = off.back();
            for (int subset = 0; subset < (1 << n_clips); ++subset) {
                std::vector<int64_t> removed;
                for (int c = 0; c < n_clips; ++c)
                    if (subset >> c & 1) removed.push_back(c);
                // the plain loop
                std::vector<int64_t> want, want_off(1, 0);
                for (int c = 0; c < n_clips; ++c) {
                    if (!(subset >> c & 1))
                        for (int64_t i = off[c]; i < off[c + 1]; ++i) want.push_back(i);
                    want_off.push_back((int64_t)want.size());
                }
                const int64_t first_removed = removed.empty() ? total : off[removed[0]];
                for (int64_t chunk : chunks) {
                    std::vector<int64_t> new_off(off.size(), -1), buf(total);
                    for (int64_t i = 0; i < total; ++i) buf[i] = i;
                    std::vector<hpfw_index_move> mv;
                    CHECK(hpfw::index_remove_plan(off.data(), n_clips, removed.data(), (int64_t)removed.size(), chunk, new_off.data(), &mv));
                    CHECK(new_off == want_off);
                    int64_t next_dst = mv.empty() ? 0 : mv[0].dst, shift = 0;
                    for (size_t i = 0; i < mv.size();) {
                        size_t j = i;
                        while (j < mv.size() && mv[j].chunk == mv[i].chunk) ++j;
                        CHECK(i == 0 || mv[i].chunk == mv[i - 1].chunk + 1);
                        const int64_t lo = mv[i].dst, hi = mv[j - 1].dst + mv[j - 1].len;
                        CHECK(hi - lo <= chunk && (j == mv.size() || hi - lo == chunk));
                        std::vector<int64_t> stage;
                        for (size_t m = i; m < j; ++m) {
                            CHECK(mv[m].len > 0 && mv[m].dst == next_dst && mv[m].dst >= first_removed && mv[m].src > mv[m].dst);
                            CHECK(mv[m].src - mv[m].dst >= shift && mv[m].src + mv[m].len <= total);
                            CHECK(mv[m].staged == mv[i].staged);
                            shift = mv[m].src - mv[m].dst;
                            next_dst += mv[m].len;
                            if (mv[i].staged)
                                for (int64_t k = 0; k < mv[m].len; ++k) stage.push_back(buf[mv[m].src + k]);
                            else
                                CHECK(mv[m].src >= hi);
                        }
                        if (mv[i].staged) {
                            CHECK(mv[i].src < hi);
                            for (int64_t k = 0; k < hi - lo; ++k) buf[lo + k] = stage[k];
                        } else {
                            for (size_t m = j; m-- > i;)
                                for (int64_t k = mv[m].len; k-- > 0;) buf[mv[m].dst + k] = buf[mv[m].src + k];
                        }
                        i = j;
                    }
                    CHECK(mv.empty() || next_dst == (int64_t)want.size());
                    for (size_t i = 0; i < want.size(); ++i) CHECK(buf[i] == want[i]);
                    ++cases;
                }
            }
        }
    }
    // what the plan refuses
    const int64_t off[3] = {0, 2, 5}, bad_off[3] = {0, 3, 2}, twice[2] = {1, 1}, outside[1] = {2}, negative[1] = {-1}, one[1] = {0};
    int64_t new_off[4];
    std::vector<hpfw_index_move> mv;
    CHECK(!hpfw::index_remove_plan(nullptr, 2, one, 1, 4, new_off, &mv));
    CHECK(!hpfw::index_remove_plan(bad_off, 2, one, 1, 4, new_off, &mv));
    CHECK(!hpfw::index_remove_plan(off, 2, twice, 2, 4, new_off, &mv));
    CHECK(!hpfw::index_remove_plan(off, 2, outside, 1, 4, new_off, &mv));
    CHECK(!hpfw::index_remove_plan(off, 2, negative, 1, 4, new_off, &mv));
    CHECK(!hpfw::index_remove_plan(off, 2, nullptr, 1, 4, new_off, &mv));
    CHECK(!hpfw::index_remove_plan(off, 2, one, 1, 0, new_off, &mv));
    CHECK(!hpfw::index_remove_plan(off, -1, one, 0, 4, new_off, &mv));
    CHECK(hpfw::index_remove_plan(off, 2, one, 1, 4, nullptr, nullptr));
    CHECK(hpfw::index_remove_plan(off, 2, one, 1, 4, new_off, &mv) && mv.size() == 1 && mv[0].dst == 0 && mv[0].src == 2 && mv[0].len == 3 &&
          mv[0].staged == 1 && new_off[1] == 0 && new_off[2] == 3);
    // positions beyond 2^32 hashprints
    const int64_t big = (int64_t)1 << 40, big_off[4] = {0, 1, big, 2 * big};
    CHECK(hpfw::index_remove_plan(big_off, 3, one, 1, big, new_off, &mv) && mv.size() == 2 && mv[1].dst == big && mv[1].src == big + 1 &&
          mv[1].len == big - 1 && mv[1].chunk == 1 && mv[1].staged == 1);
    std::printf("index_plan_check ok (%ld cases)\n", cases);
    return 0;
}
