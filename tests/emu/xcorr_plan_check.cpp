// xcorr_plan_check.cpp -- the host side of the exact cross-correlation (hpfw_amd/csrc/xcorr_plan.h) in a program of its
// own, for the sanitizers: what a job must satisfy, and that the parts a job is split into cover every lag of every
// sample exactly once within the accumulators' bound.  Built and run by tests/test_xcorr_host.py.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>

#include "../../hpfw_amd/csrc/xcorr_plan.h"

using namespace hpfw;

static int failures = 0;
#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("line %d: %s\n", __LINE__, #cond);                      \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

static hpfw_xcorr_job job(int64_t a_off, int64_t a_len, int64_t b_off, int64_t b_len, int64_t p, int64_t q, int64_t len, int32_t radius)
{
    return hpfw_xcorr_job{a_off, a_len, b_off, b_len, p, q, len, radius, 0};
}

static void check_split(const hpfw_xcorr_job &j, bool valu_only)
{
    std::vector<XcItem> mfma, valu;
    const XcJob x = xcorr_plan_job(j, 3, 1000, valu_only, mfma, valu);
    EXPECT(x.n_lags == 2 * j.radius + 1 && x.n_mfma >= 0 && x.n_mfma <= x.n_lags && x.r_off == 1000);
    EXPECT(x.w == j.p - j.radius && x.b0 == j.b_off + j.q && x.len == j.len && x.a0 == j.a_off && x.a_len == j.a_len);
    EXPECT(!valu_only || (x.n_mfma == 0 && mfma.empty()));
    EXPECT(x.n_mfma == (valu_only ? 0 : x.n_lags));
    // (first lag of a block, first sample of a chunk) -> times covered
    std::map<std::pair<int64_t, int64_t>, int> seen;
    for (const XcItem &it : mfma) {
        EXPECT(it.job == 3 && it.t0 % kXcTile == 0 && it.t0 < x.n_mfma && it.m0 % kXcChunk == 0 && it.m0 >= 0 && it.m0 < j.len);
        ++seen[{it.t0, it.m0}];
    }
    for (const XcItem &it : valu) {
        EXPECT(it.job == 3 && it.t0 >= x.n_mfma && (it.t0 - x.n_mfma) % kXcValuLags == 0 && it.t0 < x.n_lags);
        EXPECT(it.m0 % kXcValuChunk == 0 && it.m0 >= 0 && it.m0 < j.len);
        ++seen[{it.t0, it.m0}];
    }
    const int64_t tiles = (x.n_mfma + kXcTile - 1) / kXcTile, chunks = (j.len + kXcChunk - 1) / kXcChunk;
    const int64_t blocks = (x.n_lags - x.n_mfma + kXcValuLags - 1) / kXcValuLags, vchunks = (j.len + kXcValuChunk - 1) / kXcValuChunk;
    EXPECT((int64_t)mfma.size() == tiles * chunks && (int64_t)valu.size() == blocks * vchunks);
    EXPECT((int64_t)seen.size() == tiles * chunks + blocks * vchunks); // no part twice
}

int main()
{
    const int64_t n = 1000;
    const hpfw_xcorr_job good = job(0, 600, 400, 600, 10, 5, 200, 8);
    EXPECT(xcorr_check(good, n) == nullptr && xcorr_check(good, -1) == nullptr);
    // the limits themselves are valid
    EXPECT(!xcorr_check(job(0, 0, 0, HPFW_XCORR_MAX_LEN, 0, 0, HPFW_XCORR_MAX_LEN, HPFW_XCORR_MAX_RADIUS), HPFW_XCORR_MAX_LEN));
    EXPECT(!xcorr_check(job(0, 600, 400, 600, -5000, 400, 200, 0), n));
    EXPECT(xcorr_check(job(1000, 0, 1000, 0, 0, 0, 1, 0), n) != nullptr); // an empty b
    EXPECT(!xcorr_check(job(1000, 0, 999, 1, 0, 0, 1, 0), n));
    // every HPFW_E_INVALID case
    const hpfw_xcorr_job bad[] = {
        job(0, 600, 400, 600, 10, 5, 0, 8), job(0, 600, 400, 600, 10, 5, -3, 8), job(0, 600, 400, 600, 10, 5, HPFW_XCORR_MAX_LEN + 1, 8),
        job(0, 600, 400, 600, 10, 5, 200, -1), job(0, 600, 400, 600, 10, 5, 200, HPFW_XCORR_MAX_RADIUS + 1),
        job(0, 600, 400, 600, 10, -1, 200, 8), job(0, 600, 400, 600, 10, 401, 200, 8), job(0, 600, 400, 600, 10, 601, 200, 8),
        job(0, 600, 400, 600, 10, INT64_MAX, 200, 8), job(500, 501, 400, 600, 10, 5, 200, 8), job(0, 600, 400, 601, 10, 5, 200, 8),
        job(-1, 600, 400, 600, 10, 5, 200, 8), job(0, -600, 400, 600, 10, 5, 200, 8), job(0, 600, -400, 600, 10, 5, 200, 8),
        job(0, 600, 400, -600, 10, 5, 200, 8), job(1001, 0, 400, 600, 10, 5, 200, 8), job(0, INT64_MAX, 400, 600, 10, 5, 200, 8),
        job(INT64_MAX, INT64_MAX, 400, 600, 10, 5, 200, 8), job(0, 600, INT64_MAX, INT64_MAX, 10, 5, 200, 8),
        job(0, 600, 400, 600, INT64_MAX, 5, 200, 8), job(0, 600, 400, 600, INT64_MIN, 5, 200, 8),
    };
    for (const hpfw_xcorr_job &b : bad) EXPECT(xcorr_check(b, n) != nullptr);
    // the device entry point is not told the buffer's size: the ranges beyond it pass, the rest does not
    EXPECT(!xcorr_check(job(500, 501, 400, 601, 10, 5, 200, 8), -1));
    EXPECT(xcorr_check(job(0, INT64_MAX, 400, 600, 10, 5, 200, 8), -1) && xcorr_check(job(-1, 600, 400, 600, 10, 5, 200, 8), -1));

    const int64_t lens[] = {1, 31, 32, 33, 1023, 4096, 4097, 16384, 16385, 70001, 1 << 18, HPFW_XCORR_MAX_LEN};
    const int32_t radii[] = {0, 1, 15, 16, 17, 127, 128, 511, 512, 513, 527, 528, 1024, 1500, 4095, 4096};
    for (int64_t len : lens)
        for (int32_t radius : radii)
            for (int v = 0; v < 2; ++v) check_split(job(0, len, 0, len, 0, 0, len, radius), v != 0);
    // radius 1024: three tiles, the last for one lag; the plain kernel: nine blocks of 256 lags
    std::vector<XcItem> m, v;
    EXPECT(xcorr_plan_job(job(0, 9, 0, 9, 0, 0, 9, 1024), 0, 0, false, m, v).n_mfma == 2049 && m.size() == 3 && v.empty());
    m.clear();
    EXPECT(xcorr_plan_job(job(0, 9, 0, 9, 0, 0, 9, 1024), 0, 0, true, m, v).n_mfma == 0 && m.empty() && v.size() == 9);
    if (failures) return 1;
    std::printf("xcorr_plan_check ok\n");
    return 0;
}
