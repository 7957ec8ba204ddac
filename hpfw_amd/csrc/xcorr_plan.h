// xcorr_plan.h -- the host side of the exact cross-correlation (k_xcorr.hip): what a job must
// satisfy, and its split into the parts the two kernels run.  Plain C++ (no HIP): tests/emu/xcorr_plan_check.cpp builds
// it alone.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/hpfw_gpu.h"

namespace hpfw {

// a job as the kernels take it: a [a0, a0 + a_len) and the segment b [b0, b0 + len) of the buffer; lag index
// t = lag + radius reads a[w + t + n] (w = p - radius, 0 outside the operand); r at d_r[r_off + t]; lags t < n_mfma run
// on the matrix cores, the rest on the plain kernel (all or none of them as the parts are planned today)
struct XcJob {
    int64_t a0, a_len, b0, w, len, r_off;
    int32_t n_lags, n_mfma;
};
// a part of a job: lags [t0, t0 + kXcTile) (matrix cores) or [t0, t0 + kXcValuLags) (plain) over samples
// [m0, m0 + chunk) of the segment
struct XcItem {
    int32_t job, t0;
    int64_t m0;
};
constexpr int kXcTile = 1024;       // lags of one accumulator tile: i + 32 j
// samples per matrix-core part: its int32 accumulators are flushed to int64 after at most this many samples (the one of
// weight 2^8 takes two digit products of up to 2^14 per sample)
constexpr int kXcChunk = 16384;
static_assert(2ll * kXcChunk * 16384 < (1ll << 31), "int32 accumulators overflow before the flush");
constexpr int kXcValuLags = 256, kXcValuChunk = 4096;
constexpr int64_t kXcMaxRange = (int64_t)1 << 46, kXcMaxP = (int64_t)1 << 40;

// nullptr when the job is valid, else what is wrong with it; n_pcm < 0: the buffer's size is not known
inline const char *xcorr_check(const hpfw_xcorr_job &j, int64_t n_pcm)
{
    if (j.len < 1 || j.len > HPFW_XCORR_MAX_LEN) return "xcorr: len outside 1 .. 2^22";
    if (j.radius < 0 || j.radius > HPFW_XCORR_MAX_RADIUS) return "xcorr: radius outside 0 .. 4096";
    if (j.a_off < 0 || j.a_len < 0 || j.b_off < 0 || j.b_len < 0) return "xcorr: negative operand range";
    if (j.a_off > kXcMaxRange || j.a_len > kXcMaxRange || j.b_off > kXcMaxRange || j.b_len > kXcMaxRange)
        return "xcorr: operand range outside any buffer";
    if (n_pcm >= 0 && (j.a_off > n_pcm || j.a_len > n_pcm - j.a_off || j.b_off > n_pcm || j.b_len > n_pcm - j.b_off))
        return "xcorr: operand range outside the buffer";
    if (j.q < 0 || j.q > j.b_len || j.len > j.b_len - j.q) return "xcorr: b[q .. q + len) outside b";
    if (j.p > kXcMaxP || j.p < -kXcMaxP) return "xcorr: |p| above 2^40";
    return nullptr;
}

inline int64_t xcorr_lags(const hpfw_xcorr_job &j) { return 2 * (int64_t)j.radius + 1; }

// the job (valid) as number `index` of a launch with r at r_off, its parts appended to the two lists: every lag on the
// matrix cores, in tiles of 1024 (2 radius + 1 is odd: radius 1024 is three tiles, the last for one lag -- a tile costs less
// than the plain kernel takes for that lag), or every lag on the plain kernel (valu_only)
inline XcJob xcorr_plan_job(const hpfw_xcorr_job &j, int32_t index, int64_t r_off, bool valu_only, std::vector<XcItem> &mfma,
                            std::vector<XcItem> &valu)
{
    const int32_t n_lags = (int32_t)xcorr_lags(j), n_mfma = valu_only ? 0 : n_lags;
    for (int32_t t0 = 0; t0 < n_mfma; t0 += kXcTile)
        for (int64_t m0 = 0; m0 < j.len; m0 += kXcChunk) mfma.push_back(XcItem{index, t0, m0});
    for (int32_t t0 = n_mfma; t0 < n_lags; t0 += kXcValuLags)
        for (int64_t m0 = 0; m0 < j.len; m0 += kXcValuChunk) valu.push_back(XcItem{index, t0, m0});
    return XcJob{j.a_off, j.a_len, j.b_off + j.q, j.p - j.radius, j.len, r_off, n_lags, n_mfma};
}

} // namespace hpfw
