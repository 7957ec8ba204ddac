// drift_plan.h -- the host side of clock drift and rendering (k_warp.hip): what a warp track must
// satisfy and which outputs can reach its source, the anchors of a pair, the robust line through their lags, and an affine
// time map in the kernel's fixed point.  Plain C++ (no HIP): tests/emu/drift_plan_check.cpp builds it alone.
#pragma once
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/hpfw_gpu.h"

namespace hpfw {

constexpr int kWarpPB = 12, kWarpP = 1 << kWarpPB; // phase rows: row p is the fractional delay p / P
constexpr int kWarpH = 16, kWarpT = 2 * kWarpH;    // taps per row
constexpr int kWarpFrac = 40;                      // fraction bits of the position
constexpr int64_t kWarpDMax = (int64_t)1 << 30, kWarpGMax = (int64_t)1 << 17, kWarpMEnd = (int64_t)1 << 31;
constexpr int64_t kWarpI0Max = (int64_t)1 << 62, kWarpMaxRange = (int64_t)1 << 46;

// nullptr when the track is valid, else what is wrong with it
inline const char *warp_check(const hpfw_warp_track &t, int64_t n_pcm)
{
    if (t.src_off < 0 || t.src_len < 0 || t.src_off > kWarpMaxRange || t.src_len > kWarpMaxRange) return "warp: source range outside any buffer";
    if (t.src_off > n_pcm || t.src_len > n_pcm - t.src_off) return "warp: source range outside the buffer";
    if (t.d > kWarpDMax || t.d < -kWarpDMax) return "warp: |d| above 2^30";
    if (t.f0 < 0 || t.f0 >= ((int64_t)1 << kWarpFrac)) return "warp: f0 outside [0, 2^40)";
    if (t.i0 > kWarpI0Max || t.i0 < -kWarpI0Max) return "warp: |i0| above 2^62";
    if (t.gain > kWarpGMax || t.gain < -kWarpGMax) return "warp: |gain| above 2^17";
    return nullptr;
}

// the integer sample the filter of output m is centred on: ip = i0 + m + floor((f0 + m d) / 2^40); it never decreases with m
inline int64_t warp_ip(const hpfw_warp_track &t, int64_t m) { return t.i0 + m + ((t.f0 + m * t.d) >> kWarpFrac); }

// the outputs [m_lo, m_hi] of 0 .. 2^31 - 1 whose taps x[ip - H + 1 .. ip + H] meet [0, src_len): (2^31, -1) when none does
inline void warp_reach(const hpfw_warp_track &t, int64_t *m_lo, int64_t *m_hi)
{
    *m_lo = kWarpMEnd;
    *m_hi = -1;
    if (t.src_len < 1) return;
    const int64_t ip_min = -(int64_t)kWarpH, ip_max = t.src_len + kWarpH - 2; // ip + H >= 0 and ip - H + 1 <= src_len - 1
    auto first_at_least = [&](int64_t want) { // the smallest m in [0, 2^31] with ip(m) >= want (2^31: none)
        int64_t lo = 0, hi = kWarpMEnd;
        while (lo < hi) {
            const int64_t mid = (lo + hi) / 2;
            if (warp_ip(t, mid) >= want) hi = mid;
            else lo = mid + 1;
        }
        return lo;
    };
    const int64_t a = first_at_least(ip_min), b = first_at_least(ip_max + 1) - 1;
    if (a <= b) {
        *m_lo = a;
        *m_hi = b;
    }
}

// ---- anchors of a pair ------------------------------------------------------------------------------------------------
// The overlap [s_lo, s_hi) of a pair in the recording's samples and the centre segment [q, q + len) refine would use for
// seg_len = anchor_len (len = min(anchor_len, overlap)).  Anchor t >= 1 on the right starts at q + t hop, on the left at
// q - t hop, each anchor_len samples, for as long as a whole anchor lies in the overlap.  starts (NULL to count):
// [centre, left 1 .. n_left, right 1 .. n_right].  < 0: invalid arguments, else the number of starts (cap must hold them).
inline int64_t drift_anchors(int64_t s_lo, int64_t s_hi, int64_t q, int64_t len, int64_t anchor_len, int64_t anchor_hop, int64_t *starts,
                             int64_t cap, int32_t *n_left, int32_t *n_right)
{
    if (anchor_len < 1 || anchor_hop < 1 || len < 1 || len > anchor_len || s_lo < 0 || q < s_lo || s_hi > kWarpMaxRange || q > s_hi ||
        len > s_hi - q)
        return -1;
    int64_t nl = 0, nr = 0;
    if (len == anchor_len) { // an overlap shorter than an anchor has its centre segment alone
        nl = (q - s_lo) / anchor_hop;
        nr = (s_hi - anchor_len - q) / anchor_hop;
    }
    if (nl > INT32_MAX || nr > INT32_MAX) return -1;
    if (n_left) *n_left = (int32_t)nl;
    if (n_right) *n_right = (int32_t)nr;
    const int64_t n = 1 + nl + nr;
    if (!starts) return n;
    if (cap < n) return -1;
    starts[0] = q;
    for (int64_t t = 1; t <= nl; ++t) starts[t] = q - t * anchor_hop;
    for (int64_t t = 1; t <= nr; ++t) starts[nl + t] = q + t * anchor_hop;
    return n;
}

// ---- Theil-Sen --------------------------------------------------------------------------------------------------------
inline double drift_median(std::vector<double> &v)
{
    std::sort(v.begin(), v.end());
    const size_t k = v.size();
    return k & 1 ? v[k / 2] : (v[k / 2 - 1] + v[k / 2]) / 2.0;
}

// lag ~ a + b n: b the median of (lag_j - lag_i) / (n_j - n_i) over the pairs i < j with n_i != n_j, a the median of
// lag_i - b n_i, rms the root mean square of lag_i - (a + b n_i); float64 in exactly this order.  Fewer than 3 points (or no
// pair with different n): b = 0 and a = lag[0] (the caller puts the centre anchor first); no point: all 0.
inline void drift_fit(const int64_t *n, const int64_t *lag, int64_t count, double *a, double *b, double *rms)
{
    *a = *b = *rms = 0.0;
    if (count < 1) return;
    std::vector<double> v;
    if (count >= 3) {
        v.reserve((size_t)count * (size_t)(count - 1) / 2);
        for (int64_t i = 0; i < count; ++i)
            for (int64_t j = i + 1; j < count; ++j)
                if (n[j] != n[i]) v.push_back((double)(lag[j] - lag[i]) / (double)(n[j] - n[i]));
    }
    if (v.empty()) {
        *a = (double)lag[0];
    } else {
        *b = drift_median(v);
        v.clear();
        for (int64_t i = 0; i < count; ++i) v.push_back((double)lag[i] - *b * (double)n[i]);
        *a = drift_median(v);
    }
    double ss = 0.0;
    for (int64_t i = 0; i < count; ++i) {
        const double e = (double)lag[i] - (*a + *b * (double)n[i]);
        ss += e * e;
    }
    *rms = std::sqrt(ss / (double)count);
}

// ---- the time map -----------------------------------------------------------------------------------------------------
// Source sample n sits at t = A + (1 + B) n of the common timeline; output m reads the source at (m - A) / (1 + B)
// = m + pos0 + m r with r = 1 / (1 + B) - 1 = -B / (1 + B) and pos0 = -A (1 + r).  d = round(r 2^40) (off by at most 2^-41
// per output), i0 + f0 2^-40 = pos0 rounded to the nearest 2^-40.  In extended precision (64-bit significand) r carries a
// relative error below 2^-62 and A r, at most 2^20 for |A| <= 2^30, an absolute one below 2^-42: with the rounding's 2^-41
// the constant term stays within 2^-40, the bound of DESIGN.md section 16.  false: |r| > 2^-10, |A| > 2^30 or not a number.
inline bool time_map_q40(double A, double B, int64_t *i0, int64_t *f0, int64_t *d)
{
#if !defined(__HIP_DEVICE_COMPILE__)
    static_assert(LDBL_MANT_DIG >= 64, "the time map needs a 64-bit significand");
#endif
    if (!(A == A) || !(B == B) || !(std::fabs(A) <= 1073741824.0) || !(std::fabs(B) <= 0.5)) return false;
    const long double one = 1.0L, scale = 1099511627776.0L; // 2^40
    const long double r = -(long double)B / (one + (long double)B);
    if (!(fabsl(r) <= 0.0009765625L)) return false; // 2^-10
    *d = (int64_t)llrintl(r * scale);
    const long double whole = floorl(-(long double)A), part = (-(long double)A - whole) - (long double)A * r; // pos0 = whole + part
    const long double pw = floorl(part);
    int64_t i = (int64_t)whole + (int64_t)pw, f = (int64_t)llrintl((part - pw) * scale);
    if (f >= ((int64_t)1 << kWarpFrac)) {
        f -= (int64_t)1 << kWarpFrac;
        ++i;
    }
    *i0 = i;
    *f0 = f;
    return true;
}

} // namespace hpfw
