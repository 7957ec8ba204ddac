// timeline.cpp -- the host-only parts of the timeline of a long recording (include/hpfw_gpu.h): the
// score of a hit from its row's integer moments, the number of windows of a recording, and the segments of a list of
// per-window hits.  No device, no handle: every binding calls these, so the numbers are the same everywhere.
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>

#include "legacy_internal.h"

namespace {
int fail(int code, const char *msg)
{
    hpfw_internal_set_error(msg);
    return code;
}
} // namespace

extern "C" {

int hpfw_gpu_hit_score(uint32_t dist, int counted, const hpfw_dist_stats *s, double *score)
{
    if (!s || !score) return fail(HPFW_E_INVALID, "null argument");
    *score = std::numeric_limits<double>::quiet_NaN();
    if (!counted || s->n < 3) return 0;
    const uint64_t d = dist;
    if (d > s->sum || d * d > s->sum_sq || s->sum - d > (uint64_t)INT64_MAX) return fail(HPFW_E_INVALID, "moments no set of distances has");
    const __int128 np = (__int128)s->n - 1, rest = (__int128)(s->sum - d);
    const __int128 var_num = np * (__int128)(s->sum_sq - d * d) - rest * rest; // n'^2 var
    if (var_num < 0) return fail(HPFW_E_INVALID, "moments no set of distances has");
    if (var_num == 0) return 0;
    const __int128 mean_num = rest - np * (__int128)d; // n' (m - d)
    // (m - d) / sqrt(var) = (mean_num / n') / (sqrt(var_num) / n')
    *score = ((double)mean_num / (double)np) / (std::sqrt((double)var_num) / (double)np);
    return 0;
}

int hpfw_gpu_window_count(int64_t n_total, int64_t win, int64_t hop, int64_t *n_w)
{
    if (!n_w) return fail(HPFW_E_INVALID, "null argument");
    if (n_total < 0) return fail(HPFW_E_INVALID, "windows: n_total must not be negative");
    if (hop < 1 || hop > win) return fail(HPFW_E_INVALID, "windows: 1 <= hop <= win");
    if (hpfw_gpu_supported_length(win) != win) return fail(HPFW_E_INVALID, "windows: win is not a supported clip length");
    *n_w = n_total < win ? 0 : (n_total - win) / hop + 1;
    return 0;
}

int hpfw_gpu_timeline_segments(const hpfw_window_hit *w, int64_t n_w, const hpfw_timeline_params *p, hpfw_segment *out, int64_t cap,
                               int64_t *n_seg)
{
    if (!p || !n_seg || n_w < 0 || cap < 0 || (n_w && !w) || (cap && !out)) return fail(HPFW_E_INVALID, "bad argument");
    if (!(p->min_score > 0)) return fail(HPFW_E_INVALID, "timeline: min_score is required and must be positive");
    if (!(p->hop_cols > 0) || !std::isfinite(p->hop_cols)) return fail(HPFW_E_INVALID, "timeline: hop_cols must be positive and finite");
    if (!(p->tol_cols >= 0)) return fail(HPFW_E_INVALID, "timeline: tol_cols must not be negative");
    if (p->hop < 1 || p->hop > p->win) return fail(HPFW_E_INVALID, "timeline: 1 <= hop <= win");
    if (p->max_gap < -1 || p->min_windows < 0) return fail(HPFW_E_INVALID, "timeline: max_gap >= 0 (-1: default), min_windows >= 1 (0: default)");
    const double tol = p->tol_cols > 0 ? p->tol_cols : std::fmax(2.0, 0.08 * p->hop_cols);
    const int64_t max_gap = p->max_gap < 0 ? 1 : p->max_gap;
    const int min_windows = p->min_windows == 0 ? 1 : p->min_windows;

    int64_t kept = 0;
    bool open = false;
    hpfw_segment seg{};
    int64_t l = 0; // the open segment's last accepted window
    auto close = [&] {
        if (open && seg.n_strong >= min_windows) {
            if (kept < cap) out[kept] = seg;
            ++kept;
        }
        open = false;
    };
    for (int64_t i = 0; i < n_w; ++i) {
        const hpfw_window_hit &x = w[i];
        if (x.clip == 0xffffffffu || !(x.score >= p->min_score)) continue; // not strong (a NaN score fails the comparison)
        bool cont = false;
        if (open && x.clip == seg.clip && i - l - 1 <= max_gap) {
            const double t_w = (double)i * p->hop_cols, t_l = (double)l * p->hop_cols;
            const double res = ((double)x.offset - (double)w[l].offset) - w[l].tempo * (t_w - t_l);
            cont = std::fabs(res) <= tol * (double)(i - l);
        }
        if (cont) {
            seg.last = i;
            seg.end = i * p->hop + p->win;
            ++seg.n_strong;
            if (x.score > seg.best_score) {
                seg.best_window = i;
                seg.best_score = x.score;
                seg.best_tempo = x.tempo;
                seg.best_offset = x.offset;
                seg.best_variant = x.variant;
            }
        } else {
            close();
            open = true;
            seg = hpfw_segment{x.clip, 1, i, i, i * p->hop, i * p->hop + p->win, i, x.score, x.tempo, x.offset, x.variant, x.offset, 0};
        }
        l = i;
    }
    close();
    *n_seg = kept;
    return 0;
}

} // extern "C"
