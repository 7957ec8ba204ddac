// timeline.cpp -- the host-only parts of the timeline of a long recording (include/hpfw_gpu.h): the
// score of a hit from its row's integer moments, the number of windows of a recording, and the segments of a list of
// per-window hits, all at once or push by push.  No device, no handle: every binding calls these, so
// the numbers are the same everywhere.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <deque>
#include <functional>
#include <limits>
#include <string>

#include "legacy_internal.h"

namespace {
int fail(int code, const char *msg)
{
    hpfw_internal_set_error(msg);
    return code;
}

// the parameter checks of the segment rule, with their messages
int check_params(const hpfw_timeline_params *p)
{
    if (!(p->min_score > 0)) return fail(HPFW_E_INVALID, "timeline: min_score is required and must be positive");
    if (!(p->hop_cols > 0) || !std::isfinite(p->hop_cols)) return fail(HPFW_E_INVALID, "timeline: hop_cols must be positive and finite");
    if (!(p->tol_cols >= 0)) return fail(HPFW_E_INVALID, "timeline: tol_cols must not be negative");
    if (p->hop < 1 || p->hop > p->win) return fail(HPFW_E_INVALID, "timeline: 1 <= hop <= win");
    if (p->max_gap < -1 || p->min_windows < 0) return fail(HPFW_E_INVALID, "timeline: max_gap >= 0 (-1: default), min_windows >= 1 (0: default)");
    return 0;
}

// The rule of include/hpfw_gpu.h, one window at a time.  A segment is closed as soon as nothing can continue it: by a strong
// window that does not continue it, or once window l + max_gap + 1 has passed without continuing it (l: its last accepted
// window; a later window lies more than max_gap windows behind l).  Closing then instead of at the next strong window or at
// the end of the list changes no segment: the whole list at once and the list push by push give the same bytes.
struct Segmenter {
    hpfw_timeline_params p;
    double tol;
    int64_t max_gap;
    int min_windows;
    std::function<void(const hpfw_segment &)> keep; // receives every closed segment of at least min_windows strong windows
    bool open = false;
    hpfw_segment seg{};
    int64_t i = 0;    // the number of the next window
    int64_t l = 0;    // the open segment's last accepted window, its offset and tempo
    int32_t l_offset = 0;
    double l_tempo = 1.0;

    Segmenter(const hpfw_timeline_params &p_, std::function<void(const hpfw_segment &)> keep_)
        : p(p_), tol(p_.tol_cols > 0 ? p_.tol_cols : std::fmax(2.0, 0.08 * p_.hop_cols)), max_gap(p_.max_gap < 0 ? 1 : p_.max_gap),
          min_windows(p_.min_windows == 0 ? 1 : p_.min_windows), keep(std::move(keep_))
    {
    }
    void close()
    {
        if (open && seg.n_strong >= min_windows) keep(seg);
        open = false;
    }
    void step(const hpfw_window_hit &x)
    {
        if (x.clip != 0xffffffffu && x.score >= p.min_score) { // strong (a NaN score fails the comparison)
            bool cont = false;
            if (open && x.clip == seg.clip && i - l - 1 <= max_gap) {
                const double t_w = (double)i * p.hop_cols, t_l = (double)l * p.hop_cols;
                const double res = ((double)x.offset - (double)l_offset) - l_tempo * (t_w - t_l);
                cont = std::fabs(res) <= tol * (double)(i - l);
            }
            if (cont) {
                seg.last = i;
                seg.end = i * p.hop + p.win;
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
                seg = hpfw_segment{x.clip, 1, i, i, i * p.hop, i * p.hop + p.win, i, x.score, x.tempo, x.offset, x.variant, x.offset, 0};
            }
            l = i;
            l_offset = x.offset;
            l_tempo = x.tempo;
        } else if (open && i - l > max_gap) { // window l + max_gap + 1 did not continue it: no later one can
            close();
        }
        ++i;
    }
};
} // namespace

struct hpfw_timeline_tracker {
    std::deque<hpfw_segment> closed; // closed and kept, not yet popped
    Segmenter sg;
    explicit hpfw_timeline_tracker(const hpfw_timeline_params &p) : sg(p, [this](const hpfw_segment &s) { closed.push_back(s); }) {}
};

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

int hpfw_gpu_overlap_rate(uint32_t dist, uint32_t overlap, uint32_t *rate)
{
    if (!rate) return fail(HPFW_E_INVALID, "null argument");
    if (overlap == 0 || overlap > 16000) return fail(HPFW_E_INVALID, "overlap rate: overlap must be in 1..16000");
    if (dist > 64 * overlap) return fail(HPFW_E_INVALID, "overlap rate: dist above 64 overlap");
    *rate = (dist << HPFW_OVERLAP_RATE_BITS) / overlap; // below 2^30: the division the device does
    return 0;
}

int hpfw_gpu_overlap_extent(int32_t lag, int64_t n_clip, int64_t k_q, int64_t span, int64_t win, int64_t m, int64_t *a, int64_t *b)
{
    if (!a || !b) return fail(HPFW_E_INVALID, "null argument");
    if (n_clip < 1 || k_q < 1 || span < 1 || win < 1 || m < 1) return fail(HPFW_E_INVALID, "overlap extent: n_clip, k_q, span, win and m must be positive");
    const int64_t d = lag;
    if (std::min(k_q, n_clip - d) - std::max<int64_t>(0, -d) < 1) return fail(HPFW_E_INVALID, "overlap extent: the window and the clip share no hashprint at this lag");
    const double col = 3.0 * (double)win / (double)m;
    const int64_t a_cols = std::max<int64_t>(0, -d), b_cols = std::min(k_q + span - 1, n_clip + span - 1 - d);
    *a = (int64_t)std::floor((double)a_cols * col + 0.5);
    *b = std::min(win, (int64_t)std::floor((double)b_cols * col + 0.5));
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
    if (int rc = check_params(p)) return rc;
    int64_t kept = 0;
    Segmenter sg(*p, [&](const hpfw_segment &seg) {
        if (kept < cap) out[kept] = seg;
        ++kept;
    });
    for (int64_t i = 0; i < n_w; ++i) sg.step(w[i]);
    sg.close();
    *n_seg = kept;
    return 0;
}

// ---- the same rule one push at a time ----
int hpfw_gpu_timeline_tracker_create(const hpfw_timeline_params *p, hpfw_timeline_tracker **out)
{
    if (!p || !out) return fail(HPFW_E_INVALID, "bad argument");
    if (int rc = check_params(p)) return rc;
    *out = new hpfw_timeline_tracker(*p);
    return 0;
}

void hpfw_gpu_timeline_tracker_destroy(hpfw_timeline_tracker *t) { delete t; }

int hpfw_gpu_timeline_tracker_push(hpfw_timeline_tracker *t, const hpfw_window_hit *w, int64_t n_w)
{
    if (!t || n_w < 0 || (n_w && !w)) return fail(HPFW_E_INVALID, "bad argument");
    for (int64_t i = 0; i < n_w; ++i) t->sg.step(w[i]);
    return 0;
}

int hpfw_gpu_timeline_tracker_pop(hpfw_timeline_tracker *t, hpfw_segment *out, int64_t cap, int64_t *n)
{
    if (!t || !n || cap < 0 || (cap && !out)) return fail(HPFW_E_INVALID, "bad argument");
    int64_t got = 0;
    for (; got < cap && !t->closed.empty(); ++got) {
        out[got] = t->closed.front();
        t->closed.pop_front();
    }
    *n = got;
    return 0;
}

int hpfw_gpu_timeline_tracker_open(hpfw_timeline_tracker *t, hpfw_segment *cur, int *has)
{
    if (!t || !cur || !has) return fail(HPFW_E_INVALID, "bad argument");
    *has = t->sg.open ? 1 : 0;
    if (t->sg.open) *cur = t->sg.seg;
    return 0;
}

int hpfw_gpu_timeline_tracker_finish(hpfw_timeline_tracker *t)
{
    if (!t) return fail(HPFW_E_INVALID, "bad argument");
    t->sg.close();
    return 0;
}

} // extern "C"
