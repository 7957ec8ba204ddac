// timeline.h -- the set list of one long recording: windows of the recording hashed on the extractor's
// handle `h` (which holds the index's filters), each searched in a GpuStorage for its best clip and scored by how far that
// clip stands out from the others (hpfw_gpu_hit_score), and the windows that name one clip at consistent offsets joined into
// segments (hpfw_gpu_timeline_segments).  With tempos and / or shifts every window is searched under every variant, as
// tempo.h / transposed.h describe them; projection mode 1 then.  A ShardedGpuStorage (sharded_storage.h) in place of the
// GpuStorage gives the same timeline from an index sharded over several devices: the windows are hashed on its shards under
// h's filters and the searches are the group's (include/hpfw_gpu_multi_search.h).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../hpfw_gpu.h"
#include "../../hpfw_gpu_multi_search.h" // (declarations only: a program that uses no sharded storage links libhpfw_gpu alone)

namespace hpfw {

struct TimelineOptions {
    double min_score = 0;          ///< REQUIRED, > 0: there is no default
    int64_t win = 220500;          ///< window and hop in samples at 44.1 kHz; win must be a supported clip length
    int64_t hop = 110250;
    std::vector<float> tempos;     ///< empty: the recording's own tempo only
    std::vector<int32_t> shifts;   ///< empty: the recording's own key only
    double tol_cols = 0;           ///< 0: the default max(2, 0.08 hop in columns)
    int max_gap = 1, min_windows = 1;
    int min_overlap = 0;           ///< 0: the plain rule.  N > 0: every window is searched by the overlap rule over at least N
                                   ///< hashprints; no tempos, no shifts, no sharded storage then
    /// search within a subset of the index.  Empty: the whole index.  hpfw::timeline takes one entry,
    /// hpfw::LiveStreams one entry for all feeds or one per feed; an entry is the clip ids (positions in the storage, strictly
    /// ascending) its windows are searched within, or nullopt for the whole index.  Scores are then against the moments of the
    /// set's clips (NaN below three counted clips).  Not with min_overlap and not with a sharded storage.
    std::vector<std::optional<std::vector<int32_t>>> within;
};

struct TimelineSegment {
    std::string filename;          ///< the clip's name in the storage
    uint32_t clip;
    double start_s, end_s;         ///< the segment in the recording
    double score;                  ///< of its best window, with that window's shift and tempo
    double offset_s;               ///< where in the indexed recording the first window starts
    int32_t shift;
    float tempo;
    hpfw_segment raw;
};

struct Timeline {
    std::vector<hpfw_window_hit> windows; ///< the best hit of every window (min_overlap: offset is the lag)
    std::vector<uint32_t> overlaps;       ///< min_overlap: the hashprints every window's hit was compared over; empty otherwise
    std::vector<TimelineSegment> segments;
};

namespace detail {
/// what min_overlap > 0 refuses, before anything runs on a device; nhp: the hashprints of a window
inline void check_min_overlap(const TimelineOptions &opt, bool sharded, int64_t nhp)
{
    if (opt.min_overlap == 0) return;
    if (!opt.tempos.empty() || !opt.shifts.empty()) throw std::runtime_error("hpfw: min_overlap: the overlap rule has no shifts and no tempos (HPFW_E_UNSUPPORTED)");
    if (sharded) throw std::runtime_error("hpfw: min_overlap: the overlap search is not available on a sharded index (HPFW_E_UNSUPPORTED)");
    if (opt.min_overlap < 1 || opt.min_overlap > nhp) throw std::runtime_error("hpfw: min_overlap must be in 1.." + std::to_string(nhp) + ", the hashprints of a window (HPFW_E_INVALID)");
}

/// TimelineOptions::within as the C ABI takes it, for `owners` owners of windows (1: hpfw::timeline; the feeds of
/// hpfw::LiveStreams): the sets in CSR form and the set of each owner (-1: the whole index).  `any` is false when nothing is
/// restricted.  Refuses, before anything runs on a device, what within does not go with.
struct WithinSets {
    std::vector<int64_t> set_off{0};
    std::vector<int32_t> set_clips, owner_set;
    bool any = false;
};
inline WithinSets within_sets(const TimelineOptions &opt, bool sharded, int owners)
{
    WithinSets ws;
    if (opt.within.empty()) return ws;
    if (opt.min_overlap != 0) throw std::runtime_error("hpfw: within: the overlap rule does not search within a set (HPFW_E_UNSUPPORTED)");
    if (sharded) throw std::runtime_error("hpfw: within: the search within a set is not available on a sharded index (HPFW_E_UNSUPPORTED)");
    if (opt.within.size() != 1 && (int)opt.within.size() != owners) throw std::runtime_error("hpfw: within: one entry, or one per feed (HPFW_E_INVALID)");
    for (int i = 0; i < owners; ++i) {
        const auto &w = opt.within[opt.within.size() == 1 ? 0 : (size_t)i];
        ws.owner_set.push_back(w ? (int32_t)ws.set_off.size() - 1 : -1);
        if (!w) continue;
        ws.any = true;
        ws.set_clips.insert(ws.set_clips.end(), w->begin(), w->end());
        ws.set_off.push_back((int64_t)ws.set_clips.size());
    }
    ws.set_clips.push_back(0); // (never empty: data() is a pointer the call may be given)
    return ws;
}

/// the best hit of n_w windows of nhp hashprints each by the overlap rule, scored by its rate among the rates of the
/// counted clips: x.offset is the lag; 0 on success (the library's status otherwise)
inline int search_windows_overlap(hpfw_gpu *index, const uint64_t *hp, int64_t n_w, int64_t nhp, int min_overlap, hpfw_window_hit *x,
                                  uint32_t *overlaps)
{
    std::vector<int64_t> q_off((size_t)n_w + 1);
    for (size_t i = 0; i < q_off.size(); ++i) q_off[i] = (int64_t)i * nhp;
    std::vector<hpfw_overlap_hit> hits((size_t)n_w);
    std::vector<hpfw_dist_stats> stats((size_t)n_w);
    if (int rc = hpfw_gpu_search_overlap_scored(index, hp, q_off.data(), n_w, nullptr, min_overlap, 1, hits.data(), stats.data())) return rc;
    for (int64_t w = 0; w < n_w; ++w) {
        const hpfw_overlap_hit &hit = hits[(size_t)w];
        x[w] = {hit.clip, hit.lag, 0, 0, 1.0, std::numeric_limits<double>::quiet_NaN()};
        overlaps[w] = hit.overlap;
        if (hit.clip == 0xffffffffu) continue;
        uint32_t rate = 0;
        if (int rc = hpfw_gpu_overlap_rate(hit.dist, hit.overlap, &rate)) return rc;
        if (int rc = hpfw_gpu_hit_score(rate, 1, &stats[(size_t)w], &x[w].score)) return rc;
    }
    return 0;
}

/// start_s, end_s and offset_s of a segment found by the overlap rule: the part of its first and last window that lies on
/// the clip of n_clip hashprints (hpfw_gpu_overlap_extent); g: the window's geometry
template <typename Segment>
int trim_segment(Segment &seg, int32_t first_lag, int32_t last_lag, int64_t n_clip, const hpfw_geometry &g, int64_t win, int64_t hop)
{
    int64_t a = 0, b = 0, unused = 0;
    const int64_t span = g.c - g.n_hp + 1;
    if (int rc = hpfw_gpu_overlap_extent(first_lag, n_clip, g.n_hp, span, win, g.m, &a, &unused)) return rc;
    if (int rc = hpfw_gpu_overlap_extent(last_lag, n_clip, g.n_hp, span, win, g.m, &unused, &b)) return rc;
    seg.start_s = (double)(seg.raw.first * hop + a) / 44100.0;
    seg.end_s = (double)(seg.raw.last * hop + b) / 44100.0;
    seg.offset_s = (double)std::max(first_lag, 0) * (3.0 * (double)win / (double)g.m / 44100.0);
    return 0;
}
} // namespace detail

/// `path`: a 44.1 kHz PCM16 WAV file (hpfw_gpu_wav_read_pcm16).  A recording shorter than one window has no window and no
/// segment; throws std::runtime_error with the library's message on failure.
template <typename Storage>
Timeline timeline(const Storage &storage, hpfw_gpu *h, const std::string &path, const TimelineOptions &opt)
{
    auto fail = [](const char *what) { throw std::runtime_error(std::string("hpfw::timeline: ") + what + ": " + hpfw_gpu_last_error()); };
    constexpr bool sharded = requires { storage.group(); };
    int64_t n = 0, n_w = 0;
    if (hpfw_gpu_window_count(0, opt.win, opt.hop, &n_w) != 0) fail("windows");
    hpfw_geometry g;
    if (hpfw_gpu_geometry(h, opt.win, &g) != 0) fail("geometry");
    detail::check_min_overlap(opt, sharded, g.n_hp);
    const detail::WithinSets ws = detail::within_sets(opt, sharded, 1);
    if (hpfw_gpu_wav_read_pcm16(path.c_str(), nullptr, 0, &n) != 0) fail(path.c_str());
    std::vector<int16_t> pcm((size_t)std::max<int64_t>(n, 1));
    if (hpfw_gpu_wav_read_pcm16(path.c_str(), pcm.data(), n, &n) != 0) fail(path.c_str());
    if (hpfw_gpu_window_count(n, opt.win, opt.hop, &n_w) != 0) fail("windows");
    Timeline out;
    if (n_w == 0) return out;
    int64_t nhp = g.n_hp;
    if (!opt.tempos.empty()) {
        int64_t ct = 0;
        if (hpfw_gpu_tempo_columns(g.c, opt.tempos.data(), (int)opt.tempos.size(), &ct) != 0) fail("tempos");
        nhp = std::max<int64_t>(ct - 99, 0);
    }
    const int n_s = (int)std::max<size_t>(opt.shifts.size(), 1);
    const int sets = (int)std::max<size_t>(opt.tempos.size(), 1) * n_s;
    const bool variants = !opt.tempos.empty() || !opt.shifts.empty();
    std::vector<uint64_t> hp((size_t)(n_w * sets * nhp));
    const float *tempos = opt.tempos.empty() ? nullptr : opt.tempos.data();
    const int32_t *shifts = opt.shifts.empty() ? nullptr : opt.shifts.data();
    if constexpr (sharded) { // the shards hash the windows, under the extractor's filters and projection mode
        std::vector<float> filters((size_t)HPFW_FILTERS * HPFW_FRAME_SIZE);
        if (hpfw_gpu_get_filters(h, filters.data()) != 0 || hpfw_gpu_group_set_filters(storage.group(), filters.data()) != 0) fail("filters");
        for (int i = 0; i < storage.shards(); ++i)
            if (hpfw_gpu_set_projection(hpfw_gpu_group_handle(storage.group(), i), hpfw_gpu_get_projection(h)) != 0) fail("projection");
        if (hpfw_gpu_group_extract_windows_pcm16(storage.group(), pcm.data(), n, opt.win, opt.hop, tempos, (int)opt.tempos.size(), shifts,
                                                 (int)opt.shifts.size(), hp.data()) != 0)
            fail("extraction");
    } else if (hpfw_gpu_extract_windows_pcm16_host(h, pcm.data(), n, opt.win, opt.hop, tempos, (int)opt.tempos.size(), shifts,
                                                   (int)opt.shifts.size(), hp.data()) != 0)
        fail("extraction");
    const hpfw_timeline_params p{opt.min_score, (double)opt.hop * (double)g.m / (3.0 * (double)opt.win), opt.tol_cols, opt.win, opt.hop,
                                 opt.max_gap, opt.min_windows};
    const double col_s = 3.0 * (double)opt.win / (double)g.m / 44100.0; // one index column in seconds
    std::vector<hpfw_segment> segs((size_t)n_w);
    int64_t n_seg = 0;
    if constexpr (!sharded) {
        if (opt.min_overlap > 0) { // the overlap rule: lags in place of offsets, segments trimmed to the clip
            out.windows.resize((size_t)n_w);
            out.overlaps.resize((size_t)n_w);
            if (detail::search_windows_overlap(storage.handle(), hp.data(), n_w, nhp, opt.min_overlap, out.windows.data(), out.overlaps.data()) != 0)
                fail("search");
            std::vector<int64_t> db_off(storage.names().size() + 1, 0);
            if (hpfw_gpu_index_get(storage.handle(), db_off.data(), nullptr, 0) != 0) fail("index");
            if (hpfw_gpu_timeline_segments(out.windows.data(), n_w, &p, segs.data(), n_w, &n_seg) != 0) fail("segments");
            for (int64_t i = 0; i < n_seg; ++i) {
                const hpfw_segment &s = segs[(size_t)i];
                out.segments.push_back({storage.names()[s.clip], s.clip, 0.0, 0.0, s.best_score, 0.0, 0, (float)s.best_tempo, s});
                if (detail::trim_segment(out.segments.back(), out.windows[(size_t)s.first].offset, out.windows[(size_t)s.last].offset,
                                         db_off[s.clip + 1] - db_off[s.clip], g, opt.win, opt.hop) != 0)
                    fail("extent");
            }
            return out;
        }
    }
    std::vector<int64_t> q_off((size_t)(n_w * sets) + 1);
    for (size_t i = 0; i < q_off.size(); ++i) q_off[i] = (int64_t)i * nhp;
    std::vector<hpfw_dist_stats> stats((size_t)(n_w * sets));
    std::vector<hpfw_shift_hit> hits((size_t)n_w);
    std::vector<hpfw_hit> plain(variants ? 0 : (size_t)n_w);
    int rc;
    if constexpr (sharded)
        rc = variants ? hpfw_gpu_group_search_topk_transposed_scored(storage.group(), hp.data(), q_off.data(), n_w, sets, 1, hits.data(), stats.data())
                      : hpfw_gpu_group_search_topk_scored(storage.group(), hp.data(), q_off.data(), n_w, 1, plain.data(), stats.data());
    else if (ws.any) { // every window within the one set
        const std::vector<int32_t> q_set((size_t)n_w, ws.owner_set[0]);
        const int n_sets = (int)ws.set_off.size() - 1;
        rc = variants ? hpfw_gpu_search_topk_transposed_within(storage.handle(), hp.data(), q_off.data(), n_w, sets, 1, ws.set_off.data(), n_sets,
                                                               ws.set_clips.data(), q_set.data(), hits.data(), stats.data())
                      : hpfw_gpu_search_topk_within(storage.handle(), hp.data(), q_off.data(), n_w, 1, ws.set_off.data(), n_sets,
                                                    ws.set_clips.data(), q_set.data(), plain.data(), stats.data());
    } else
        rc = variants ? hpfw_gpu_search_topk_transposed_scored(storage.handle(), hp.data(), q_off.data(), n_w, sets, 1, hits.data(), stats.data())
                      : hpfw_gpu_search_topk_scored(storage.handle(), hp.data(), q_off.data(), n_w, 1, plain.data(), stats.data());
    if (rc != 0) fail("search");
    if (!variants)
        for (int64_t w = 0; w < n_w; ++w) hits[(size_t)w] = {plain[(size_t)w].dist, plain[(size_t)w].clip, plain[(size_t)w].offset, 0};
    std::vector<int64_t> db_off(storage.names().size() + 1, 0);
    if constexpr (sharded)
        db_off = storage.index_offsets();
    else if (hpfw_gpu_index_get(storage.handle(), db_off.data(), nullptr, 0) != 0)
        fail("index");
    out.windows.resize((size_t)n_w);
    for (int64_t w = 0; w < n_w; ++w) {
        const hpfw_shift_hit &hit = hits[(size_t)w];
        hpfw_window_hit &x = out.windows[(size_t)w];
        x = {hit.clip, hit.offset, std::max(hit.shift_index, 0), 0, 1.0, std::numeric_limits<double>::quiet_NaN()};
        if (hit.clip == 0xffffffffu) continue;
        if (!opt.tempos.empty()) x.tempo = opt.tempos[(size_t)(x.variant / n_s)];
        const int counted = db_off[hit.clip + 1] - db_off[hit.clip] >= nhp;
        if (hpfw_gpu_hit_score(hit.dist, counted, &stats[(size_t)(w * sets + x.variant)], &x.score) != 0) fail("score");
    }
    if (hpfw_gpu_timeline_segments(out.windows.data(), n_w, &p, segs.data(), n_w, &n_seg) != 0) fail("segments");
    for (int64_t i = 0; i < n_seg; ++i) {
        const hpfw_segment &s = segs[(size_t)i];
        out.segments.push_back({storage.names()[s.clip], s.clip, (double)s.start / 44100.0, (double)s.end / 44100.0, s.best_score,
                                s.first_offset * col_s, opt.shifts.empty() ? 0 : opt.shifts[(size_t)(s.best_variant % n_s)],
                                (float)s.best_tempo, s});
    }
    return out;
}

} // namespace hpfw
