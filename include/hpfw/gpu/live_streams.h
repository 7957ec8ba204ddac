// live_streams.h -- hpfw::LiveStreams: the timeline of feeds that are still running.  Chunks of mono
// PCM16 are appended to any of n_streams feeds (at 44.1 kHz, or with LiveStreamsOptions::resample at any rate in [8 000, 192 000]
// Hz, converted chunk by chunk on the GPU exactly as a file at that rate is); every window that has become complete is hashed on the extractor's handle
// `h` (which holds the index's filters) in one extraction pass over all feeds, searched in a GpuStorage or a ShardedGpuStorage
// and scored exactly as hpfw::timeline (timeline.h) does it, and a segmenter per feed hands out each segment as soon as nothing
// can continue it.  What a feed yields is, window for window and segment for segment, what hpfw::timeline yields for a file that
// holds everything pushed to the feed, however the samples were cut into chunks.
#pragma once

#include <map>
#include <memory>
#include <optional>

#include "timeline.h"

namespace hpfw {

struct LiveStreamsOptions : TimelineOptions {
    int64_t capacity = 0;      ///< samples per feed's ring, >= win; 0: 2 win.  A push may not bring more than the ring has room for
    bool keep_windows = false; ///< windows() holds the best hit of every window of the last push
    int rate = 44100;          ///< the feeds' sample rate; another rate than 44 100 Hz needs `resample`
    bool resample = false;     ///< take feeds at other rates, as GpuCollector's switch takes files (refused without it)
    std::vector<int> rates;    ///< one rate per feed; empty: `rate` for all.  Chunks and LiveChunk::n count at the feed's rate
};

struct LiveChunk {
    int feed;
    const int16_t *pcm;
    int64_t n;
};

struct LiveSegment {
    int feed;
    TimelineSegment segment; ///< start_s / end_s count from the feed's start (its last reset)
};

struct LiveWindow {
    int feed;
    int64_t window;
    hpfw_window_hit hit;
};

template <typename Storage>
class LiveStreams {
public:
    /// `storage` and `h` outlive the object; throws std::runtime_error with the library's message on failure
    LiveStreams(const Storage &storage, hpfw_gpu *h, int n_streams, const LiveStreamsOptions &opt) : storage_(storage), opt_(opt)
    {
        std::vector<int32_t> rates(opt.rates.begin(), opt.rates.end());
        if (rates.empty()) rates.assign((size_t)std::max(n_streams, 0), opt.rate);
        if ((int)rates.size() != n_streams) throw std::runtime_error("hpfw::LiveStreams: one rate per feed");
        for (int32_t r : rates)
            if (r != 44100 && !opt.resample) throw std::runtime_error("hpfw::LiveStreams: feeds are 44.1 kHz mono PCM16");
        constexpr bool sharded = requires { storage.group(); };
        if (hpfw_gpu_geometry(h, opt.win, &g_) != 0) fail("geometry");
        detail::check_min_overlap(opt, sharded, g_.n_hp);
        within_ = detail::within_sets(opt, sharded, std::max(n_streams, 0));
        lags_.resize((size_t)std::max(n_streams, 0));
        hpfw_streams_params p{n_streams, (int32_t)opt.tempos.size(), (int32_t)opt.shifts.size(), 0, opt.win, opt.hop, opt.capacity,
                              opt.tempos.empty() ? nullptr : opt.tempos.data(), opt.shifts.empty() ? nullptr : opt.shifts.data()};
        hpfw_gpu_streams *s = nullptr;
        if (hpfw_gpu_streams_create_rates(h, &p, rates.empty() ? nullptr : rates.data(), &s) != 0) fail("create");
        s_.reset(s);
        if (hpfw_gpu_streams_info(s, &info_, nullptr, nullptr) != 0) fail("info");
        const hpfw_geometry &g = g_;
        col_s_ = 3.0 * (double)opt.win / (double)g.m / 44100.0; // one index column in seconds
        tp_ = {opt.min_score, (double)opt.hop * (double)g.m / (3.0 * (double)opt.win), opt.tol_cols, opt.win, opt.hop, opt.max_gap, opt.min_windows};
        for (int i = 0; i < n_streams; ++i) trackers_.emplace_back(tracker());
    }

    /// appends the chunks (at most one per feed; the feeds not named receive nothing), hashes and searches every window that
    /// has become complete, and returns the segments these windows closed, by feed and then in order
    std::vector<LiveSegment> push(const std::vector<LiveChunk> &chunks)
    {
        std::vector<int64_t> counts((size_t)info_.n_streams, 0);
        std::vector<const int16_t *> src((size_t)info_.n_streams, nullptr);
        for (const LiveChunk &c : chunks) {
            if (c.feed < 0 || c.feed >= info_.n_streams || c.n < 0 || counts[(size_t)c.feed]) throw std::runtime_error("hpfw::LiveStreams: bad chunk");
            counts[(size_t)c.feed] = c.n;
            src[(size_t)c.feed] = c.pcm;
        }
        pcm_.clear();
        for (size_t i = 0; i < counts.size(); ++i) pcm_.insert(pcm_.end(), src[i], src[i] + counts[i]);
        int64_t ready = 0;
        if (hpfw_gpu_streams_push(s_.get(), pcm_.empty() ? nullptr : pcm_.data(), counts.data(), &ready) != 0) fail("push");
        windows_.clear();
        if (ready == 0) return {};
        const int sets = info_.n_sets, n_s = (int)std::max<size_t>(opt_.shifts.size(), 1);
        const int64_t nhp = info_.per_window / sets;
        const bool variants = !opt_.tempos.empty() || !opt_.shifts.empty();
        std::vector<uint64_t> hp((size_t)(ready * info_.per_window));
        std::vector<hpfw_stream_window> which((size_t)ready);
        int64_t n_w = 0;
        if (hpfw_gpu_streams_extract_host(s_.get(), ready, hp.data(), nullptr, which.data(), &n_w) != 0) fail("extraction");
        constexpr bool sharded = requires { storage_.group(); };
        if constexpr (!sharded) {
            if (opt_.min_overlap > 0) return push_overlap(hp, which, n_w, nhp);
        }
        std::vector<int64_t> q_off((size_t)(n_w * sets) + 1);
        for (size_t i = 0; i < q_off.size(); ++i) q_off[i] = (int64_t)i * nhp;
        std::vector<hpfw_dist_stats> stats((size_t)(n_w * sets));
        std::vector<hpfw_shift_hit> hits((size_t)n_w);
        std::vector<hpfw_hit> plain(variants ? 0 : (size_t)n_w);
        int rc;
        if constexpr (sharded)
            rc = variants ? hpfw_gpu_group_search_topk_transposed_scored(storage_.group(), hp.data(), q_off.data(), n_w, sets, 1, hits.data(), stats.data())
                          : hpfw_gpu_group_search_topk_scored(storage_.group(), hp.data(), q_off.data(), n_w, 1, plain.data(), stats.data());
        else if (within_.any) { // every window within its feed's set, in the one search of the push
            std::vector<int32_t> q_set((size_t)n_w);
            for (int64_t w = 0; w < n_w; ++w) q_set[(size_t)w] = within_.owner_set[(size_t)which[(size_t)w].feed];
            const int n_sets = (int)within_.set_off.size() - 1;
            rc = variants ? hpfw_gpu_search_topk_transposed_within(storage_.handle(), hp.data(), q_off.data(), n_w, sets, 1, within_.set_off.data(),
                                                                   n_sets, within_.set_clips.data(), q_set.data(), hits.data(), stats.data())
                          : hpfw_gpu_search_topk_within(storage_.handle(), hp.data(), q_off.data(), n_w, 1, within_.set_off.data(), n_sets,
                                                        within_.set_clips.data(), q_set.data(), plain.data(), stats.data());
        } else
            rc = variants ? hpfw_gpu_search_topk_transposed_scored(storage_.handle(), hp.data(), q_off.data(), n_w, sets, 1, hits.data(), stats.data())
                          : hpfw_gpu_search_topk_scored(storage_.handle(), hp.data(), q_off.data(), n_w, 1, plain.data(), stats.data());
        if (rc != 0) fail("search");
        if (!variants)
            for (int64_t w = 0; w < n_w; ++w) hits[(size_t)w] = {plain[(size_t)w].dist, plain[(size_t)w].clip, plain[(size_t)w].offset, 0};
        std::vector<int64_t> db_off(storage_.names().size() + 1, 0);
        if constexpr (sharded)
            db_off = storage_.index_offsets();
        else if (hpfw_gpu_index_get(storage_.handle(), db_off.data(), nullptr, 0) != 0)
            fail("index");
        std::vector<LiveSegment> out;
        for (int64_t w = 0; w < n_w; ++w) { // (in order of feed and window: a feed's windows reach its tracker in order)
            const hpfw_shift_hit &hit = hits[(size_t)w];
            hpfw_window_hit x{hit.clip, hit.offset, std::max(hit.shift_index, 0), 0, 1.0, std::numeric_limits<double>::quiet_NaN()};
            if (hit.clip != 0xffffffffu) {
                if (!opt_.tempos.empty()) x.tempo = opt_.tempos[(size_t)(x.variant / n_s)];
                const int counted = db_off[hit.clip + 1] - db_off[hit.clip] >= nhp;
                if (hpfw_gpu_hit_score(hit.dist, counted, &stats[(size_t)(w * sets + x.variant)], &x.score) != 0) fail("score");
            }
            const int feed = which[(size_t)w].feed;
            if (opt_.keep_windows) windows_.push_back({feed, which[(size_t)w].window, x});
            if (hpfw_gpu_timeline_tracker_push(trackers_[(size_t)feed].get(), &x, 1) != 0) fail("tracker");
            if (w + 1 == n_w || which[(size_t)w + 1].feed != feed) pop(feed, out);
        }
        return out;
    }

    /// the segment in progress of a feed as it would close now, whatever min_windows ("now playing")
    std::optional<TimelineSegment> open(int feed) const
    {
        hpfw_segment cur;
        int has = 0;
        if (feed < 0 || feed >= info_.n_streams || hpfw_gpu_timeline_tracker_open(trackers_[(size_t)feed].get(), &cur, &has) != 0) fail("open");
        if (!has) return std::nullopt;
        return named(cur, feed);
    }

    /// closes the segment in progress of one feed, or of every feed (-1), and returns what that released
    std::vector<LiveSegment> finish(int feed = -1)
    {
        std::vector<LiveSegment> out;
        for (int i = 0; i < info_.n_streams; ++i) {
            if (feed >= 0 && i != feed) continue;
            if (hpfw_gpu_timeline_tracker_finish(trackers_[(size_t)i].get()) != 0) fail("finish");
            pop(i, out);
            lags_[(size_t)i].clear();
        }
        return out;
    }

    /// the feed starts again at sample 0 and window 0, with a new segmenter; its segment in progress is dropped
    void reset(int feed)
    {
        if (hpfw_gpu_streams_reset(s_.get(), feed) != 0) fail("reset");
        trackers_[(size_t)feed].reset(tracker());
        lags_[(size_t)feed].clear();
    }

    const std::vector<LiveWindow> &windows() const { return windows_; }
    const hpfw_streams_info &info() const { return info_; }

private:
    [[noreturn]] static void fail(const char *what) { throw std::runtime_error(std::string("hpfw::LiveStreams: ") + what + ": " + hpfw_gpu_last_error()); }

    hpfw_timeline_tracker *tracker() const
    {
        hpfw_timeline_tracker *t = nullptr;
        if (hpfw_gpu_timeline_tracker_create(&tp_, &t) != 0) fail("tracker");
        return t;
    }

    TimelineSegment named(const hpfw_segment &s, int feed) const
    {
        const int n_s = (int)std::max<size_t>(opt_.shifts.size(), 1);
        TimelineSegment seg{storage_.names()[s.clip], s.clip, (double)s.start / 44100.0, (double)s.end / 44100.0, s.best_score, s.first_offset * col_s_,
                            opt_.shifts.empty() ? 0 : opt_.shifts[(size_t)(s.best_variant % n_s)], (float)s.best_tempo, s};
        if constexpr (!requires { storage_.group(); }) {
            if (opt_.min_overlap > 0) { // the part of the first and last window that lies on the clip
                const auto &lags = lags_[(size_t)feed];
                // the clip's length as it was added: a segment open on a recording removed since (GpuStorage::remove) ends as
                // it would have ended had the feed stopped matching
                if (detail::trim_segment(seg, lags.at(s.first), lags.at(s.last), storage_.added_length(s.clip), g_, opt_.win, opt_.hop) != 0)
                    fail("extent");
            }
        }
        return seg;
    }

    /// push() by the overlap rule (opt.min_overlap > 0): the lag of every window is kept, from the first window of the feed's
    /// segment in progress on, for the extent of the segment that window may open or close
    std::vector<LiveSegment> push_overlap(const std::vector<uint64_t> &hp, const std::vector<hpfw_stream_window> &which, int64_t n_w, int64_t nhp)
    {
        std::vector<hpfw_window_hit> x((size_t)n_w);
        std::vector<uint32_t> overlaps((size_t)n_w);
        if (detail::search_windows_overlap(storage_.handle(), hp.data(), n_w, nhp, opt_.min_overlap, x.data(), overlaps.data()) != 0) fail("search");
        std::vector<LiveSegment> out;
        for (int64_t w = 0; w < n_w; ++w) {
            const int feed = which[(size_t)w].feed;
            lags_[(size_t)feed][which[(size_t)w].window] = x[(size_t)w].offset;
            if (opt_.keep_windows) windows_.push_back({feed, which[(size_t)w].window, x[(size_t)w]});
            if (hpfw_gpu_timeline_tracker_push(trackers_[(size_t)feed].get(), &x[(size_t)w], 1) != 0) fail("tracker");
            if (w + 1 == n_w || which[(size_t)w + 1].feed != feed) {
                pop(feed, out);
                hpfw_segment cur;
                int has = 0;
                if (hpfw_gpu_timeline_tracker_open(trackers_[(size_t)feed].get(), &cur, &has) != 0) fail("open");
                auto &lags = lags_[(size_t)feed];
                lags.erase(lags.begin(), has ? lags.lower_bound(cur.first) : lags.end());
            }
        }
        return out;
    }

    void pop(int feed, std::vector<LiveSegment> &out)
    {
        hpfw_segment seg[8];
        for (int64_t n = 8; n == 8;) {
            if (hpfw_gpu_timeline_tracker_pop(trackers_[(size_t)feed].get(), seg, 8, &n) != 0) fail("pop");
            for (int64_t i = 0; i < n; ++i) out.push_back({feed, named(seg[i], feed)});
        }
    }

    struct Destroy {
        void operator()(hpfw_gpu_streams *s) const { hpfw_gpu_streams_destroy(s); }
        void operator()(hpfw_timeline_tracker *t) const { hpfw_gpu_timeline_tracker_destroy(t); }
    };
    const Storage &storage_;
    LiveStreamsOptions opt_;
    std::unique_ptr<hpfw_gpu_streams, Destroy> s_;
    std::vector<std::unique_ptr<hpfw_timeline_tracker, Destroy>> trackers_;
    hpfw_streams_info info_{};
    hpfw_timeline_params tp_{};
    hpfw_geometry g_{};
    std::vector<std::map<int64_t, int32_t>> lags_; // min_overlap: per feed, window -> lag
    detail::WithinSets within_;                    // opt.within: the feeds' sets
    double col_s_ = 0;
    std::vector<int16_t> pcm_;
    std::vector<LiveWindow> windows_;
};

} // namespace hpfw
