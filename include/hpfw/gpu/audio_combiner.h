// audio_combiner.h -- hpfw::GpuAudioCombiner: the MI355X counterpart of hpfw::AudioCombiner<>
// (reference include/hpfw/audioproblems/combiner/combiner.h:15-132).  Header-only over the C-ABI (hpfw_gpu.h):
// the Mel front end and the uint16 hashprints of HashPrint<uint16_t, MelSpectrogram<>, 32, 50> run on the GPU, the
// index is the exact-hash inverted index in HBM and find() / align() vote on offsets there.
//
// Recordings are numbered in the order they are given (the reference's order comes from parallel threads and is not
// deterministic).  The reference keys its votes by file name; here names must be distinct (build() throws).
// The cereal save / load of the reference (:36-57) is not provided: it archives an Algo type the reference lacks.
//
// Beyond the reference: set_keep_audio(true) makes prepare() keep every file's PCM and the frames its hashprint columns
// came from, and refine() turns the column offsets of align() (441 samples each) into offsets in samples by the exact
// cross-correlation of the PCM (hpfw_gpu_xcorr_pcm16_host) -- the rule of hpfw_amd.combiner.AudioCombiner.refine.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <iostream>
#include <map>
#include <stdexcept>
#include <string>
#include <tuple>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../hpfw_gpu.h"

namespace hpfw {

class GpuAudioCombiner {
public:
    struct SearchResult { // combiner.h:76-81; filename "" when no event matched
        std::string filename;
        size_t cnt;
        size_t confidence;
        long long offset;
    };
    struct AlignHit { // the recording's most votes on one offset, at the smallest such offset
        std::string filename;
        uint32_t peak;
        long long offset;
    };
    struct RefinedHit { // query[n + offset_samples] ~ recording[n]; score = r / (|a| |b|) of the segment at the peak
        std::string filename;
        long long offset_samples;
        bool inverted;
        double score;
        uint32_t peak; // the votes of the hit that was refined
    };
    using Hashprint = std::vector<uint16_t>;
    using FilenameFingerprintPair = std::pair<std::string, Hashprint>;

    explicit GpuAudioCombiner(int device = 0)
    {
        if (hpfw_gpu_create(device, &h_) != 0) throw std::runtime_error(std::string("hpfw::GpuAudioCombiner: ") + hpfw_gpu_last_error());
    }
    ~GpuAudioCombiner() { hpfw_gpu_destroy(h_); }
    GpuAudioCombiner(const GpuAudioCombiner &) = delete;
    GpuAudioCombiner &operator=(const GpuAudioCombiner &) = delete;

    /// on: prepare() and the searches by file name read WAV files at any rate in [8 000, 192 000] Hz and convert them to
    /// 44.1 kHz on the GPU (hpfw_gpu_resample_pcm16); off (the default): 44.1 kHz files only
    void set_resample(bool on) { resample_ = on; }

    /// on: prepare() keeps every file's mono 44.1 kHz PCM and its kept-frame map on the host, for refine(); off (the
    /// default): nothing is kept
    void set_keep_audio(bool on) { keep_audio_ = on; }

    /// filters: Matrix<float, 16, 33 * 32> column-major (hpfw_gpu_cfg_set_filters)
    void set_filters(const float *filters_colmajor)
    {
        check(hpfw_gpu_cfg_set_filters(h_, &cfg_, filters_colmajor));
        has_filters_ = true;
    }
    void set_filters(const std::vector<float> &filters_colmajor)
    {
        if (filters_colmajor.size() != (size_t)cfg_.bits * cfg_.rows * cfg_.context)
            throw std::invalid_argument("hpfw::GpuAudioCombiner: filters must hold 16 x 1056 floats");
        set_filters(filters_colmajor.data());
    }

    /// Algo::prepare: hashprints of every file in the order given; the filters are learned from the files first
    /// when none are set
    std::vector<FilenameFingerprintPair> prepare(const std::vector<std::string> &filenames)
    {
        std::vector<std::vector<int16_t>> pcm;
        for (const auto &f : filenames) pcm.push_back(read_wav(f));
        if (!has_filters_) {
            check(hpfw_gpu_cfg_cov_reset(h_, &cfg_));
            for (const auto &x : pcm) // an empty file adds nothing (and gets no hashprints)
                if (!x.empty()) check(hpfw_gpu_mel_cov_accumulate_pcm16_host(h_, x.data(), (int64_t)x.size(), 1));
            check(hpfw_gpu_cfg_learn_filters(h_, &cfg_, nullptr));
            has_filters_ = true;
        }
        std::vector<FilenameFingerprintPair> out;
        for (size_t i = 0; i < pcm.size(); ++i) out.emplace_back(filenames[i], hashprints(pcm[i]));
        if (keep_audio_)
            for (size_t i = 0; i < pcm.size(); ++i) {
                Audio &a = audio_[filenames[i]];
                a.frames = kept_frames(pcm[i]);
                a.pcm = std::move(pcm[i]);
            }
        return out;
    }

    /// build_db (combiner.h:90-97)
    void build(const std::vector<FilenameFingerprintPair> &pairs)
    {
        std::unordered_map<std::string, uint32_t> ids;
        std::vector<uint16_t> all;
        std::vector<int64_t> off{0};
        for (const auto &[name, hp] : pairs) {
            if (!ids.emplace(name, (uint32_t)ids.size()).second)
                throw std::invalid_argument("hpfw::GpuAudioCombiner: duplicate recording name " + name);
            all.insert(all.end(), hp.begin(), hp.end());
            off.push_back((int64_t)all.size());
        }
        check(hpfw_gpu_combiner_clear(h_));
        if (!pairs.empty()) check(hpfw_gpu_combiner_add(h_, all.empty() ? &dummy_ : all.data(), off.data(), (int64_t)pairs.size()));
        pairs_ = pairs;
        ids_ = std::move(ids);
    }

    size_t size() const { return pairs_.size(); }

    /// find (combiner.h:100-132) for hashprints; exclude: the recording id skipped (the query's own), -1 for none
    SearchResult find(const Hashprint &hp, int exclude = -1) const { return find_many({hp}, {exclude})[0]; }

    /// find for a file, as the reference does: prints "FINDING <file>", skips the recording of that name
    SearchResult find(const std::string &filename)
    {
        std::cout << "FINDING " << filename << std::endl;
        return find(hashprint_of(filename), id_of(filename));
    }

    std::vector<SearchResult> find_many(const std::vector<Hashprint> &hps, const std::vector<int> &exclude) const
    {
        std::vector<uint16_t> all;
        std::vector<int64_t> off{0};
        std::vector<int32_t> ex(exclude.begin(), exclude.end());
        ex.resize(hps.size(), -1);
        for (const auto &hp : hps) {
            all.insert(all.end(), hp.begin(), hp.end());
            off.push_back((int64_t)all.size());
        }
        std::vector<hpfw_combine_result> res(hps.size());
        if (!hps.empty())
            check(hpfw_gpu_combiner_find(h_, all.empty() ? &dummy_ : all.data(), off.data(), ex.data(), (int64_t)hps.size(), res.data()));
        std::vector<SearchResult> out;
        for (const auto &r : res)
            out.push_back({r.rec == 0xffffffffu ? std::string() : pairs_[r.rec].first, (size_t)r.cnt, (size_t)r.confidence,
                           (long long)r.offset});
        return out;
    }

    /// the k recordings with the most votes on one offset, by (peak desc, position in the index); exclude as find
    std::vector<AlignHit> align(const Hashprint &hp, int k, int exclude = -1) const
    {
        const int64_t off[2] = {0, (int64_t)hp.size()};
        const int32_t ex = exclude;
        std::vector<hpfw_align_hit> hits((size_t)k);
        check(hpfw_gpu_combiner_align(h_, hp.empty() ? &dummy_ : hp.data(), off, &ex, 1, k, hits.data()));
        std::vector<AlignHit> out;
        for (const auto &a : hits)
            if (a.rec != 0xffffffffu) out.push_back({pairs_[a.rec].first, a.peak, (long long)a.offset});
        return out;
    }

    /// the hits of align() for the indexed recording `query`, refined to the sample (set_keep_audio(true) before prepare()).
    /// For a hit with column offset d (query column - recording column): o* = the middle column of the column overlap,
    /// c* = o* + d, D0 = 441 (frame_q[c*] - frame_r[o*]); the segment is len = min(seg_len, sample overlap) samples of the
    /// recording centred on sample 441 frame_r[o*], clamped into the overlap; offset_samples = D0 + the lag of the largest
    /// |r| over -radius .. radius.  A hit without overlap keeps 441 d and gets score 0.
    std::vector<RefinedHit> refine(const std::string &query, const std::vector<AlignHit> &hits, int64_t seg_len = (int64_t)1 << 18,
                                   int radius = 1024) const
    {
        if (!keep_audio_) throw std::logic_error("hpfw::GpuAudioCombiner: refine needs set_keep_audio(true)");
        if (seg_len < 1 || seg_len > HPFW_XCORR_MAX_LEN || radius < 0 || radius > HPFW_XCORR_MAX_RADIUS)
            throw std::invalid_argument("hpfw::GpuAudioCombiner: seg_len in 1 .. 2^22 and radius in 0 .. 4096");
        const int qi = id_of(query);
        if (qi < 0) throw std::invalid_argument("hpfw::GpuAudioCombiner: " + query + " is not indexed");
        const Audio &aq = audio_.at(query);
        const int64_t n_q = (int64_t)pairs_[(size_t)qi].second.size(), len_q = (int64_t)aq.pcm.size();
        std::vector<int16_t> packed; // only the two slices a job reads
        std::vector<hpfw_xcorr_job> jobs;
        std::vector<int64_t> d0s;
        std::vector<int> job_of(hits.size(), -1);
        for (size_t i = 0; i < hits.size(); ++i) {
            const Audio &ar = audio_.at(hits[i].filename);
            const int64_t d = hits[i].offset, n_r = (int64_t)pairs_[(size_t)id_of(hits[i].filename)].second.size();
            const int64_t len_r = (int64_t)ar.pcm.size();
            const int64_t o_lo = std::max<int64_t>(0, -d), o_hi = std::min(n_r, n_q - d);
            if (o_lo >= o_hi) continue;
            const int64_t o = floor_half(o_lo + o_hi - 1);
            const int64_t d0 = 441 * ((int64_t)aq.frames[(size_t)(o + d)] - (int64_t)ar.frames[(size_t)o]);
            const int64_t s_lo = std::max<int64_t>(0, -d0), s_hi = std::min(len_r, len_q - d0);
            if (s_lo >= s_hi) continue;
            const int64_t n = std::min(seg_len, s_hi - s_lo);
            const int64_t q = std::min(std::max(441 * (int64_t)ar.frames[(size_t)o] - n / 2, s_lo), s_hi - n), p = q + d0;
            const int64_t a0 = std::max<int64_t>(0, p - radius), a1 = std::max(a0, std::min(len_q, p + radius + n));
            const int64_t at = (int64_t)packed.size();
            packed.insert(packed.end(), aq.pcm.begin() + a0, aq.pcm.begin() + a1);
            packed.insert(packed.end(), ar.pcm.begin() + q, ar.pcm.begin() + q + n);
            job_of[i] = (int)jobs.size();
            jobs.push_back(hpfw_xcorr_job{at, a1 - a0, at + (a1 - a0), n, p - a0, 0, n, radius, 0});
            d0s.push_back(d0);
        }
        std::vector<hpfw_xcorr_peak> peaks(jobs.size());
        if (!jobs.empty())
            check(hpfw_gpu_xcorr_pcm16_host(h_, packed.data(), (int64_t)packed.size(), jobs.data(), (int64_t)jobs.size(), nullptr,
                                            peaks.data()));
        std::vector<RefinedHit> out;
        for (size_t i = 0; i < hits.size(); ++i) {
            if (job_of[i] < 0) {
                out.push_back({hits[i].filename, 441 * hits[i].offset, false, 0.0, hits[i].peak});
                continue;
            }
            const hpfw_xcorr_peak &pk = peaks[(size_t)job_of[i]];
            const double ea = (double)pk.energy_a, eb = (double)pk.energy_b;
            const double score = (ea == 0.0 || eb == 0.0) ? 0.0 : (double)pk.r / (std::sqrt(ea) * std::sqrt(eb));
            out.push_back({hits[i].filename, (long long)(d0s[(size_t)job_of[i]] + pk.lag), pk.r < 0, score, hits[i].peak});
        }
        return out;
    }

    // ---- clock drift between recorders, and the event rendered -------------------------------------
    struct DriftHit { // query[n + offset + drift n] ~ recording[n], drift = drift_ppm 1e-6: the line through the used anchors' lags
        std::string filename;
        int rec;
        double offset, drift_ppm;
        bool inverted;
        double score; // the median |score| of the used anchors
        int anchors, used;
        double rms;
    };
    struct WarpedComponent { // sample n of members[k] sits at starts[k] + rates[k] n on the clock of members[0]
        struct Residual {
            int i, j;
            double samples, ppm;
        };
        std::vector<int> members;
        std::vector<double> starts, rates;
        std::vector<bool> inverted;
        std::vector<Residual> residuals;
    };
    struct DriftEdge { // sample n of j sits at offset + (1 + drift) n of i
        int i, j;
        double offset, drift, score;
        bool inverted;
    };

    /// hpfw_amd.combiner.place_affine: the forest of the edges by (|score| desc, i, j), the affine maps composed in float64
    /// along it from each component's lowest id; lengths (optional): the recordings' lengths, for the centre of an unused
    /// edge's overlap
    static std::vector<WarpedComponent> place_affine(int n_rec, std::vector<DriftEdge> es, const std::vector<int64_t> &lengths = {})
    {
        for (const DriftEdge &e : es)
            if (e.i < 0 || e.i >= n_rec || e.j < 0 || e.j >= n_rec || e.i == e.j || e.score != e.score || e.offset != e.offset ||
                !(std::fabs(e.drift) < 0.5))
                throw std::invalid_argument("hpfw::GpuAudioCombiner: bad edge");
        std::stable_sort(es.begin(), es.end(), [](const DriftEdge &a, const DriftEdge &b) {
            return std::make_tuple(-std::fabs(a.score), a.i, a.j, a.offset, a.drift, a.inverted, a.score) <
                   std::make_tuple(-std::fabs(b.score), b.i, b.j, b.offset, b.drift, b.inverted, b.score);
        });
        std::vector<int> parent((size_t)n_rec), comp((size_t)n_rec, -1);
        for (int i = 0; i < n_rec; ++i) parent[(size_t)i] = i;
        auto root = [&](int x) {
            while (parent[(size_t)x] != x) x = parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
            return x;
        };
        struct Arc {
            int to;
            double off, dr;
            bool inv, forward;
        };
        std::vector<std::vector<Arc>> adj((size_t)n_rec);
        std::vector<DriftEdge> rest;
        for (const DriftEdge &e : es) {
            const int a = root(e.i), b = root(e.j);
            if (a == b) {
                rest.push_back(e);
                continue;
            }
            parent[(size_t)std::max(a, b)] = std::min(a, b);
            adj[(size_t)e.i].push_back({e.j, e.offset, e.drift, e.inverted, true});
            adj[(size_t)e.j].push_back({e.i, e.offset, e.drift, e.inverted, false});
        }
        std::vector<double> start((size_t)n_rec, 0.0), rate((size_t)n_rec, 1.0);
        std::vector<char> pol((size_t)n_rec, 0);
        std::vector<WarpedComponent> out;
        for (int first = 0; first < n_rec; ++first) {
            if (comp[(size_t)first] >= 0) continue;
            comp[(size_t)first] = (int)out.size();
            std::vector<int> members{first}, todo{first};
            while (!todo.empty()) {
                const int x = todo.back();
                todo.pop_back();
                for (const Arc &a : adj[(size_t)x]) {
                    const size_t y = (size_t)a.to;
                    if (comp[y] >= 0) continue;
                    if (a.forward) { // y's sample n is x's sample off + (1 + dr) n
                        start[y] = start[(size_t)x] + rate[(size_t)x] * a.off;
                        rate[y] = rate[(size_t)x] * (1.0 + a.dr);
                    } else { // x's sample n is y's sample off + (1 + dr) n
                        rate[y] = rate[(size_t)x] / (1.0 + a.dr);
                        start[y] = start[(size_t)x] - rate[y] * a.off;
                    }
                    comp[y] = (int)out.size();
                    pol[y] = (char)(pol[(size_t)x] != (char)a.inv);
                    members.push_back(a.to);
                    todo.push_back(a.to);
                }
            }
            std::sort(members.begin(), members.end());
            double base = start[(size_t)members[0]];
            for (int m : members) base = std::min(base, start[(size_t)m]);
            WarpedComponent c;
            for (int m : members) {
                start[(size_t)m] -= base;
                c.members.push_back(m);
                c.starts.push_back(start[(size_t)m]);
                c.rates.push_back(rate[(size_t)m]);
                c.inverted.push_back(pol[(size_t)m] != 0);
            }
            out.push_back(std::move(c));
        }
        for (const DriftEdge &e : rest) {
            const size_t i = (size_t)e.i, j = (size_t)e.j;
            const double p_off = (start[j] - start[i]) / rate[i], p_rate = rate[j] / rate[i];
            double at = 0.0;
            if (!lengths.empty()) { // the centre of the overlap, in j's samples
                const double lo = std::max(0.0, -e.offset / (1.0 + e.drift));
                const double hi = std::min((double)lengths[j], ((double)lengths[i] - e.offset) / (1.0 + e.drift));
                at = hi > lo ? (lo + hi) / 2.0 : 0.0;
            }
            out[(size_t)comp[i]].residuals.push_back(
                {e.i, e.j, (e.offset - p_off) + ((1.0 + e.drift) - p_rate) * at, ((1.0 + e.drift) - p_rate) * 1e6});
        }
        return out;
    }

    /// the hits of align() for the indexed recording `query` as lines: short anchors of anchor_len samples every anchor_hop
    /// outward from refine()'s segment, each correlated around what the anchors before it predict, then once more with the
    /// query read on the recording's clock by the first line (hpfw_gpu_warp_pcm16_host), and the Theil-Sen line
    /// (hpfw_gpu_drift_fit) through the lags of those with |score| >= min_score -- the rule of
    /// hpfw_amd.combiner.AudioCombiner.refine_drift
    std::vector<DriftHit> refine_drift(const std::string &query, const std::vector<AlignHit> &hits, double min_score,
                                       int64_t anchor_len = (int64_t)1 << 16, int64_t anchor_hop = (int64_t)1 << 21, int radius = 1024) const
    {
        const int qi = id_of(query);
        if (qi < 0) throw std::invalid_argument("hpfw::GpuAudioCombiner: " + query + " is not indexed");
        std::vector<std::pair<int, AlignHit>> pairs;
        for (const AlignHit &h : hits) pairs.emplace_back(qi, h);
        return drift_pairs(pairs, min_score, anchor_len, anchor_hop, radius);
    }

    /// align all against all (k best each), per unordered pair the hit with the larger peak (ties: the smaller query id),
    /// those with peak >= min_peak through refine_drift, those with a used anchor placed by place_affine
    std::vector<WarpedComponent> layout_drift(uint32_t min_peak, double min_score, int k = 8, int64_t anchor_len = (int64_t)1 << 16,
                                              int64_t anchor_hop = (int64_t)1 << 21, int radius = 1024) const
    {
        std::map<std::pair<int, int>, std::pair<int, AlignHit>> best;
        for (int qi = 0; qi < (int)pairs_.size(); ++qi)
            for (const AlignHit &h : align(pairs_[(size_t)qi].second, k, qi)) {
                const int rec = id_of(h.filename);
                const std::pair<int, int> key{std::min(qi, rec), std::max(qi, rec)};
                auto it = best.find(key);
                if (it == best.end()) best.emplace(key, std::make_pair(qi, h));
                else if (h.peak > it->second.second.peak) it->second = std::make_pair(qi, h);
            }
        std::vector<std::pair<int, AlignHit>> pairs;
        for (const auto &kv : best)
            if (kv.second.second.peak >= min_peak) pairs.push_back(kv.second);
        const std::vector<DriftHit> hits = drift_pairs(pairs, min_score, anchor_len, anchor_hop, radius);
        std::vector<DriftEdge> edges;
        for (size_t i = 0; i < pairs.size(); ++i)
            if (hits[i].used) edges.push_back({pairs[i].first, hits[i].rec, hits[i].offset, hits[i].drift_ppm * 1e-6, hits[i].score, hits[i].inverted});
        std::vector<int64_t> lengths;
        for (const auto &p : pairs_) lengths.push_back((int64_t)audio_.at(p.first).pcm.size());
        return place_affine((int)pairs_.size(), edges, lengths);
    }

    /// the event of a component as audio on its clock: int16 [n_out], the mix (hpfw_gpu_mix_pcm16_host), or with `tracks`
    /// [n_members][n_out], every member alone (hpfw_gpu_warp_pcm16_host), `chunk` outputs at a time.  gains: signed Q15 per
    /// member (empty: round(2^15 / n_members), negative for inverted members)
    std::vector<int16_t> render(const WarpedComponent &c, std::vector<int32_t> gains = {}, bool tracks = false, int64_t chunk = (int64_t)1 << 24) const
    {
        if (!keep_audio_) throw std::logic_error("hpfw::GpuAudioCombiner: render needs set_keep_audio(true)");
        const size_t n = c.members.size();
        if (gains.empty()) {
            const int32_t g = (int32_t)std::nearbyint(32768.0 / (double)std::max<size_t>(n, 1));
            for (size_t k = 0; k < n; ++k) gains.push_back(c.inverted[k] ? -g : g);
        }
        if (gains.size() != n || chunk < 1) throw std::invalid_argument("hpfw::GpuAudioCombiner: render takes one gain per member and chunk >= 1");
        std::vector<int16_t> pcm;
        std::vector<hpfw_warp_track> tr(n);
        int64_t n_out = 0;
        for (size_t k = 0; k < n; ++k) {
            const std::vector<int16_t> &x = audio_.at(pairs_[(size_t)c.members[k]].first).pcm;
            hpfw_warp_track &t = tr[k];
            t = hpfw_warp_track{(int64_t)pcm.size(), (int64_t)x.size(), 0, 0, 0, gains[k], 0};
            check(hpfw_gpu_time_map_q40(c.starts[k], c.rates[k] - 1.0, &t.i0, &t.f0, &t.d));
            n_out = std::max(n_out, (int64_t)std::ceil(c.starts[k] + c.rates[k] * (double)x.size()));
            pcm.insert(pcm.end(), x.begin(), x.end());
        }
        const int64_t rows = tracks ? (int64_t)n : 1;
        std::vector<int16_t> out((size_t)(rows * n_out)), piece;
        for (int64_t m0 = 0; m0 < n_out; m0 += chunk) {
            const int64_t len = std::min(chunk, n_out - m0);
            piece.assign((size_t)(rows * len), 0);
            if (tracks)
                check(hpfw_gpu_warp_pcm16_host(h_, pcm.data(), (int64_t)pcm.size(), tr.data(), (int64_t)n, m0, len, piece.data()));
            else
                check(hpfw_gpu_mix_pcm16_host(h_, pcm.data(), (int64_t)pcm.size(), tr.data(), (int64_t)n, m0, len, piece.data()));
            for (int64_t r = 0; r < rows; ++r) std::copy(piece.begin() + r * len, piece.begin() + (r + 1) * len, out.begin() + r * n_out + m0);
        }
        return out;
    }

    /// samples of a recording kept by prepare() under set_keep_audio(true)
    int64_t samples_of(const std::string &filename) const { return (int64_t)audio_.at(filename).pcm.size(); }

    /// the hashprints of an indexed recording (empty when the name is not indexed)
    Hashprint hashprints_of(const std::string &filename) const
    {
        const int id = id_of(filename);
        return id >= 0 ? pairs_[(size_t)id].second : Hashprint();
    }

    /// combine (combiner.h:23-33): index the files unless an index exists, then find every file without itself;
    /// prints what the reference prints
    std::vector<SearchResult> combine(const std::vector<std::string> &filenames)
    {
        if (pairs_.empty()) build(prepare(filenames));
        std::vector<Hashprint> hps;
        std::vector<int> ex;
        for (const auto &f : filenames) {
            hps.push_back(hashprint_of(f));
            ex.push_back(id_of(f));
        }
        auto res = find_many(hps, ex);
        for (size_t i = 0; i < filenames.size(); ++i)
            std::cout << "FINDING " << filenames[i] << std::endl
                      << res[i].filename << " " << res[i].cnt << " " << res[i].confidence << " " << res[i].offset << std::endl
                      << std::endl;
        return res;
    }

private:
    hpfw_gpu *h_ = nullptr;
    hpfw_handle_config cfg_ = HPFW_CONFIG_COMBINER;
    bool has_filters_ = false;
    bool resample_ = false;
    bool keep_audio_ = false;
    struct Audio {
        std::vector<int16_t> pcm;
        std::vector<int32_t> frames; // the frame of every kept Mel column (hpfw_gpu_mel_kept_frames_pcm16_host)
    };
    std::unordered_map<std::string, Audio> audio_;
    std::vector<FilenameFingerprintPair> pairs_;
    std::unordered_map<std::string, uint32_t> ids_;
    static inline uint16_t dummy_ = 0;

    static void check(int rc)
    {
        if (rc != 0) throw std::runtime_error(std::string("hpfw::GpuAudioCombiner: ") + hpfw_gpu_last_error());
    }

    std::vector<int16_t> read_wav(const std::string &path)
    {
        int64_t n = 0;
        if (!resample_) {
            check(hpfw_gpu_wav_read_pcm16(path.c_str(), nullptr, 0, &n));
            std::vector<int16_t> pcm((size_t)n);
            check(hpfw_gpu_wav_read_pcm16(path.c_str(), pcm.data(), n, &n));
            return pcm;
        }
        int32_t rate = 0;
        check(hpfw_gpu_wav_read_pcm16_any(path.c_str(), nullptr, 0, &n, &rate));
        std::vector<int16_t> pcm((size_t)n);
        check(hpfw_gpu_wav_read_pcm16_any(path.c_str(), pcm.data(), n, &n, &rate));
        if (rate == 44100 || pcm.empty()) return pcm;
        int64_t n_out = 0;
        check(hpfw_gpu_resample_length(n, rate, &n_out));
        std::vector<int16_t> out((size_t)n_out);
        check(hpfw_gpu_resample_pcm16_host(h_, pcm.data(), n, 1, rate, out.data()));
        return out;
    }

    Hashprint hashprints(const std::vector<int16_t> &pcm)
    {
        if (pcm.empty()) return {};
        const int64_t stride = std::max<int64_t>(hpfw_gpu_mel_frames((int64_t)pcm.size()) - 81, 1);
        Hashprint hp((size_t)stride);
        int32_t n = 0;
        check(hpfw_gpu_mel_hashprints_pcm16_host(h_, pcm.data(), (int64_t)pcm.size(), 1, hp.data(), stride, &n));
        hp.resize((size_t)n);
        return hp;
    }

    static int64_t floor_half(int64_t x) { return x >= 0 ? x / 2 : -((-x + 1) / 2); }

    static double xcorr_score(const hpfw_xcorr_peak &pk)
    {
        const double ea = (double)pk.energy_a, eb = (double)pk.energy_b;
        return (ea == 0.0 || eb == 0.0) ? 0.0 : (double)pk.r / (std::sqrt(ea) * std::sqrt(eb));
    }

    struct AnchorPoint { // an anchor correlated: its centre sample, the lag found, the score there
        int64_t pos, lag;
        double score;
        bool used;
    };
    struct Chain { // a pair's anchors and what the two passes found
        const Audio *q = nullptr, *r = nullptr;
        int64_t d0 = 0, len = 0;
        std::vector<int64_t> centre, left, right; // the anchors' first samples, going outward
        std::vector<AnchorPoint> points, first;
        std::vector<AnchorPoint> trail[2];        // the used anchors of a side going outward, the centre included
        bool live = false, has_line = false;
        double a = 0.0, b = 0.0;
    };

    // the lag expected at sample pos: on the line through the last two used anchors of the side, the last one's lag while
    // there is one, the hit's own while there is none
    static int64_t predict(const std::vector<AnchorPoint> &trail, int64_t fallback, int64_t pos)
    {
        if (trail.empty()) return fallback;
        if (trail.size() == 1) return trail.back().lag;
        const AnchorPoint &p1 = trail[trail.size() - 2], &p2 = trail.back();
        return p2.lag + (int64_t)std::nearbyint((double)((p2.lag - p1.lag) * (pos - p2.pos)) / (double)(p2.pos - p1.pos));
    }

    void fit(const std::vector<AnchorPoint> &pts, double *a, double *b, double *rms) const
    {
        std::vector<int64_t> n, lag;
        for (const AnchorPoint &p : pts) {
            n.push_back(p.pos);
            lag.push_back(p.lag);
        }
        check(hpfw_gpu_drift_fit(n.data(), lag.data(), (int)n.size(), a, b, rms));
    }

    // hpfw_amd.combiner.AudioCombiner._drift_pairs, step for step
    std::vector<DriftHit> drift_pairs(const std::vector<std::pair<int, AlignHit>> &pairs, double min_score, int64_t anchor_len,
                                      int64_t anchor_hop, int radius) const
    {
        if (!keep_audio_) throw std::logic_error("hpfw::GpuAudioCombiner: refine_drift needs set_keep_audio(true)");
        if (anchor_len < 1 || anchor_len > HPFW_XCORR_MAX_LEN || radius < 0 || radius > HPFW_XCORR_MAX_RADIUS || anchor_hop < 1)
            throw std::invalid_argument("hpfw::GpuAudioCombiner: anchor_len in 1 .. 2^22, anchor_hop >= 1 and radius in 0 .. 4096");
        std::vector<Chain> chains(pairs.size());
        size_t rounds = 0;
        bool any = false;
        for (size_t i = 0; i < pairs.size(); ++i) {
            Chain &c = chains[i];
            const int qi = pairs[i].first, ri = id_of(pairs[i].second.filename);
            c.q = &audio_.at(pairs_[(size_t)qi].first);
            c.r = &audio_.at(pairs[i].second.filename);
            const int64_t n_q = (int64_t)pairs_[(size_t)qi].second.size(), n_r = (int64_t)pairs_[(size_t)ri].second.size();
            const int64_t len_q = (int64_t)c.q->pcm.size(), len_r = (int64_t)c.r->pcm.size(), d = pairs[i].second.offset;
            const int64_t o_lo = std::max<int64_t>(0, -d), o_hi = std::min(n_r, n_q - d);
            if (o_lo >= o_hi) continue;
            const int64_t o = floor_half(o_lo + o_hi - 1);
            c.d0 = 441 * ((int64_t)c.q->frames[(size_t)(o + d)] - (int64_t)c.r->frames[(size_t)o]);
            const int64_t s_lo = std::max<int64_t>(0, -c.d0), s_hi = std::min(len_r, len_q - c.d0);
            if (s_lo >= s_hi) continue;
            c.len = std::min(anchor_len, s_hi - s_lo);
            const int64_t q = std::min(std::max(441 * (int64_t)c.r->frames[(size_t)o] - c.len / 2, s_lo), s_hi - c.len);
            int32_t nl = 0, nr = 0;
            int64_t count = 0;
            check(hpfw_gpu_drift_anchors(s_lo, s_hi, q, c.len, anchor_len, anchor_hop, nullptr, 0, &nl, &nr, &count));
            std::vector<int64_t> starts((size_t)count);
            check(hpfw_gpu_drift_anchors(s_lo, s_hi, q, c.len, anchor_len, anchor_hop, starts.data(), count, &nl, &nr, &count));
            c.centre.assign(starts.begin(), starts.begin() + 1);
            c.left.assign(starts.begin() + 1, starts.begin() + 1 + nl);
            c.right.assign(starts.begin() + 1 + nl, starts.end());
            c.live = true;
            rounds = std::max(rounds, std::max(c.left.size(), c.right.size()));
            any = true;
        }
        struct Todo {
            Chain *c;
            int side; // -1: the centre
            int64_t start, guess;
        };
        auto correlate = [&](const std::vector<int16_t> &packed, const std::vector<hpfw_xcorr_job> &jobs) {
            std::vector<hpfw_xcorr_peak> peaks(jobs.size());
            if (!jobs.empty())
                check(hpfw_gpu_xcorr_pcm16_host(h_, packed.data(), (int64_t)packed.size(), jobs.data(), (int64_t)jobs.size(), nullptr, peaks.data()));
            return peaks;
        };
        for (size_t t = 0; any && t <= rounds; ++t) {
            std::vector<Todo> todo;
            for (Chain &c : chains) {
                if (!c.live) continue;
                if (t == 0) todo.push_back({&c, -1, c.centre[0], 0});
                else
                    for (int side = 0; side < 2; ++side) {
                        const std::vector<int64_t> &s = side ? c.right : c.left;
                        if (t <= s.size()) todo.push_back({&c, side, s[t - 1], 0});
                    }
            }
            std::vector<int16_t> packed;
            std::vector<hpfw_xcorr_job> jobs;
            for (Todo &w : todo) {
                const Chain &c = *w.c;
                const int64_t n = c.len, size = (int64_t)c.q->pcm.size();
                w.guess = w.side < 0 ? c.d0 : predict(c.trail[w.side], c.d0, w.start + n / 2);
                const int64_t p = w.start + w.guess;
                const int64_t a0 = std::min(std::max<int64_t>(0, p - radius), size), a1 = std::max(a0, std::min(size, p + radius + n));
                const int64_t at = (int64_t)packed.size();
                packed.insert(packed.end(), c.q->pcm.begin() + a0, c.q->pcm.begin() + a1);
                packed.insert(packed.end(), c.r->pcm.begin() + w.start, c.r->pcm.begin() + w.start + n);
                jobs.push_back(hpfw_xcorr_job{at, a1 - a0, at + (a1 - a0), n, p - a0, 0, n, radius, 0});
            }
            const std::vector<hpfw_xcorr_peak> peaks = correlate(packed, jobs);
            for (size_t i = 0; i < todo.size(); ++i) {
                Chain &c = *todo[i].c;
                const double score = xcorr_score(peaks[i]);
                const AnchorPoint pt{todo[i].start + c.len / 2, todo[i].guess + peaks[i].lag, score, std::fabs(score) >= min_score};
                c.points.push_back(pt);
                if (!pt.used) continue;
                if (todo[i].side < 0) {
                    c.trail[0].push_back(pt);
                    c.trail[1].push_back(pt);
                } else {
                    c.trail[todo[i].side].push_back(pt);
                }
            }
        }
        // the second pass: every anchor again, the query read on the recording's clock by the first pass's line
        std::vector<int64_t> lens;
        for (Chain &c : chains) {
            if (!c.live) continue;
            std::vector<AnchorPoint> used;
            for (const AnchorPoint &p : c.points)
                if (p.used) used.push_back(p);
            double rms = 0.0;
            c.has_line = !used.empty();
            if (c.has_line) {
                fit(used, &c.a, &c.b, &rms);
                lens.push_back(c.len);
            }
            c.first = std::move(c.points);
            c.points.clear();
        }
        std::sort(lens.begin(), lens.end());
        lens.erase(std::unique(lens.begin(), lens.end()), lens.end());
        for (const int64_t n : lens) {
            std::vector<Todo> batch;
            for (Chain &c : chains) {
                if (!c.live || !c.has_line || c.len != n) continue;
                for (const std::vector<int64_t> *group : {&c.centre, &c.left, &c.right})
                    for (const int64_t start : *group) batch.push_back({&c, 0, start, 0});
            }
            std::vector<int16_t> packed;
            std::vector<hpfw_warp_track> tracks;
            const int64_t n_out = n + 2 * (int64_t)radius;
            for (Todo &w : batch) {
                const Chain &c = *w.c;
                const double b = std::min(std::max(c.b, -0.0009765625), 0.0009765625);
                const int64_t mid = w.start + n / 2, size = (int64_t)c.q->pcm.size();
                w.guess = (int64_t)std::nearbyint(c.a + b * (double)mid);
                // output m stands for the recording's sample start - radius + m: the query at that + lag + b (that - mid)
                const double bend = b * (double)(w.start - radius - mid), whole = std::floor(bend);
                const int64_t pos0 = w.start - radius + w.guess + (int64_t)whole;
                const int64_t f0 = std::min((int64_t)((bend - whole) * 1099511627776.0), ((int64_t)1 << 40) - 1);
                const int64_t reach = (int64_t)(std::fabs(b) * (double)n_out) + 2 + 32;
                const int64_t lo = std::min(std::max<int64_t>(0, pos0 - reach), size), hi = std::min(std::max<int64_t>(0, pos0 + n_out + reach), size);
                tracks.push_back(hpfw_warp_track{(int64_t)packed.size(), hi - lo, pos0 - lo, f0, (int64_t)std::nearbyint(b * 1099511627776.0), 1, 0});
                packed.insert(packed.end(), c.q->pcm.begin() + lo, c.q->pcm.begin() + hi);
            }
            std::vector<int16_t> bent((size_t)((int64_t)batch.size() * n_out));
            check(hpfw_gpu_warp_pcm16_host(h_, packed.data(), (int64_t)packed.size(), tracks.data(), (int64_t)tracks.size(), 0, n_out, bent.data()));
            std::vector<hpfw_xcorr_job> jobs;
            for (size_t k = 0; k < batch.size(); ++k) {
                jobs.push_back(hpfw_xcorr_job{(int64_t)k * n_out, n_out, (int64_t)bent.size() + (int64_t)k * n, n, radius, 0, n, radius, 0});
            }
            for (const Todo &w : batch) bent.insert(bent.end(), w.c->r->pcm.begin() + w.start, w.c->r->pcm.begin() + w.start + n);
            const std::vector<hpfw_xcorr_peak> peaks = correlate(bent, jobs);
            for (size_t k = 0; k < batch.size(); ++k) {
                const double score = xcorr_score(peaks[k]);
                batch[k].c->points.push_back({batch[k].start + n / 2, batch[k].guess + peaks[k].lag, score, std::fabs(score) >= min_score});
            }
        }
        std::vector<DriftHit> out;
        for (size_t i = 0; i < pairs.size(); ++i) {
            const Chain &c = chains[i];
            const AlignHit &hit = pairs[i].second;
            std::vector<AnchorPoint> used;
            for (const AnchorPoint &p : c.points)
                if (p.used) used.push_back(p);
            if (used.empty()) { // nothing to go by: the hit as it is, score 0
                out.push_back({hit.filename, id_of(hit.filename), (double)(441 * hit.offset), 0.0, false, 0.0, (int)c.first.size(), 0, 0.0});
                continue;
            }
            double a = 0.0, b = 0.0, rms = 0.0;
            fit(used, &a, &b, &rms);
            size_t neg = 0;
            std::vector<double> mags;
            for (const AnchorPoint &p : used) {
                neg += p.score < 0;
                mags.push_back(std::fabs(p.score));
            }
            std::sort(mags.begin(), mags.end());
            const double med = mags.size() & 1 ? mags[mags.size() / 2] : (mags[mags.size() / 2 - 1] + mags[mags.size() / 2]) / 2.0;
            const bool inverted = c.points[0].used ? used[0].score < 0 : 2 * neg > used.size();
            out.push_back({hit.filename, id_of(hit.filename), a, b * 1e6, inverted, med, (int)c.points.size(), (int)used.size(), rms});
        }
        return out;
    }

    std::vector<int32_t> kept_frames(const std::vector<int16_t> &pcm)
    {
        if (pcm.empty()) return {};
        const int64_t stride = std::max<int64_t>(hpfw_gpu_mel_frames((int64_t)pcm.size()), 1);
        std::vector<int32_t> frames((size_t)stride);
        int32_t n = 0;
        check(hpfw_gpu_mel_kept_frames_pcm16_host(h_, pcm.data(), (int64_t)pcm.size(), 1, frames.data(), stride, &n));
        frames.resize((size_t)n);
        return frames;
    }

    int id_of(const std::string &name) const
    {
        auto it = ids_.find(name);
        return it == ids_.end() ? -1 : (int)it->second;
    }

    Hashprint hashprint_of(const std::string &filename)
    {
        const int id = id_of(filename);
        return id >= 0 ? pairs_[(size_t)id].second : hashprints(read_wav(filename));
    }
};

} // namespace hpfw
