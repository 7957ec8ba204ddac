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
#include <stdexcept>
#include <string>
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
