// gpu_storage.h -- hpfw::db::GpuStorage<Collector>: the MI355X counterpart of
// hpfw::db::MemoryStorage<Collector> (reference include/hpfw/audioproblems/live-song-id/storage.h:8-92):
// build() keeps the hashprints in HBM, find() runs the exhaustive sliding Hamming scan on the GPU and
// returns SearchResult{filename, cnt, offset} of the first strict minimum in database order.
// find_topk() adds the notebook's "10 best tracks" (examples/python/liveid.ipynb cell 9), ordered by
// (distance, position in the database).
#pragma once

#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <limits>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../hpfw_gpu.h"

namespace hpfw::db {

template <typename Collector>
class GpuStorage {
public:
    struct SearchResult { // storage.h:11-15
        std::string filename;
        size_t cnt;
        int64_t offset;
    };

    /// the device: HPFW_GPU_DEVICE (the collector reads the same variable), default 0; ShardedGpuStorage
    /// (sharded_storage.h) is the storage over several devices
    GpuStorage() : GpuStorage(env_device()) {}
    explicit GpuStorage(int device)
    {
        if (hpfw_gpu_create(device, &h_) != 0) throw std::runtime_error(std::string("hpfw::db::GpuStorage: ") + hpfw_gpu_last_error());
    }
    ~GpuStorage() { hpfw_gpu_destroy(h_); }
    GpuStorage(const GpuStorage &) = delete;
    GpuStorage &operator=(const GpuStorage &) = delete;

    /// storage.h:21-25; accepts any range of Collector::FilenameFingerprintPair (vector, tbb::concurrent_vector)
    template <typename Range>
    void build(Range &&hashprints)
    {
        names_.clear();
        std::vector<uint64_t> all;
        std::vector<int64_t> off{0};
        for (auto &p : hashprints) {
            names_.push_back(p.filename);
            all.insert(all.end(), p.fingerprint.begin(), p.fingerprint.end());
            off.push_back((int64_t)all.size());
        }
        check(hpfw_gpu_index_clear(h_));
        if (!names_.empty()) check(hpfw_gpu_index_add(h_, all.empty() ? &dummy_ : all.data(), off.data(), (int64_t)names_.size()));
        removed_.assign(names_.size(), 0); // a fresh index forgets all removals
        added_len_.clear();
        for (size_t i = 0; i + 1 < off.size(); ++i) added_len_.push_back(off[i + 1] - off[i]);
    }

    /// index maintenance (hpfw_gpu_index_remove): the recordings named leave the index in place.  Slots
    /// are ids: names() and size() keep counting them, live() counts the recordings that remain, and no search names a removed
    /// one.  Every live slot carrying one of the names goes; returns the number removed.  A name that is unknown (or already
    /// removed) throws std::out_of_range before anything changes.
    auto remove(const std::vector<std::string> &names) -> size_t
    {
        std::vector<int64_t> ids;
        for (const std::string &name : names) {
            bool found = false;
            for (size_t i = 0; i < names_.size(); ++i)
                if (!removed_[i] && names_[i] == name) {
                    ids.push_back((int64_t)i);
                    found = true;
                }
            if (!found) throw std::out_of_range("hpfw::db::GpuStorage: no recording " + name);
        }
        if (ids.empty()) return 0;
        check(hpfw_gpu_index_remove(h_, ids.data(), (int64_t)ids.size(), nullptr));
        size_t n = 0;
        for (int64_t i : ids) { // (a name may repeat in the list)
            n += !removed_[(size_t)i];
            removed_[(size_t)i] = 1;
        }
        return n;
    }

    /// appends a range of Collector::FilenameFingerprintPair behind the index (hpfw_gpu_index_add): the new recordings take
    /// the slots size(), size() + 1, ... and use the room removals freed before anything is allocated
    template <typename Range>
    void add(Range &&hashprints)
    {
        std::vector<std::string> names;
        std::vector<uint64_t> all;
        std::vector<int64_t> off{0};
        for (auto &p : hashprints) {
            names.push_back(p.filename);
            all.insert(all.end(), p.fingerprint.begin(), p.fingerprint.end());
            off.push_back((int64_t)all.size());
        }
        if (names.empty()) return;
        check(hpfw_gpu_index_add(h_, all.empty() ? &dummy_ : all.data(), off.data(), (int64_t)names.size()));
        names_.insert(names_.end(), names.begin(), names.end());
        removed_.resize(names_.size(), 0);
        for (size_t i = 0; i + 1 < off.size(); ++i) added_len_.push_back(off[i + 1] - off[i]);
    }

    /// the hashprints slot `clip` had when its recording was added, removed since or not (hpfw::LiveStreams trims a segment
    /// by it)
    int64_t added_length(size_t clip) const { return added_len_.at(clip); }

    /// the recordings that remain (size() counts slots)
    size_t live() const
    {
        size_t n = 0;
        for (char r : removed_) n += !r;
        return n;
    }

    /// storage.h:27-64
    auto find(const typename Collector::Hashprint &hp) const -> SearchResult
    {
        auto top = find_topk(hp, 1);
        if (top.empty()) return {"", std::numeric_limits<size_t>::max(), 0}; // storage.h:28
        return top[0];
    }

    auto find_topk(const typename Collector::Hashprint &hp, int k) const -> std::vector<SearchResult>
    {
        std::vector<SearchResult> out;
        if (hp.empty() || names_.empty()) return out;
        const int64_t q_off[2] = {0, (int64_t)hp.size()};
        std::vector<hpfw_hit> hits((size_t)k);
        check(hpfw_gpu_search_topk(h_, hp.data(), q_off, 1, k, hits.data()));
        for (const hpfw_hit &hit : hits) {
            if (hit.clip == 0xffffffffu) break;
            out.push_back({names_[hit.clip], (size_t)hit.dist, (int64_t)hit.offset});
        }
        return out;
    }

    /// find_topk() within a subset of the index (hpfw_gpu_search_topk_within): `clips` are positions in
    /// the database in strictly ascending order, and the answer is the one a storage built from just those recordings gives.
    /// The scan covers the listed recordings only.
    auto find_within(const typename Collector::Hashprint &hp, int k, const std::vector<int32_t> &clips) const -> std::vector<SearchResult>
    {
        std::vector<SearchResult> out;
        for (const ScoredResult &r : within(hp, k, clips, false)) out.push_back({r.filename, r.cnt, r.offset});
        return out;
    }

    /// find_within() with scores: per hit how far its distance stands out from the best distances of the other counted
    /// recordings of the SET (hpfw_gpu_hit_score; NaN below three counted recordings, as an index of two gives)
    struct ScoredResult {
        std::string filename;
        size_t cnt;
        int64_t offset;
        double score;
    };
    auto find_within_scored(const typename Collector::Hashprint &hp, int k, const std::vector<int32_t> &clips) const -> std::vector<ScoredResult>
    {
        return within(hp, k, clips, true);
    }

    /// a query played in another key: per_shift[i] holds the query's hashprints under shift i
    /// (hpfw::transposed_hashprints, include/hpfw/gpu/transposed.h); per clip the smallest distance over the shifts, ties
    /// to the first shift; the k best clips by (distance, position in the database) with the index of their shift
    struct ShiftResult {
        std::string filename;
        size_t cnt;
        int64_t offset;
        int shift_index;
    };
    auto find_topk_transposed(const std::vector<typename Collector::Hashprint> &per_shift, int k) const -> std::vector<ShiftResult>
    {
        std::vector<ShiftResult> out;
        if (per_shift.empty() || names_.empty()) return out;
        std::vector<uint64_t> all;
        std::vector<int64_t> off{0};
        for (const auto &hp : per_shift) {
            all.insert(all.end(), hp.begin(), hp.end());
            off.push_back((int64_t)all.size());
        }
        std::vector<hpfw_shift_hit> hits((size_t)k);
        check(hpfw_gpu_search_topk_transposed(h_, all.empty() ? &dummy_ : all.data(), off.data(), 1, (int)per_shift.size(), k, hits.data()));
        for (const hpfw_shift_hit &hit : hits) {
            if (hit.clip == 0xffffffffu) break;
            out.push_back({names_[hit.clip], (size_t)hit.dist, (int64_t)hit.offset, (int)hit.shift_index});
        }
        return out;
    }

    /// the overlap search (hpfw_gpu_search_overlap): the query may overhang either end of a clip, and
    /// clips are ordered by mismatching bits per overlapping hashprint over at least min_overlap hashprints (the caller's:
    /// there is no default), then the larger overlap, then the position in the database.  Query position 0 lies on clip
    /// position lag (negative: the query begins before the clip does).
    struct OverlapResult {
        std::string filename;
        size_t cnt;     // mismatching bits over the overlap
        int64_t lag;
        size_t overlap; // hashprints compared
    };
    auto find_overlap(const typename Collector::Hashprint &hp, int k, int min_overlap) const -> std::vector<OverlapResult>
    {
        std::vector<OverlapResult> out;
        if (hp.empty() || names_.empty()) return out;
        const int64_t q_off[2] = {0, (int64_t)hp.size()};
        std::vector<hpfw_overlap_hit> hits((size_t)k);
        check(hpfw_gpu_search_overlap(h_, hp.data(), q_off, 1, nullptr, min_overlap, k, hits.data()));
        for (const hpfw_overlap_hit &hit : hits) {
            if (hit.clip == 0xffffffffu) break;
            out.push_back({names_[hit.clip], (size_t)hit.dist, (int64_t)hit.lag, (size_t)hit.overlap});
        }
        return out;
    }

    /// the catalogue self-join (hpfw_gpu_index_selfjoin): the pairs of indexed recordings a before b
    /// whose best alignment by the overlap rule, over at least min_overlap hashprints, has dist * rate_den <= rate_num *
    /// overlap, in database order of (a, b).  min_overlap and the threshold rate_num / rate_den (mismatching bits per
    /// hashprint) are the caller's: there is no default.  Position 0 of a lies on position lag of b.
    struct DuplicateResult {
        std::string name_a, name_b;
        size_t dist;    // mismatching bits over the overlap
        size_t overlap; // hashprints compared
        int64_t lag;
    };
    auto duplicates(int min_overlap, int rate_num, int rate_den) const -> std::vector<DuplicateResult>
    {
        std::vector<hpfw_dup_pair> pairs(256);
        int64_t count = 0;
        check(hpfw_gpu_index_selfjoin(h_, min_overlap, rate_num, rate_den, pairs.data(), (int64_t)pairs.size(), &count));
        if (count > (int64_t)pairs.size()) { // (the buffer was too small: once more with room for all)
            pairs.resize((size_t)count);
            check(hpfw_gpu_index_selfjoin(h_, min_overlap, rate_num, rate_den, pairs.data(), (int64_t)pairs.size(), &count));
        }
        std::vector<DuplicateResult> out;
        for (int64_t i = 0; i < count; ++i) {
            const hpfw_dup_pair &p = pairs[(size_t)i];
            out.push_back({names_[p.a], names_[p.b], (size_t)p.dist, (size_t)p.overlap, (int64_t)p.lag});
        }
        return out;
    }

    /// the local self-join (hpfw_gpu_index_localjoin): the pairs of indexed recordings a before b that
    /// share a passage -- the best run of consecutive hashprints on any diagonal of the two scores at least min_score, at
    /// max_rate - (mismatching bits) a hashprint.  max_rate, 1..31, and min_score >= 1 are the caller's: there is no default.
    /// Hashprints a_start .. a_start + length - 1 of a lie on columns lag + a_start onwards of b; score = max_rate * length - cnt.
    struct PassageResult {
        std::string name_a, name_b;
        int64_t score;  // max_rate * length - cnt
        int64_t lag;    // column of b that hashprint 0 of a lies on (negative: before b begins)
        size_t a_start; // first hashprint of the passage in a
        size_t length;  // hashprints of the passage
        size_t cnt;     // mismatching bits over the passage
    };
    auto shared_passages(int max_rate, int min_score) const -> std::vector<PassageResult>
    {
        std::vector<hpfw_passage_pair> pairs(256);
        int64_t count = 0;
        check(hpfw_gpu_index_localjoin(h_, max_rate, min_score, pairs.data(), (int64_t)pairs.size(), &count));
        if (count > (int64_t)pairs.size()) { // (the buffer was too small: once more with room for all)
            pairs.resize((size_t)count);
            check(hpfw_gpu_index_localjoin(h_, max_rate, min_score, pairs.data(), (int64_t)pairs.size(), &count));
        }
        std::vector<PassageResult> out;
        for (int64_t i = 0; i < count; ++i) {
            const hpfw_passage_pair &p = pairs[(size_t)i];
            out.push_back({names_[p.a], names_[p.b], (int64_t)p.score, (int64_t)p.lag, (size_t)p.a_start, (size_t)p.length, (size_t)p.dist});
        }
        return out;
    }

    /// the ingest check (hpfw_gpu_index_join): what duplicates() would report in addition after
    /// add(hashprints), without the index changing -- the pairs whose b is one of the recordings given (named as add() would
    /// name it) and whose a is an indexed recording or, with among_new, an earlier one of the range.  Accepts any range of
    /// Collector::FilenameFingerprintPair; min_overlap and the threshold are the caller's.
    template <typename Range>
    auto join(Range &&hashprints, int min_overlap, int rate_num, int rate_den, bool among_new) const -> std::vector<DuplicateResult>
    {
        std::vector<std::string> names = names_;
        std::vector<uint64_t> all;
        std::vector<int64_t> off{0};
        for (auto &p : hashprints) {
            names.push_back(p.filename);
            all.insert(all.end(), p.fingerprint.begin(), p.fingerprint.end());
            off.push_back((int64_t)all.size());
        }
        const int64_t n_x = (int64_t)off.size() - 1;
        std::vector<hpfw_dup_pair> pairs(256);
        int64_t count = 0;
        for (int round = 0; round < 2; ++round) { // (the buffer was too small: once more with room for all)
            check(hpfw_gpu_index_join(h_, all.empty() ? &dummy_ : all.data(), off.data(), n_x, among_new ? 1 : 0, min_overlap, rate_num,
                                      rate_den, pairs.data(), (int64_t)pairs.size(), &count));
            if (count <= (int64_t)pairs.size()) break;
            pairs.resize((size_t)count);
        }
        std::vector<DuplicateResult> out;
        for (int64_t i = 0; i < count; ++i) {
            const hpfw_dup_pair &p = pairs[(size_t)i];
            out.push_back({names[p.a], names[p.b], (size_t)p.dist, (size_t)p.overlap, (int64_t)p.lag});
        }
        return out;
    }

    /// the warped search (hpfw_gpu_search_dtw): the query may run faster or slower than the recording
    /// inside the window (local slope 1/2 .. 2).  candidates is the caller's (there is no default): 0 warps every clip of the
    /// index, k..64 re-ranks that many best clips of the plain search.  Query hashprint 0 lies on column start of the
    /// recording and the last one on column end.
    struct WarpedResult {
        std::string filename;
        size_t cnt;    // mismatching bits along the path
        int64_t start;
        int64_t end;
    };
    auto find_warped(const typename Collector::Hashprint &hp, int k, int candidates) const -> std::vector<WarpedResult>
    {
        std::vector<WarpedResult> out;
        if (hp.empty() || names_.empty()) return out;
        const int64_t q_off[2] = {0, (int64_t)hp.size()};
        std::vector<hpfw_dtw_hit> hits((size_t)k);
        check(hpfw_gpu_search_dtw(h_, hp.data(), q_off, 1, candidates, k, hits.data()));
        for (const hpfw_dtw_hit &hit : hits) {
            if (hit.clip == 0xffffffffu) break;
            out.push_back({names_[hit.clip], (size_t)hit.dist, (int64_t)hit.start, (int64_t)hit.end});
        }
        return out;
    }

    /// the local search (hpfw_gpu_search_local): which part of the query is which part of which
    /// recording.  A run of consecutive query hashprints on one diagonal of a recording scores max_rate * length - cnt;
    /// max_rate, 1..31 mismatching bits per hashprint, is the caller's (there is no default).  Recordings come by larger
    /// score, then by their position in the database.  Query hashprints q_start .. q_start + length - 1 lie on columns
    /// lag + q_start onwards of the recording.
    struct LocalResult {
        std::string filename;
        int64_t score;  // max_rate * length - cnt
        int64_t lag;    // column of the recording query hashprint 0 lies on (negative: before it begins)
        size_t q_start; // first query hashprint of the run
        size_t length;  // hashprints of the run
        size_t cnt;     // mismatching bits over the run
    };
    auto find_local(const typename Collector::Hashprint &hp, int k, int max_rate) const -> std::vector<LocalResult>
    {
        std::vector<LocalResult> out;
        if (hp.empty() || names_.empty()) return out;
        const int64_t q_off[2] = {0, (int64_t)hp.size()};
        std::vector<hpfw_local_hit> hits((size_t)k);
        check(hpfw_gpu_search_local(h_, hp.data(), q_off, 1, max_rate, k, hits.data()));
        for (const hpfw_local_hit &hit : hits) {
            if (hit.clip == 0xffffffffu) break;
            out.push_back({names_[hit.clip], (int64_t)hit.score, (int64_t)hit.lag, (size_t)hit.q_start, (size_t)hit.length, (size_t)hit.dist});
        }
        return out;
    }

    /// the column of recording `clip` (position in the database) every hashprint of the query lies on, and the distance
    /// along that path; nullopt when the recording is too short for the query (fewer than hp.size() / 2 + 1 columns)
    struct WarpPath {
        size_t cnt;
        std::vector<int32_t> columns;
    };
    auto warp_path(const typename Collector::Hashprint &hp, size_t clip) const -> std::optional<WarpPath>
    {
        if (hp.empty() || clip >= names_.size()) return std::nullopt;
        WarpPath out{0, std::vector<int32_t>(hp.size())};
        hpfw_dtw_hit hit;
        check(hpfw_gpu_dtw_path(h_, hp.data(), (int64_t)hp.size(), (int32_t)clip, out.columns.data(), &hit));
        if (hit.clip == 0xffffffffu) return std::nullopt;
        out.cnt = hit.dist;
        return out;
    }

    /// find_overlap() with scores (hpfw_gpu_search_overlap_scored): the same hits, and per hit how far
    /// its rate (mismatching bits per overlapping hashprint, in units of 2^-10) stands out from the rates of the other clips
    /// that have a candidate: (their mean - the rate) / their standard deviation (hpfw_gpu_hit_score; NaN below three clips)
    struct ScoredOverlapResult {
        std::string filename;
        size_t cnt;
        int64_t lag;
        size_t overlap;
        double score;
    };
    auto find_overlap_scored(const typename Collector::Hashprint &hp, int k, int min_overlap) const -> std::vector<ScoredOverlapResult>
    {
        std::vector<ScoredOverlapResult> out;
        if (hp.empty() || names_.empty()) return out;
        const int64_t q_off[2] = {0, (int64_t)hp.size()};
        std::vector<hpfw_overlap_hit> hits((size_t)k);
        hpfw_dist_stats stats{};
        check(hpfw_gpu_search_overlap_scored(h_, hp.data(), q_off, 1, nullptr, min_overlap, k, hits.data(), &stats));
        for (const hpfw_overlap_hit &hit : hits) {
            if (hit.clip == 0xffffffffu) break;
            uint32_t rate = 0;
            double score = 0;
            check(hpfw_gpu_overlap_rate(hit.dist, hit.overlap, &rate));
            check(hpfw_gpu_hit_score(rate, 1, &stats, &score));
            out.push_back({names_[hit.clip], (size_t)hit.dist, (int64_t)hit.lag, (size_t)hit.overlap, score});
        }
        return out;
    }

    /// find() for many queries in one scan of the database (same result per query as find();
    /// an empty hashprint yields the empty result of storage.h:28)
    auto find_batch(const std::vector<typename Collector::Hashprint> &hps) const -> std::vector<SearchResult>
    {
        const SearchResult none{"", std::numeric_limits<size_t>::max(), 0};
        std::vector<SearchResult> out(hps.size(), none);
        if (names_.empty()) return out;
        std::vector<uint64_t> all;
        std::vector<int64_t> off{0};
        std::vector<size_t> which;
        for (size_t i = 0; i < hps.size(); ++i) {
            if (hps[i].empty()) continue;
            all.insert(all.end(), hps[i].begin(), hps[i].end());
            off.push_back((int64_t)all.size());
            which.push_back(i);
        }
        if (which.empty()) return out;
        std::vector<hpfw_hit> hits(which.size());
        check(hpfw_gpu_search_topk(h_, all.data(), off.data(), (int64_t)which.size(), 1, hits.data()));
        for (size_t q = 0; q < which.size(); ++q)
            if (hits[q].clip != 0xffffffffu) out[which[q]] = {names_[hits[q].clip], (size_t)hits[q].dist, (int64_t)hits[q].offset};
        return out;
    }

    size_t size() const { return names_.size(); }
    /// the handle that holds the index and the names of its clips in index order (hpfw::timeline, timeline.h)
    hpfw_gpu *handle() const { return h_; }
    const std::vector<std::string> &names() const { return names_; }

    /// AnnStorage<Collector>::find (reference annoy_storage.h:41-63) with exact nearest neighbours in
    /// place of the Annoy forest: per query position the 5 nearest 64-hashprint windows vote
    /// 1 / (distance + 1) for (track, offset); returns the reference's {filename, cnt, offset} of
    /// the winning bucket ({"", 0, 0} when nothing votes).
    struct VoteResult { // annoy_storage.h:16-20
        std::string filename;
        float cnt;
        int64_t offset;
    };
    auto find_votes(const typename Collector::Hashprint &hp) const -> VoteResult
    {
        if (hp.empty() || names_.empty()) return {"", 0.0f, 0};
        const int64_t q_off[2] = {0, (int64_t)hp.size()};
        hpfw_vote v;
        check(hpfw_gpu_search_votes(h_, hp.data(), q_off, 1, &v));
        if (v.clip == 0xffffffffu) return {"", 0.0f, 0};
        return {names_[v.clip], v.cnt, v.offset};
    }

    /// storage.h:67-75: the cereal BinaryOutputArchive image of std::vector<FilenameFingerprintPair>
    /// (parallel_collector.h:26-35): u64 count, then per entry u64 length + bytes of the filename and
    /// u64 length + that many u64 hashprints.  The FORMAT is the reference's: a dump written by either side loads on
    /// the other.  Whether queries hashed on one side match a database hashed on the other is a separate question:
    /// it needs the same filters.cereal and as far as essentia's unverifiable conventions agree (INTEGRATION.md,
    /// "What a switch changes"; hpfw_gpu_set_conventions).
    auto save(const std::optional<std::string> &filename) const -> std::string
    {
        const auto dump_name = filename.value_or("db/dump.cereal");
        std::vector<int64_t> off(names_.size() + 1, 0);
        check(hpfw_gpu_index_get(h_, off.data(), nullptr, 0));
        std::vector<uint64_t> all((size_t)off.back());
        check(hpfw_gpu_index_get(h_, off.data(), all.empty() ? &dummy_ : all.data(), (int64_t)all.size()));
        std::ofstream os(dump_name, std::ios::binary);
        if (!os) throw std::runtime_error("hpfw::db::GpuStorage: cannot write " + dump_name);
        put(os, (uint64_t)live()); // the live recordings only: the dump loads compact
        for (size_t i = 0; i < names_.size(); ++i) {
            if (removed_[i]) continue;
            put(os, (uint64_t)names_[i].size());
            os.write(names_[i].data(), (std::streamsize)names_[i].size());
            const uint64_t n = (uint64_t)(off[i + 1] - off[i]);
            put(os, n);
            os.write(reinterpret_cast<const char *>(all.data() + off[i]), (std::streamsize)(n * 8));
        }
        if (!os) throw std::runtime_error("hpfw::db::GpuStorage: write failed: " + dump_name);
        return dump_name;
    }

    /// storage.h:78-86
    auto load(const std::string &dump_name) -> GpuStorage &
    {
        std::ifstream is(dump_name, std::ios::binary);
        if (!is) throw std::runtime_error("hpfw::db::GpuStorage: cannot read " + dump_name);
        struct Pair {
            std::string filename;
            std::vector<uint64_t> fingerprint;
        };
        std::vector<Pair> db((size_t)get(is, dump_name));
        for (Pair &p : db) {
            p.filename.resize((size_t)get(is, dump_name));
            is.read(p.filename.data(), (std::streamsize)p.filename.size());
            p.fingerprint.resize((size_t)get(is, dump_name));
            is.read(reinterpret_cast<char *>(p.fingerprint.data()), (std::streamsize)(p.fingerprint.size() * 8));
            if (!is) throw std::runtime_error("hpfw::db::GpuStorage: truncated dump " + dump_name);
        }
        build(db);
        return *this;
    }

private:
    auto within(const typename Collector::Hashprint &hp, int k, const std::vector<int32_t> &clips, bool scored) const -> std::vector<ScoredResult>
    {
        std::vector<ScoredResult> out;
        if (hp.empty() || names_.empty()) return out;
        const int64_t q_off[2] = {0, (int64_t)hp.size()}, set_off[2] = {0, (int64_t)clips.size()};
        const int32_t q_set = 0, none = 0;
        std::vector<hpfw_hit> hits((size_t)k);
        hpfw_dist_stats stats{};
        check(hpfw_gpu_search_topk_within(h_, hp.data(), q_off, 1, k, set_off, 1, clips.empty() ? &none : clips.data(), &q_set, hits.data(),
                                          scored ? &stats : nullptr));
        for (const hpfw_hit &hit : hits) {
            if (hit.clip == 0xffffffffu) break;
            double score = 0;
            if (scored) check(hpfw_gpu_hit_score(hit.dist, added_len_[hit.clip] >= (int64_t)hp.size(), &stats, &score));
            out.push_back({names_[hit.clip], (size_t)hit.dist, (int64_t)hit.offset, score});
        }
        return out;
    }
    static int env_device()
    {
        const char *e = std::getenv("HPFW_GPU_DEVICE");
        return e ? std::atoi(e) : 0;
    }
    static void put(std::ostream &os, uint64_t v) { os.write(reinterpret_cast<const char *>(&v), 8); }
    static uint64_t get(std::istream &is, const std::string &name)
    {
        uint64_t v = 0;
        is.read(reinterpret_cast<char *>(&v), 8);
        if (!is || v > (uint64_t(1) << 40)) throw std::runtime_error("hpfw::db::GpuStorage: malformed dump " + name);
        return v;
    }
    static void check(int rc)
    {
        if (rc != 0) throw std::runtime_error(std::string("hpfw::db::GpuStorage: ") + hpfw_gpu_last_error());
    }
    hpfw_gpu *h_ = nullptr;
    std::vector<std::string> names_;
    std::vector<char> removed_; // per slot: its recording was removed
    std::vector<int64_t> added_len_; // per slot: its hashprints when it was added
    mutable uint64_t dummy_ = 0;
};

} // namespace hpfw::db
