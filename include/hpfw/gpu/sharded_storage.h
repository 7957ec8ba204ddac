// sharded_storage.h -- hpfw::db::ShardedGpuStorage<Collector>: MemoryStorage<Collector> (reference
// include/hpfw/audioproblems/live-song-id/storage.h:8-92) over the GPUs of one node, usable as the `Storage`
// template argument of LiveSongIdentification (reference live_song_id.h:19-21) exactly like GpuStorage.
//
// build() shards the tracks per audio file -- contiguous blocks of the input range, one per shard, each
// resident in its GPU's HBM under its global track ids; find() replicates the query, every shard scans its
// block and keeps its own top-k, ONE RCCL all-gather of the per-shard lists over xGMI follows, and the lists
// are merged by (distance, track id): the answer is the one GpuStorage gives on the unsharded index, for any
// number of shards.  Header-only; the work is done by libhpfw_gpu_multi.so (include/hpfw_gpu_multi.h).
//
// The finds of a query in another key or at another tempo (transposed.h, tempo.h) and the scored searches behind
// hpfw::timeline (timeline.h) are here too, over include/hpfw_gpu_multi_search.h: same names and result types as GpuStorage's.
// So is the voting search (find_votes, include/hpfw_gpu_multi_votes.h).
//
// Placement: HPFW_GPU_DEVICES="0,1,2,3,4,5,6,7" (one ordinal per shard; default: every visible device), or
// the explicit constructor.
#pragma once

#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../hpfw_gpu_multi.h"
#include "../../hpfw_gpu_multi_index.h"
#include "../../hpfw_gpu_multi_search.h"
#include "../../hpfw_gpu_multi_votes.h"

namespace hpfw::db {

template <typename Collector>
class ShardedGpuStorage {
public:
    struct SearchResult { // storage.h:11-15
        std::string filename;
        size_t cnt;
        int64_t offset;
    };

    ShardedGpuStorage() { check(hpfw_gpu_group_create_env(&g_)); }
    explicit ShardedGpuStorage(const std::vector<int> &devices) { check(hpfw_gpu_group_create(devices.data(), (int)devices.size(), &g_)); }
    ~ShardedGpuStorage() { hpfw_gpu_group_destroy(g_); }
    ShardedGpuStorage(const ShardedGpuStorage &) = delete;
    ShardedGpuStorage &operator=(const ShardedGpuStorage &) = delete;

    int shards() const { return hpfw_gpu_group_size(g_); }
    size_t size() const { return names_.size(); }

    /// storage.h:21-25; accepts any range of Collector::FilenameFingerprintPair
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
        check(hpfw_gpu_group_index_build(g_, all.empty() ? &dummy_ : all.data(), off.data(), (int64_t)names_.size()));
        off_ = off;
        removed_.assign(names_.size(), 0); // a fresh index forgets all removals
    }

    /// GpuStorage::remove over the shards (hpfw_gpu_group_index_remove): the recordings named leave
    /// their shards in place; slots are ids, so names() and size() keep counting them and live() counts what remains.  A
    /// name that is unknown (or already removed) throws std::out_of_range before anything changes.  There is no add():
    /// a sharded index is rebuilt (include/hpfw_gpu_multi_index.h).
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
            if (!found) throw std::out_of_range("hpfw::db::ShardedGpuStorage: no recording " + name);
        }
        if (ids.empty()) return 0;
        check(hpfw_gpu_group_index_remove(g_, ids.data(), (int64_t)ids.size()));
        size_t n = 0;
        for (int64_t i : ids) { // (a name may repeat in the list)
            n += !removed_[(size_t)i];
            removed_[(size_t)i] = 1;
        }
        std::vector<int64_t> off(off_.size(), 0);
        for (size_t i = 0; i < names_.size(); ++i) off[i + 1] = off[i] + (removed_[i] ? 0 : off_[i + 1] - off_[i]);
        off_ = off;
        return n;
    }

    /// the recordings that remain (size() counts slots)
    size_t live() const
    {
        size_t n = 0;
        for (char r : removed_) n += !r;
        return n;
    }

    /// the group that holds the shards, the names of the clips in index order and their offsets [size() + 1] (hpfw::timeline,
    /// timeline.h, searches a sharded storage through these)
    hpfw_gpu_group *group() const { return g_; }
    const std::vector<std::string> &names() const { return names_; }
    const std::vector<int64_t> &index_offsets() const { return off_; }

    /// GpuStorage::find_topk_transposed over the shards: per_shift[i] holds the query's hashprints under variant i
    /// (hpfw::transposed_hashprints, hpfw::tempo_hashprints); per clip the smallest distance over the variants, ties to the
    /// first; the k best clips by (distance, position in the database) with the index of their variant
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
        check(hpfw_gpu_group_search_topk_transposed(g_, all.empty() ? &dummy_ : all.data(), off.data(), 1, (int)per_shift.size(), k, hits.data()));
        for (const hpfw_shift_hit &hit : hits) {
            if (hit.clip == 0xffffffffu) break;
            out.push_back({names_[hit.clip], (size_t)hit.dist, (int64_t)hit.offset, (int)hit.shift_index});
        }
        return out;
    }

    /// storage.h:27-64: the first strict minimum in database order
    auto find(const typename Collector::Hashprint &hp) const -> SearchResult
    {
        auto top = find_topk(hp, 1);
        if (top.empty()) return {"", std::numeric_limits<size_t>::max(), 0}; // storage.h:28
        return top[0];
    }

    /// the notebook's "k best tracks" (examples/python/liveid.ipynb cell 9), by (distance, position in the database)
    auto find_topk(const typename Collector::Hashprint &hp, int k) const -> std::vector<SearchResult>
    {
        std::vector<SearchResult> out;
        if (hp.empty() || names_.empty()) return out;
        const int64_t q_off[2] = {0, (int64_t)hp.size()};
        std::vector<hpfw_hit> hits((size_t)k);
        check(hpfw_gpu_group_search_topk(g_, hp.data(), q_off, 1, k, hits.data()));
        for (const hpfw_hit &hit : hits) {
            if (hit.clip == 0xffffffffu) break;
            out.push_back({names_[hit.clip], (size_t)hit.dist, (int64_t)hit.offset});
        }
        return out;
    }

    /// find() for many queries with one scan per shard and one all-gather
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
        check(hpfw_gpu_group_search_topk(g_, all.data(), off.data(), (int64_t)which.size(), 1, hits.data()));
        for (size_t q = 0; q < which.size(); ++q)
            if (hits[q].clip != 0xffffffffu) out[which[q]] = {names_[hits[q].clip], (size_t)hits[q].dist, (int64_t)hits[q].offset};
        return out;
    }

    /// GpuStorage::find_votes over the shards (AnnStorage::find, annoy_storage.h:41-63, with exact neighbours): the
    /// reference's {filename, cnt, offset} of the winning bucket, {"", 0, 0} when nothing votes
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
        check(hpfw_gpu_group_search_votes(g_, hp.data(), q_off, 1, &v));
        if (v.clip == 0xffffffffu) return {"", 0.0f, 0};
        return {names_[v.clip], v.cnt, v.offset};
    }

private:
    static void check(int rc)
    {
        if (rc != 0) throw std::runtime_error(std::string("hpfw::db::ShardedGpuStorage: ") + hpfw_gpu_last_error());
    }
    hpfw_gpu_group *g_ = nullptr;
    std::vector<std::string> names_;
    std::vector<int64_t> off_{0};
    std::vector<char> removed_; // per slot: its recording was removed
    mutable uint64_t dummy_ = 0;
};

} // namespace hpfw::db
