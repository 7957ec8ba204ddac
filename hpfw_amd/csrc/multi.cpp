// multi.cpp -- libhpfw_gpu_multi.so: the multi-GPU host path of include/hpfw_gpu_multi.h.
//
// One process, one hpfw_gpu handle per shard, shards placed on the devices of one node.  What
// LiveSongIdentification::index / search do around MemoryStorage (reference live_song_id.h:31-54,
// storage.h:21-64) becomes: build = contiguous blocks of clips per shard; find = replicated queries, one scan
// per shard (each on its own device and stream, enqueued by its own host thread), ONE ncclAllGather of the
// per-shard top-k lists over xGMI, one deterministic merge.  No torch, no Python: librccl and libamdhip64 only.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include "../../include/hpfw_gpu_multi.h"
#include "../../include/hpfw_gpu_multi_resample.h"
#include "../../include/hpfw_gpu_multi_search.h"
#include "../../include/hpfw_gpu_multi_index.h"
#include "../../include/hpfw_gpu_multi_votes.h"
#include "hip_owned.h"
#include "index_plan.h"
#include "legacy_internal.h"

namespace {

int fail(int code, const std::string &msg)
{
    hpfw_internal_set_error(msg.c_str());
    return code;
}

// move-only owners of what has a C destroy call: a shard's handle, its collector, an RCCL communicator
template <auto Destroy>
struct Del {
    template <class T>
    void operator()(T *p) const { (void)Destroy(p); }
};
using GpuPtr = std::unique_ptr<hpfw_gpu, Del<hpfw_gpu_destroy>>;
using CollectorPtr = std::unique_ptr<hpfw_legacy_collector, Del<par_collector_del>>;
using Comm = std::unique_ptr<std::remove_pointer_t<ncclComm_t>, Del<ncclCommDestroy>>;

// Members are destroyed in reverse order of declaration: a shard's buffer, event and stream go before its handle.
struct Shard {
    int device = 0;    // ordinal of its device
    int dev_slot = 0;  // index into hpfw_gpu_group::devs
    int local = 0;     // position among the shards of that device
    GpuPtr h;
    hpfw::Stream stream;
    hpfw::Event done;
    hpfw::DevBuf d_q;
    int64_t lo = 0, hi = 0; // global clip ids of its block
};

// Reverse order of declaration again: the communicator goes before the device's buffers, the buffers before the stream.
struct Dev {
    int device = 0;
    std::vector<int> shards;
    hpfw::Stream stream;
    // device 0 of a search: the merged hits and summed moments, and (several devices) the gathered regions packed shard
    // after shard
    hpfw::DevBuf d_pack, d_merged;
    hpfw::DevBuf d_recv, d_send; // bytes: hits, then moments (group_search); neighbour keys (group_search_votes)
    hpfw::DevBuf d_db_off;       // device 0: hpfw_gpu_group::db_off
    Comm comm;
};

} // namespace

// The devices go first (reverse order of declaration), then the collectors, then the shards with their handles; the
// destructor waits for every stream before any of that.  None of the frees needs its device to be the current one.
struct hpfw_gpu_group {
    std::vector<Shard> shards;
    std::vector<CollectorPtr> collectors; // one per shard, created by the first load / prepare
    std::vector<Dev> devs;
    std::string cache;
    int per_dev = 1; // shards on every device (uniform)
    int64_t n_clips = 0;
    // the clip offsets of the whole index from 0, as index_build took them, and their copy on device 0 (the tally of the voting
    // search runs there against global positions); uploaded by the first voting search after a build
    std::vector<int64_t> db_off{0};
    bool db_off_dirty = true;
    std::string exchange;
    bool resample = false; // hpfw_gpu_group_set_resample: applied to every shard collector, those made later included
    ~hpfw_gpu_group();
};

namespace {

#define HIP_OK(expr, what)                                                                                         \
    do {                                                                                                           \
        hipError_t e_ = (expr);                                                                                    \
        if (e_ != hipSuccess) return fail(HPFW_E_HIP, std::string(what) + ": " + hipGetErrorString(e_));          \
    } while (0)
#define NCCL_OK(expr, what)                                                                                        \
    do {                                                                                                           \
        ncclResult_t r_ = (expr);                                                                                  \
        if (r_ != ncclSuccess) return fail(HPFW_E_HIP, std::string(what) + ": " + ncclGetErrorString(r_));        \
    } while (0)

int ensure(hpfw::DevBuf &b, size_t bytes)
{
    return b.ensure(bytes) == hipSuccess ? 0 : fail(HPFW_E_NOMEM, "device allocation failed");
}

// Waits for every shard stream and every device stream of the group, all of them whatever fails; the first failure is
// returned and no message is set, so that the caller's earlier failure keeps its own.
hipError_t drain(hpfw_gpu_group *g)
{
    hipError_t first = hipSuccess;
    const auto wait = [&first](int device, const hpfw::Stream &s) {
        if (!s) return;
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = hipStreamSynchronize(s.get());
        if (first == hipSuccess) first = e;
    };
    for (const Shard &s : g->shards) wait(s.device, s.stream);
    for (const Dev &d : g->devs) wait(d.device, d.stream);
    return first;
}

// fn(shard index) on one host thread per shard; the first failure's code and message reach the caller's thread
template <class F>
int per_shard(hpfw_gpu_group *g, F fn)
{
    const int n = (int)g->shards.size();
    std::vector<int> rc((size_t)n, 0);
    std::vector<std::string> why((size_t)n);
    auto run = [&](int i) {
        (void)hipSetDevice(g->shards[(size_t)i].device);
        rc[(size_t)i] = fn(i);
        if (rc[(size_t)i]) why[(size_t)i] = hpfw_gpu_last_error(); // thread-local in libhpfw_gpu.so
    };
    if (n == 1) {
        run(0);
    } else {
        std::vector<std::thread> th;
        for (int i = 1; i < n; ++i) th.emplace_back(run, i);
        run(0);
        for (auto &t : th) t.join();
    }
    for (int i = 0; i < n; ++i)
        if (rc[(size_t)i]) return fail(rc[(size_t)i], "shard " + std::to_string(i) + ": " + why[(size_t)i]);
    return 0;
}

// fn(shard index, lo, hi) on every shard whose block [lo, hi) of n_items items is not empty
template <class F>
int per_shard_range(hpfw_gpu_group *g, int64_t n_items, F fn)
{
    const int n = (int)g->shards.size();
    return per_shard(g, [&](int i) {
        int64_t lo, hi;
        hpfw_gpu_shard_range(n_items, i, n, &lo, &hi);
        return hi == lo ? 0 : fn(i, lo, hi);
    });
}

} // namespace

hpfw_gpu_group::~hpfw_gpu_group() { (void)drain(this); }

extern "C" {

void hpfw_gpu_shard_range(int64_t n_clips, int shard, int n_shards, int64_t *lo, int64_t *hi)
{
    const int64_t base = n_clips / n_shards, extra = n_clips % n_shards;
    const int64_t l = shard * base + std::min<int64_t>(shard, extra);
    if (lo) *lo = l;
    if (hi) *hi = l + base + (shard < extra ? 1 : 0);
}

int hpfw_gpu_group_create(const int *devices, int n_shards, hpfw_gpu_group **out)
{
    if (!out || n_shards < 1 || n_shards > 64) return fail(HPFW_E_INVALID, "bad argument");
    *out = nullptr;
    int n_dev = 0;
    HIP_OK(hipGetDeviceCount(&n_dev), "hipGetDeviceCount");
    auto g = std::make_unique<hpfw_gpu_group>(); // a failure below takes down what was built so far
    g->shards.resize((size_t)n_shards);
    for (int i = 0; i < n_shards; ++i) {
        const int d = devices ? devices[i] : i;
        if (d < 0 || d >= n_dev) return fail(HPFW_E_INVALID, "shard " + std::to_string(i) + ": no device " + std::to_string(d));
        size_t slot = 0;
        while (slot < g->devs.size() && g->devs[slot].device != d) ++slot;
        if (slot == g->devs.size()) {
            g->devs.emplace_back();
            g->devs.back().device = d;
        }
        g->shards[(size_t)i].device = d;
        g->shards[(size_t)i].dev_slot = (int)slot;
        g->shards[(size_t)i].local = (int)g->devs[slot].shards.size();
        g->devs[slot].shards.push_back(i);
    }
    g->per_dev = (int)g->devs[0].shards.size();
    for (const Dev &d : g->devs)
        if ((int)d.shards.size() != g->per_dev) return fail(HPFW_E_INVALID, "every device must hold the same number of shards");
    for (Shard &s : g->shards) {
        hpfw_gpu *h = nullptr;
        if (hpfw_gpu_create(s.device, &h) != 0) return HPFW_E_HIP; // message set by hpfw_gpu_create
        s.h.reset(h);
        if (hipSetDevice(s.device) != hipSuccess || s.stream.create() != hipSuccess || s.done.create() != hipSuccess)
            return fail(HPFW_E_HIP, "stream/event creation failed");
    }
    // one communicator per distinct device, all in this process (ncclCommInitAll); world size 1 is allowed
    std::vector<int> devlist;
    for (Dev &d : g->devs) devlist.push_back(d.device);
    std::vector<ncclComm_t> comms(devlist.size(), nullptr);
    NCCL_OK(ncclCommInitAll(comms.data(), (int)devlist.size(), devlist.data()), "ncclCommInitAll");
    for (size_t i = 0; i < g->devs.size(); ++i) g->devs[i].comm = Comm(comms[i]);
    for (Dev &d : g->devs)
        if (hipSetDevice(d.device) != hipSuccess || d.stream.create() != hipSuccess) return fail(HPFW_E_HIP, "stream creation failed");
    g->exchange = g->per_dev == 1 ? "rccl" : "rccl+local";
    *out = g.release();
    return 0;
}

int hpfw_gpu_group_create_env(hpfw_gpu_group **out)
{
    std::vector<int> devs;
    if (const char *e = std::getenv("HPFW_GPU_DEVICES")) {
        for (const char *p = e; *p;) {
            char *end = nullptr;
            const long v = std::strtol(p, &end, 10);
            if (end == p) return fail(HPFW_E_INVALID, std::string("HPFW_GPU_DEVICES: cannot parse '") + e + "'");
            devs.push_back((int)v);
            p = *end == ',' ? end + 1 : end;
            if (*end && *end != ',') return fail(HPFW_E_INVALID, std::string("HPFW_GPU_DEVICES: cannot parse '") + e + "'");
        }
    }
    if (devs.empty()) {
        int n = 0;
        HIP_OK(hipGetDeviceCount(&n), "hipGetDeviceCount");
        for (int i = 0; i < n; ++i) devs.push_back(i);
    }
    return hpfw_gpu_group_create(devs.data(), (int)devs.size(), out);
}

void hpfw_gpu_group_destroy(hpfw_gpu_group *g) { delete g; } // the destructor drains, then the members go

int hpfw_gpu_group_size(const hpfw_gpu_group *g) { return g ? (int)g->shards.size() : 0; }

hpfw_gpu *hpfw_gpu_group_handle(hpfw_gpu_group *g, int shard)
{
    return g && shard >= 0 && shard < (int)g->shards.size() ? g->shards[(size_t)shard].h.get() : nullptr;
}

const char *hpfw_gpu_group_exchange(const hpfw_gpu_group *g) { return g ? g->exchange.c_str() : ""; }

int hpfw_gpu_group_set_filters(hpfw_gpu_group *g, const float *f)
{
    if (!g || !f) return fail(HPFW_E_INVALID, "null argument");
    for (Shard &s : g->shards) {
        const int rc = hpfw_gpu_set_filters(s.h.get(), f);
        if (rc) return rc;
    }
    return 0;
}

int hpfw_gpu_group_extract_pcm16(hpfw_gpu_group *g, const int16_t *pcm, int64_t n_samples, int64_t n_clips, uint64_t *hp)
{
    if (!g || !pcm || !hp || n_clips < 0) return fail(HPFW_E_INVALID, "bad argument");
    hpfw_geometry geo;
    int rc = hpfw_gpu_geometry(g->shards[0].h.get(), n_samples, &geo);
    if (rc) return rc;
    return per_shard_range(g, n_clips, [&](int i, int64_t lo, int64_t hi) {
        return hpfw_gpu_extract_pcm16_host(g->shards[(size_t)i].h.get(), pcm + lo * n_samples, n_samples, hi - lo, hp + lo * geo.n_hp);
    });
}

int hpfw_gpu_group_index_build(hpfw_gpu_group *g, const uint64_t *hp, const int64_t *offsets, int64_t n_clips)
{
    if (!g || !offsets || n_clips < 0 || (n_clips > 0 && !hp)) return fail(HPFW_E_INVALID, "bad argument");
    if (n_clips > 0xfffffff0ll) return fail(HPFW_E_INVALID, "too many clips");
    const int n = (int)g->shards.size();
    const int rc = per_shard(g, [&](int i) {
        Shard &s = g->shards[(size_t)i];
        hpfw_gpu_shard_range(n_clips, i, n, &s.lo, &s.hi);
        int r = hpfw_gpu_index_clear(s.h.get());
        if (!r) r = hpfw_gpu_index_set_clip_base(s.h.get(), (uint32_t)s.lo);
        if (!r && s.hi > s.lo) r = hpfw_gpu_index_add(s.h.get(), hp, offsets + s.lo, s.hi - s.lo);
        return r;
    });
    if (!rc) {
        g->n_clips = n_clips;
        g->db_off.resize((size_t)n_clips + 1);
        for (int64_t i = 0; i <= n_clips; ++i) g->db_off[(size_t)i] = offsets[i] - offsets[0];
        g->db_off_dirty = true;
    }
    return rc;
}

int64_t hpfw_gpu_group_index_size(const hpfw_gpu_group *g) { return g ? g->n_clips : 0; }

// ---- the searches over the shards (include/hpfw_gpu_multi.h, include/hpfw_gpu_multi_search.h) ----
namespace {

// a shard's copy of the replicated queries, queued on its stream: `total` hashprints from q_hp + first
int upload_queries(Shard &s, const uint64_t *q_hp, int64_t first, int64_t total)
{
    if (int r = ensure(s.d_q, (size_t)std::max<int64_t>(total, 1) * 8)) return r;
    if (total && hipMemcpyAsync(s.d_q.get(), q_hp + first, (size_t)total * 8, hipMemcpyHostToDevice, s.stream.get()) != hipSuccess)
        return fail(HPFW_E_HIP, "H2D copy of the queries failed");
    return 0;
}

// the exchange step of every search: each device's stream waits for its shards' work, then ONE all-gather of the devices'
// send buffers (`send` bytes each) into every device's receive buffer
int all_gather(hpfw_gpu_group *g, size_t send)
{
    for (Dev &d : g->devs) {
        HIP_OK(hipSetDevice(d.device), "hipSetDevice");
        for (int si : d.shards)
            HIP_OK(hipStreamWaitEvent(d.stream.get(), g->shards[(size_t)si].done.get(), 0), "hipStreamWaitEvent");
    }
    NCCL_OK(ncclGroupStart(), "ncclGroupStart");
    for (Dev &d : g->devs) {
        ncclResult_t r = ncclAllGather(d.d_send.get(), d.d_recv.get(), send, ncclUint8, d.comm.get(), d.stream.get());
        if (r != ncclSuccess) {
            (void)ncclGroupEnd();
            return fail(HPFW_E_HIP, std::string("ncclAllGather: ") + ncclGetErrorString(r));
        }
    }
    NCCL_OK(ncclGroupEnd(), "ncclGroupEnd");
    return 0;
}

// The skeleton of every search over the shards.  A shard writes one or two parts (part0, part1 bytes per shard; part1 may be
// 0): a device's send buffer is [local shard] part 0, then [local shard] part 1, and the gathered buffer holds one such
// region per device, 16-byte aligned.
//   1. every shard, on its own stream: the replicated queries in (`total` hashprints from q_hp + first), then
//      shard_call(shard, its slot of part 0, its slot of part 1);
//   2. ONE all-gather of the devices' regions (all_gather);
//   3. on device 0's stream: with several devices the regions' parts packed shard after shard, then
//      finish(device 0, part 0 of all n shards, part 1 of all n shards, the stream), which queues what it makes of them in
//      d_merged (`merged` bytes) and the copy back to the host.
// From the first upload on, queued work reads and writes the caller's host arrays: whichever step fails, the call returns only
// after every stream of the group has been waited for.  A failure of the wait is reported when nothing failed before it.
using ShardCall = std::function<int(Shard &, void *, void *)>;
using Finish = std::function<int(Dev &, const char *, const char *, hipStream_t)>;
static int exchange(hpfw_gpu_group *g, const uint64_t *q_hp, int64_t first, int64_t total, size_t part0, size_t part1, size_t merged,
                    const ShardCall &shard_call, const Finish &finish)
{
    const int m = (int)g->devs.size();
    const size_t dev0 = part0 * g->per_dev, dev1 = part1 * g->per_dev;
    const size_t send = (std::max<size_t>(dev0 + dev1, 16) + 15) / 16 * 16;
    for (Dev &d : g->devs) {
        HIP_OK(hipSetDevice(d.device), "hipSetDevice");
        int rc = ensure(d.d_send, send);
        if (!rc) rc = ensure(d.d_recv, send * m);
        if (rc) return rc;
    }
    Dev &d0 = g->devs[0];
    HIP_OK(hipSetDevice(d0.device), "hipSetDevice");
    int rc = ensure(d0.d_merged, merged);
    if (!rc && m > 1) rc = ensure(d0.d_pack, std::max<size_t>((dev0 + dev1) * m, 16));
    if (rc) return rc;
    const auto fan_out = [&]() {
        return per_shard(g, [&](int i) {
            Shard &s = g->shards[(size_t)i];
            if (int r = upload_queries(s, q_hp, first, total)) return r;
            char *base = g->devs[(size_t)s.dev_slot].d_send.as<char>();
            if (int r = shard_call(s, base + (size_t)s.local * part0, base + dev0 + (size_t)s.local * part1)) return r;
            if (hipEventRecord(s.done.get(), s.stream.get()) != hipSuccess) return fail(HPFW_E_HIP, "event record failed");
            return 0;
        });
    };
    // one device: its region is already [shard] part 0, [shard] part 1
    const auto pack_and_finish = [&]() {
        hipStream_t on = d0.stream.get();
        HIP_OK(hipSetDevice(d0.device), "hipSetDevice");
        const char *recv = d0.d_recv.as<char>();
        const char *in0 = recv, *in1 = recv + dev0;
        if (m > 1) {
            char *pack = d0.d_pack.as<char>();
            for (int i = 0; i < m; ++i) {
                if (dev0)
                    HIP_OK(hipMemcpyAsync(pack + (size_t)i * dev0, recv + (size_t)i * send, dev0, hipMemcpyDeviceToDevice, on),
                           "packing the gathered lists");
                if (dev1)
                    HIP_OK(hipMemcpyAsync(pack + (size_t)m * dev0 + (size_t)i * dev1, recv + (size_t)i * send + dev0, dev1,
                                          hipMemcpyDeviceToDevice, on),
                           "packing the gathered moments");
            }
            in0 = pack;
            in1 = pack + (size_t)m * dev0;
        }
        return finish(d0, in0, in1, on);
    };
    if (!(rc = fan_out()) && !(rc = all_gather(g, send))) rc = pack_and_finish();
    const hipError_t waited = drain(g);
    if (!rc && waited != hipSuccess) rc = fail(HPFW_E_HIP, std::string("all-gather: ") + hipGetErrorString(waited));
    return rc;
}

// One body for the four searches: n_sets = 0 is the plain search (one query set per query, hpfw_hit), n_sets >= 1 the
// transposed one (hpfw_shift_hit); stats non-null asks for the moments.  A shard's parts are its [n_q][k] hits and its
// [rows] moments; device 0 merges the n lists and sums the n rows, and the host takes n_q k hits and the rows.
int group_search(hpfw_gpu_group *g, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int n_sets, int k, void *out,
                 hpfw_dist_stats *stats)
{
    const bool transposed = n_sets > 0;
    const int64_t rows = n_q * (transposed ? n_sets : 1); // query sets
    const int64_t total = q_off[rows] - q_off[0];
    if (total < 0) return fail(HPFW_E_INVALID, "q_off must be non-decreasing");
    if (total > 0 && !q_hp) return fail(HPFW_E_INVALID, "null queries");
    std::vector<int64_t> rel((size_t)rows + 1);
    int64_t k_max = 0;
    for (int64_t i = 0; i <= rows; ++i) rel[(size_t)i] = q_off[i] - q_off[0];
    for (int64_t i = 0; i < rows; ++i) {
        if (rel[(size_t)i + 1] < rel[(size_t)i]) return fail(HPFW_E_INVALID, "q_off must be non-decreasing");
        k_max = std::max(k_max, rel[(size_t)i + 1] - rel[(size_t)i]);
    }
    // the limits of the one-handle call on the unsharded index: a shard sees only its own block of clips, and the sum
    // of the shards' rows must not wrap where the unsharded row would be refused
    if (g->n_clips > 0 && k_max > 16000) return fail(HPFW_E_UNSUPPORTED, "query longer than 16000 hashprints");
    if (stats && (unsigned __int128)g->n_clips * (uint64_t)(k_max * k_max) * 4096 >= ((unsigned __int128)1 << 64))
        return fail(HPFW_E_UNSUPPORTED, "scored search: n_clips * k_max^2 * 4096 must stay below 2^64");
    const int n = (int)g->shards.size();
    const size_t list = (size_t)n_q * k * sizeof(hpfw_hit);                  // bytes of hits per shard
    const size_t srows = stats ? (size_t)rows * sizeof(hpfw_dist_stats) : 0; // bytes of moments per shard
    return exchange(
        g, q_hp, q_off[0], total, list, srows, list + srows,
        [&](Shard &s, void *hits, void *moments) {
            uint64_t *d_q = s.d_q.as<uint64_t>();
            hpfw_dist_stats *st = stats ? static_cast<hpfw_dist_stats *>(moments) : nullptr;
            hpfw_gpu *h = s.h.get();
            hipStream_t on = s.stream.get();
            if (transposed)
                return st ? hpfw_gpu_search_topk_transposed_scored_device(h, d_q, rel.data(), n_q, n_sets, k, (hpfw_shift_hit *)hits, st, on)
                          : hpfw_gpu_search_topk_transposed_device(h, d_q, rel.data(), n_q, n_sets, k, (hpfw_shift_hit *)hits, on);
            return st ? hpfw_gpu_search_topk_scored_device(h, d_q, rel.data(), n_q, k, (hpfw_hit *)hits, st, on)
                      : hpfw_gpu_search_topk_device(h, d_q, rel.data(), n_q, k, (hpfw_hit *)hits, on);
        },
        [&](Dev &d0, const char *hits_in, const char *stats_in, hipStream_t on) {
            hpfw_gpu *h0 = g->shards[(size_t)d0.shards[0]].h.get();
            char *merged = d0.d_merged.as<char>();
            int r = hpfw_gpu_merge_topk_device(h0, hits_in, n, n_q, k, merged, on);
            if (!r && stats)
                r = hpfw_gpu_sum_stats_device(h0, reinterpret_cast<const hpfw_dist_stats *>(stats_in), n, rows,
                                              reinterpret_cast<hpfw_dist_stats *>(merged + list), on);
            if (r) return r;
            HIP_OK(hipMemcpyAsync(out, merged, list, hipMemcpyDeviceToHost, on), "D2H copy of the merged lists");
            if (stats) HIP_OK(hipMemcpyAsync(stats, merged + list, srows, hipMemcpyDeviceToHost, on), "D2H copy of the moments");
            return 0;
        });
}

// the argument checks of the one-handle functions, before the group or any device is touched
int group_search_checked(hpfw_gpu_group *g, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int n_sets, bool transposed,
                         int k, void *out, hpfw_dist_stats *stats, bool scored)
{
    if (scored && !stats) return fail(HPFW_E_INVALID, "null stats");
    if (transposed && (n_sets < 1 || n_sets > 64)) return fail(HPFW_E_INVALID, "bad argument");
    if (k < 1 || k > 64) return fail(HPFW_E_INVALID, "k must be in 1..64");
    if (!g || !q_off || !out || n_q < 0) return fail(HPFW_E_INVALID, "bad argument");
    if (n_q == 0) return 0;
    return group_search(g, q_hp, q_off, n_q, transposed ? n_sets : 0, k, out, scored ? stats : nullptr);
}

} // namespace

// ---- the voting search over the shards (include/hpfw_gpu_multi_votes.h) ----
// Replicated queries -> per shard the 5 nearest windows of every query window in its own block of clips -> ONE all-gather of
// the key lists -> device 0: the lists merged with every shard's first position added (the unsharded list, ties included),
// the tally against the whole index's offsets, n_q votes back.
int hpfw_gpu_group_search_votes(hpfw_gpu_group *g, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, hpfw_vote *out)
{
    if (!g || !q_off || !out || n_q < 0) return fail(HPFW_E_INVALID, "bad argument");
    if (n_q == 0) return 0;
    std::vector<int64_t> rel((size_t)n_q + 1), wf((size_t)n_q + 1, 0);
    for (int64_t i = 0; i <= n_q; ++i) rel[(size_t)i] = q_off[i] - q_off[0];
    for (int64_t i = 0; i < n_q; ++i) {
        const int64_t k = rel[(size_t)i + 1] - rel[(size_t)i];
        if (k < 0) return fail(HPFW_E_INVALID, "q_off must be non-decreasing");
        wf[(size_t)i + 1] = wf[(size_t)i] + std::max<int64_t>(k - 63, 0);
    }
    const int64_t total = rel[(size_t)n_q], n_win = wf[(size_t)n_q];
    if (total > 0 && !q_hp) return fail(HPFW_E_INVALID, "null queries");
    const int n = (int)g->shards.size();
    const size_t list = (size_t)n_win * 5 * 8; // bytes of keys per shard
    const size_t list_al = (list + 15) / 16 * 16, votes = (size_t)n_q * sizeof(hpfw_vote);
    HIP_OK(hipSetDevice(g->devs[0].device), "hipSetDevice");
    if (int rc = ensure(g->devs[0].d_db_off, g->db_off.size() * 8)) return rc;
    std::vector<int64_t> pos_base((size_t)n);
    for (int i = 0; i < n; ++i) {
        int64_t lo, hi;
        hpfw_gpu_shard_range(g->n_clips, i, n, &lo, &hi);
        pos_base[(size_t)i] = g->db_off[(size_t)lo];
    }
    return exchange(
        g, q_hp, q_off[0], total, list, 0, list_al + votes,
        [&](Shard &s, void *keys, void *) {
            return hpfw_gpu_knn_windows_device(s.h.get(), s.d_q.as<uint64_t>(), rel.data(), n_q, static_cast<uint64_t *>(keys), n_win * 5,
                                               s.stream.get());
        },
        [&](Dev &d0, const char *keys_in, const char *, hipStream_t on) {
            if (g->db_off_dirty) {
                HIP_OK(hipMemcpyAsync(d0.d_db_off.get(), g->db_off.data(), g->db_off.size() * 8, hipMemcpyHostToDevice, on), "H2D copy of the offsets");
                HIP_OK(hipStreamSynchronize(on), "H2D copy of the offsets");
                g->db_off_dirty = false;
            }
            hpfw_gpu *h0 = g->shards[(size_t)d0.shards[0]].h.get();
            char *merged = d0.d_merged.as<char>();
            hpfw_vote *d_votes = reinterpret_cast<hpfw_vote *>(merged + list_al);
            int r = hpfw_gpu_merge_knn_device(h0, reinterpret_cast<const uint64_t *>(keys_in), pos_base.data(), n, n_win,
                                              reinterpret_cast<uint64_t *>(merged), on);
            if (!r)
                r = hpfw_gpu_vote_windows_device(h0, reinterpret_cast<const uint64_t *>(merged), wf.data(), n_q, d0.d_db_off.as<int64_t>(), g->n_clips,
                                                 0, d_votes, on);
            if (r) return r;
            HIP_OK(hipMemcpyAsync(out, d_votes, votes, hipMemcpyDeviceToHost, on), "D2H copy of the votes");
            return 0;
        });
}

// ---- removal from the sharded index (include/hpfw_gpu_multi_index.h) ----
// Global ids are checked against the group's clip count, routed to the shard whose range holds them and handed to
// hpfw_gpu_index_remove as local ids on the shard's stream; the group's own offsets follow the same rule.  No collective.
int hpfw_gpu_group_index_remove(hpfw_gpu_group *g, const int64_t *clips, int64_t n)
{
    if (!g) return fail(HPFW_E_INVALID, "null group");
    if (n < 0) return fail(HPFW_E_INVALID, "n must not be negative");
    if (n > 0 && !clips) return fail(HPFW_E_INVALID, "null clips");
    for (int64_t i = 0; i < n; ++i)
        if (clips[i] < 0 || clips[i] >= g->n_clips)
            return fail(HPFW_E_INVALID, "group_index_remove: clip " + std::to_string(clips[i]) + " outside [0, " + std::to_string(g->n_clips) + ")");
    if (n == 0) return 0;
    std::vector<int64_t> ids(clips, clips + n);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    std::vector<int64_t> new_off(g->db_off.size());
    if (!hpfw::index_remove_plan(g->db_off.data(), g->n_clips, ids.data(), (int64_t)ids.size(), 1, new_off.data(), nullptr))
        return fail(HPFW_E_INVALID, "group_index_remove: no plan");
    const int rc = per_shard(g, [&](int i) {
        Shard &s = g->shards[(size_t)i];
        std::vector<int64_t> local;
        for (auto it = std::lower_bound(ids.begin(), ids.end(), s.lo); it != ids.end() && *it < s.hi; ++it) local.push_back(*it - s.lo);
        return local.empty() ? 0 : hpfw_gpu_index_remove(s.h.get(), local.data(), (int64_t)local.size(), s.stream.get());
    });
    if (!rc) {
        g->db_off = std::move(new_off);
        g->db_off_dirty = true;
    }
    return rc;
}

int hpfw_gpu_group_search_topk(hpfw_gpu_group *g, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int k, hpfw_hit *out)
{
    return group_search_checked(g, q_hp, q_off, n_q, 0, false, k, out, nullptr, false);
}

int hpfw_gpu_group_search_topk_scored(hpfw_gpu_group *g, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int k, hpfw_hit *out,
                                      hpfw_dist_stats *stats)
{
    return group_search_checked(g, q_hp, q_off, n_q, 0, false, k, out, stats, true);
}

int hpfw_gpu_group_search_topk_transposed(hpfw_gpu_group *g, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int n_shifts, int k,
                                          hpfw_shift_hit *out)
{
    return group_search_checked(g, q_hp, q_off, n_q, n_shifts, true, k, out, nullptr, false);
}

int hpfw_gpu_group_search_topk_transposed_scored(hpfw_gpu_group *g, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int n_shifts,
                                                 int k, hpfw_shift_hit *out, hpfw_dist_stats *stats)
{
    return group_search_checked(g, q_hp, q_off, n_q, n_shifts, true, k, out, stats, true);
}

int hpfw_gpu_group_extract_windows_pcm16(hpfw_gpu_group *g, const int16_t *pcm, int64_t n_total, int64_t win, int64_t hop,
                                         const float *tempos, int n_tempos, const int32_t *shifts, int n_shifts, uint64_t *hp)
{
    if (!g) return fail(HPFW_E_INVALID, "null group");
    hpfw_gpu *h0 = g->shards[0].h.get();
    // the one-handle call's checks (lists, projection mode, window and hop, a window too short for the slowest tempo), made
    // once: over no samples it checks everything and extracts nothing
    int rc = hpfw_gpu_extract_windows_pcm16_host(h0, nullptr, 0, win, hop, tempos, n_tempos, shifts, n_shifts, nullptr);
    if (rc) return rc;
    int64_t n_w = 0;
    if ((rc = hpfw_gpu_window_count(n_total, win, hop, &n_w))) return rc;
    if (n_w == 0) return 0;
    if (!pcm || !hp) return fail(HPFW_E_INVALID, "bad argument");
    hpfw_geometry geo;
    if ((rc = hpfw_gpu_geometry(h0, win, &geo))) return rc;
    int64_t n_hp = geo.n_hp;
    if (tempos) {
        int64_t c_t = 0;
        if ((rc = hpfw_gpu_tempo_columns(geo.c, tempos, n_tempos, &c_t))) return rc;
        n_hp = c_t - (HPFW_CONTEXT - 1) - HPFW_LAG;
    }
    const int64_t per_window = (int64_t)(tempos ? n_tempos : 1) * std::max(n_shifts, 1) * n_hp;
    return per_shard_range(g, n_w, [&](int i, int64_t lo, int64_t hi) {
        return hpfw_gpu_extract_windows_pcm16_host(g->shards[(size_t)i].h.get(), pcm + lo * hop, (hi - 1 - lo) * hop + win, win, hop, tempos,
                                                   n_tempos, shifts, n_shifts, hp + lo * per_window);
    });
}

int hpfw_gpu_group_cov_reset(hpfw_gpu_group *g)
{
    if (!g) return fail(HPFW_E_INVALID, "null group");
    for (Shard &s : g->shards) {
        const int rc = hpfw_gpu_cov_reset(s.h.get());
        if (rc) return rc;
    }
    return 0;
}

int hpfw_gpu_group_cov_accumulate_pcm16(hpfw_gpu_group *g, const int16_t *pcm, int64_t n_samples, int64_t n_clips)
{
    if (!g || !pcm || n_clips < 0) return fail(HPFW_E_INVALID, "bad argument");
    return per_shard_range(g, n_clips, [&](int i, int64_t lo, int64_t hi) {
        return hpfw_gpu_cov_accumulate_pcm16_host(g->shards[(size_t)i].h.get(), pcm + lo * n_samples, n_samples, hi - lo);
    });
}

// accum_cov summed over the given handles (one per shard, shard order): afterwards every handle holds the total
// and the total file count.  One in-place ncclAllReduce of 23.4 MB when every shard has its own device.
static int sum_covariances(hpfw_gpu_group *g, const std::vector<hpfw_gpu *> &hs, int64_t *files_out)
{
    const size_t nn = (size_t)HPFW_FRAME_SIZE * HPFW_FRAME_SIZE;
    int64_t files = 0;
    for (hpfw_gpu *h : hs) files += hpfw_gpu_cov_files(h);
    *files_out = files;
    if (files == 0) return fail(HPFW_E_INVALID, "no covariance accumulated");
    int rc;
    if (g->per_dev == 1) {
        // accum_cov is a plain sum over files (parallel_collector.h:93-97)
        std::vector<float *> d_cov(hs.size(), nullptr);
        for (size_t i = 0; i < hs.size(); ++i)
            if ((rc = hpfw_gpu_cov_device(hs[i], &d_cov[i]))) return rc;
        for (Dev &d : g->devs) {
            HIP_OK(hipSetDevice(d.device), "hipSetDevice");
            HIP_OK(hipDeviceSynchronize(), "covariance kernels"); // the accumulation ran on the handles' own streams
        }
        NCCL_OK(ncclGroupStart(), "ncclGroupStart");
        for (Dev &d : g->devs) {
            float *p = d_cov[(size_t)d.shards[0]];
            ncclResult_t r = ncclAllReduce(p, p, nn, ncclFloat, ncclSum, d.comm.get(), d.stream.get());
            if (r != ncclSuccess) {
                (void)ncclGroupEnd();
                return fail(HPFW_E_HIP, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
            }
        }
        NCCL_OK(ncclGroupEnd(), "ncclGroupEnd");
        for (Dev &d : g->devs) {
            HIP_OK(hipSetDevice(d.device), "hipSetDevice");
            HIP_OK(hipStreamSynchronize(d.stream.get()), "all-reduce");
        }
    } else {
        // shards that share a device: their matrices are summed on the host (RCCL has one rank per device)
        std::vector<float> sum(nn, 0.0f), one(nn);
        for (hpfw_gpu *h : hs) {
            if ((rc = hpfw_gpu_cov_get(h, one.data(), nullptr))) return rc;
            for (size_t i = 0; i < nn; ++i) sum[i] += one[i];
        }
        for (hpfw_gpu *h : hs)
            if ((rc = hpfw_gpu_cov_set(h, sum.data(), files))) return rc;
    }
    for (hpfw_gpu *h : hs)
        if ((rc = hpfw_gpu_cov_set_files(h, files))) return rc;
    return 0;
}

int hpfw_gpu_group_learn_filters(hpfw_gpu_group *g, float *filters_out)
{
    if (!g) return fail(HPFW_E_INVALID, "null group");
    std::vector<hpfw_gpu *> hs;
    for (Shard &s : g->shards) hs.push_back(s.h.get());
    int64_t files = 0;
    int rc = sum_covariances(g, hs, &files);
    if (rc) return rc;
    std::vector<float> f((size_t)HPFW_FILTERS * HPFW_FRAME_SIZE);
    HIP_OK(hipSetDevice(g->shards[0].device), "hipSetDevice");
    if ((rc = hpfw_gpu_learn_filters(g->shards[0].h.get(), f.data()))) return rc;
    for (size_t i = 1; i < g->shards.size(); ++i)
        if ((rc = hpfw_gpu_set_filters(g->shards[i].h.get(), f.data()))) return rc;
    // the reference keeps accumulating across calls (parallel_collector.h:93-97): the total stays on shard 0 only, so
    // that an accumulate + learn that follows adds every earlier file once and not once per shard
    for (size_t i = 1; i < g->shards.size(); ++i)
        if ((rc = hpfw_gpu_cov_reset(g->shards[i].h.get()))) return rc;
    if (filters_out) std::memcpy(filters_out, f.data(), f.size() * 4);
    return 0;
}

// ---- ParallelCollector over the shards ----------------------------------------------------------------------
static int ensure_collectors(hpfw_gpu_group *g, const char *cache)
{
    if (cache && *cache) g->cache = cache;
    if (!g->collectors.empty()) return 0;
    for (size_t i = 0; i < g->shards.size(); ++i) {
        hpfw_legacy_collector *c = hpfw_internal_collector_on_device(g->shards[i].device, g->cache.c_str());
        if (!c) {
            g->collectors.clear();
            return HPFW_E_HIP; // message set by hpfw_gpu_create
        }
        // accum_cov.cereal carries the covariance of earlier runs (the reference keeps accumulating, cache.h:34-36,
        // live_song_id.h:23-29): it enters the sum once, through shard 0
        if (i > 0) (void)hpfw_gpu_cov_reset(hpfw_internal_collector_gpu(c));
        (void)hpfw_gpu_collector_set_resample(c, g->resample);
        g->collectors.emplace_back(c);
    }
    return 0;
}

int hpfw_gpu_group_set_resample(hpfw_gpu_group *g, int on)
{
    if (!g) return fail(HPFW_E_INVALID, "null group");
    g->resample = on != 0;
    for (auto &c : g->collectors) (void)hpfw_gpu_collector_set_resample(c.get(), g->resample);
    return 0;
}

int hpfw_gpu_group_load(hpfw_gpu_group *g, const char *cache)
{
    if (!g) return fail(HPFW_E_INVALID, "null group");
    if (!g->collectors.empty()) { // load again: every shard re-reads the cache
        if (cache && *cache) g->cache = cache;
        for (size_t i = 0; i < g->collectors.size(); ++i) {
            par_collector_load(g->collectors[i].get(), g->cache.c_str());
            if (i > 0) (void)hpfw_gpu_cov_reset(hpfw_internal_collector_gpu(g->collectors[i].get()));
        }
        return 0;
    }
    return ensure_collectors(g, cache);
}

int hpfw_gpu_group_save(hpfw_gpu_group *g, const char *cache)
{
    if (!g) return fail(HPFW_E_INVALID, "null group");
    if (cache && *cache) g->cache = cache;
    if (g->collectors.empty()) return 0; // nothing loaded, nothing learned
    par_collector_save(g->collectors[0].get(), g->cache.c_str());
    return 0;
}

FilenameHashprintPair *hpfw_gpu_group_prepare(hpfw_gpu_group *g, const char **filenames, int n, int *got)
{
    if (got) *got = 0;
    if (!g || !filenames || n < 0 || !got) {
        (void)fail(HPFW_E_INVALID, "bad argument");
        return nullptr;
    }
    if (ensure_collectors(g, nullptr)) return nullptr;
    const int ns = (int)g->shards.size();
    const bool learn = !std::getenv("HPFW_PREPARE_KEEP_FILTERS");
    std::vector<hpfw_prepare_job *> jobs((size_t)ns, nullptr);
    std::vector<int64_t> lo((size_t)ns), hi((size_t)ns);
    for (int i = 0; i < ns; ++i) hpfw_gpu_shard_range(n, i, ns, &lo[(size_t)i], &hi[(size_t)i]);
    // 1. preprocess (parallel_collector.h:82-105) on every shard's block of files
    int rc = per_shard(g, [&](int i) {
        jobs[(size_t)i] = hpfw_internal_prepare_accumulate(g->collectors[(size_t)i].get(), filenames + lo[(size_t)i],
                                                           (int)(hi[(size_t)i] - lo[(size_t)i]), learn ? 1 : 0);
        return jobs[(size_t)i] ? 0 : (int)HPFW_E_NOMEM;
    });
    // 2. one all-reduce of accum_cov, the eigen-solve on shard 0 (:111), the filters to every shard, the cache saved (:61-66)
    bool ok = rc == 0;
    if (ok && learn) {
        std::vector<hpfw_gpu *> hs;
        for (auto &c : g->collectors) hs.push_back(hpfw_internal_collector_gpu(c.get()));
        int64_t files = 0, used = 0;
        for (hpfw_prepare_job *j : jobs) used += hpfw_internal_prepare_used(j);
        std::vector<float> f((size_t)HPFW_FILTERS * HPFW_FRAME_SIZE);
        ok = used > 0 && sum_covariances(g, hs, &files) == 0 && hipSetDevice(hpfw_gpu_device(hs[0])) == hipSuccess &&
             hpfw_gpu_learn_filters(hs[0], f.data()) == 0;
        for (size_t i = 0; ok && i < g->collectors.size(); ++i) ok = hpfw_internal_collector_set_filters(g->collectors[i].get(), f.data()) == 0;
        // the total stays on shard 0 only, so that the next prepare() adds every file once
        for (size_t i = 1; i < hs.size(); ++i) (void)hpfw_gpu_cov_reset(hs[i]);
        if (ok) par_collector_save(g->collectors[0].get(), g->cache.c_str());
        if (used == 0) ok = true; // nothing readable: an empty result, as the single collector returns
    }
    // 3. collect_fingerprints (:115-137): every shard hashes its own files; shard 0 adds the older tracks of the cache
    std::vector<FilenameHashprintPair *> part((size_t)ns, nullptr);
    std::vector<int> part_n((size_t)ns, 0);
    (void)per_shard(g, [&](int i) {
        if (jobs[(size_t)i])
            part[(size_t)i] = hpfw_internal_prepare_finish(g->collectors[(size_t)i].get(), jobs[(size_t)i], filenames + lo[(size_t)i],
                                                           (int)(hi[(size_t)i] - lo[(size_t)i]), ok ? 1 : 0, 0, &part_n[(size_t)i]);
        return 0;
    });
    FilenameHashprintPair *cached = nullptr;
    int cached_n = 0;
    if (ok && !std::getenv("HPFW_NO_SPECTRO_CACHE")) // older tracks: a walk of the cache, told about all n names
        cached = hpfw_internal_prepare_finish_cached(g->collectors[0].get(), filenames, n, &cached_n);
    if (!ok) {
        for (int i = 0; i < ns; ++i)
            if (part[(size_t)i]) prepare_result_free(part[(size_t)i], part_n[(size_t)i]);
        (void)fail(HPFW_E_INVALID, "prepare: the filters could not be learned");
        return nullptr;
    }
    int total = cached_n;
    for (int i = 0; i < ns; ++i) total += part_n[(size_t)i];
    auto *res = new FilenameHashprintPair[(size_t)std::max(total, 1)];
    int w = 0;
    auto take = [&](FilenameHashprintPair *p, int cnt) {
        for (int k = 0; k < cnt; ++k) res[w++] = p[k]; // ownership of the strings and hashprints moves
        delete[] p;
    };
    for (int i = 0; i < ns; ++i)
        if (part[(size_t)i]) take(part[(size_t)i], part_n[(size_t)i]);
    if (cached) take(cached, cached_n);
    *got = w;
    return res;
}

uint64_t *hpfw_gpu_group_calc_hashprint(hpfw_gpu_group *g, const char *filename, int *size)
{
    if (size) *size = 0;
    if (!g || !filename || !size || ensure_collectors(g, nullptr)) return nullptr;
    (void)hipSetDevice(g->shards[0].device);
    return par_collector_calc_hashprint(g->collectors[0].get(), filename, size);
}

} // extern "C"
