// handle.h -- what the sources of the C-ABI declared in include/hpfw_gpu.h (handle.hip, plans.hip, extract.hip, learn.hip,
// search.hip, selfjoin.hip, dtw.hip, local.hip, votes.hip, combiner.hip, warp.hip) share.  Host orchestration only: plans, workspaces, batching over clips (the role of
// ParallelCollector::collect_fingerprints' parallel_for, reference
// include/hpfw/core/parallel_collector.h:115-137) and MemoryStorage::build/find
// (include/hpfw/audioproblems/live-song-id/storage.h:21-64).  All arithmetic is in the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "../../include/hpfw_gpu.h"
#include "combiner.h"
#include "hip_owned.h"
#include "kernels.h"
#include "legacy_internal.h" // hpfw_internal_set_error (handle.hip), hpfw_internal_note_idle (plans.hip)
#include "plan.h"
#include "search_plan.h"

using hpfw::DevBuf, hpfw::Event, hpfw::HostBuf, hpfw::Stream;

int fail(int code, const std::string &msg);

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(HPFW_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                 \
    } while (0)

// Device memory of the per-length tables.  A plan takes its memory from the handle's pool: small tables are carved out of
// 4 MB chunks, large ones are blocks of their own, and an evicted plan's chunks and blocks go back to the pool for the next
// length (a corpus of tracks brings a new length with every file: ~40 hipMalloc and, at eviction, as many hipFree per plan
// cost more than generating the tables).
struct DevPlan {
    hpfw_gpu *owner = nullptr;
    std::vector<DevBuf> blocks; // what this plan holds of the pool, each block with its real size
    char *cur = nullptr;                           // the open chunk
    size_t left = 0;
    // small tables are written to a host image of the open chunk and go over in one copy per run of them (plan_flush):
    // some thirty-five synchronous copies of a few KB each cost more than the tables' bytes
    char *chunk_base = nullptr;
    std::vector<char> stage;
    std::vector<std::pair<size_t, size_t>> staged; // (offset, bytes) written to the image, in order
    hpfw::HostPlan hp;
    hpfw::ColsQArgs cols;
    hpfw::Rows2Out rows_out;
    hpfw::RowsArgs rows;
    hpfw::BzArgs bz; // clip lengths with a prime factor above 7 (hp.bluestein)
    hpfw::CqPlanDev cq;
    std::vector<hpfw::CqClassDev> cls;
    int cq_rows_max = 0;   // the largest band of cq.g2, in entries (what its generator's launch is sized by)
    // the tables' bytes as they are asked for (not the pool's block sizes): every upload and every device-generated table adds
    // its own while the plan is built; the cache's budget is charged in this
    size_t bytes = 0;
    uint64_t last_use = 0; // for the least-recently-used eviction in get_plan
    ~DevPlan(); // (gives its blocks back to the handle's pool)
};

struct PlanTiming; // (plans.hip)

enum KernelKind { K_ROWS = 0, K_COLS, K_CQ, K_DB, K_PROJECT, K_PACK, K_SCAN, K_TOPK, K_PAIRS, K_FWD, K_COUNT };

struct TimedLaunch {
    int kind;
    Event a, b;
};

// the first HIP failure met by a destructor (Timed, a fan-out's join) during the call in progress (ordered_call)
struct CallStatus {
    int rc = 0;
    std::string msg;
};

struct hpfw_gpu {
    int device = 0;
    bool has_filters = false;
    std::vector<float> filters; // the filters as they were installed (hpfw_gpu_get_filters)
    DevBuf d_fpack;
    DevBuf d_fq_image; // the filters' fixed-point digits (k_project_q.hip)
    // the six-product split of the unshifted fixed-point extraction (k_project_q.hip): the rows' thresholds; the
    // tiles' counts of open values of a launch; the tiles of the last launch (hpfw_gpu_debug_q_products).
    // HPFW_Q_PRODUCTS=9 in the environment at creation: the nine-product kernel alone.
    DevBuf d_q_thr, d_q_split;
    int q_products = 6;
    int64_t q_last_tiles = 0;
    int projection = 1; // 1: fixed point (S9q), 0: the f32 fma chain (S9); hpfw_gpu_set_projection
    // the tables of every clip length in use and the device memory they come from (plans.hip)
    struct PlanCache {
        PlanCache(); // (both in plans.hip, where PlanTiming is known; the destructor prints its report)
        ~PlanCache();
        // free chunks and blocks of evicted plans, by size (declared before `plans`: a plan gives its blocks back when it goes)
        std::multimap<size_t, DevBuf> dev_pool;
        size_t dev_pool_bytes = 0;
        std::map<int64_t, std::unique_ptr<DevPlan>> plans; // one per clip length, least recently used evicted
        // host halves of plans prepared ahead by other threads (hpfw_gpu_prepare_length): a null entry is being built
        std::mutex host_mtx;
        std::condition_variable host_cv;
        std::map<int64_t, std::unique_ptr<hpfw::HostPlan>> host_ready;
        std::set<int64_t> host_seen; // lengths being prepared, prepared, or resident on the device (not prepared again while they are)
        size_t plan_bytes = 0;
        uint64_t plan_clock = 0;
        // plans last used at or before this value of plan_clock are known to be idle: the caller has waited for all the work it
        // queued on this handle since (hpfw_internal_note_idle: the file collectors, once per window of files) -- such plans
        // are evicted without the device-wide wait that an eviction otherwise needs
        uint64_t idle_clock = 0;
        std::unique_ptr<PlanTiming> plan_timing; // HPFW_PLAN_TIMING
        // The tables of a new clip length go to the device on a stream of the handle's own, from a pinned ring, without a host
        // wait (the stream that first uses them waits for plan_ev): synchronous copies on the default stream waited behind
        // whatever shared its hardware queue -- after bench.py's host-buffer section that was the collector's extraction stream,
        // and a corpus of distinct lengths lost a fifth of its rate (tools/ffi_interaction.sh)
        Stream plan_stream;
        HostBuf pin_ring;
        size_t pin_off = 0;
        // the tables a new length generates on the device (default stream) are awaited by the stream that first uses them
        // (ordered_call), not by the host: a caller on a stream of its own keeps preparing lengths while earlier files run
        Event plan_ev;
        bool plan_ev_pending = false;
    } cache;
    unsigned conventions = 0; // hpfw_gpu_set_conventions: essentia conventions that cannot be checked offline
    // clips per pass: 2.5 GB of workspace at 30 s; every launch but the forward transform's chunks fills the 256 CUs many
    // times over, and what one stage leaves for the next (forward bins, dB terms: 2.3 MB per clip) is still in the caches
    // when it is read (1000 clips: 10.25 ms in one pass, 10.0 in four)
    int batch = 256;
    // extraction workspace: yp, x, mag, proj, wave maxima [clip][121][16], pairs, second planar buffer of the chirp-z
    // forward transform
    DevBuf ws[7];
    // the index and the scratch of its searches (search.hip, votes.hip)
    struct Index {
        DevBuf d_db; // uint64 hashprints
        std::vector<int64_t> db_off{0};
        DevBuf d_db_off;
        bool db_off_dirty = true;
        uint32_t clip_base = 0;
        DevBuf d_best, d_q_off;
        DevBuf d_qa; // queries expanded to fp4 for the matrix-core scan
        DevBuf d_gk; // longest query of each group of 32
        DevBuf d_topk_scratch;
        DevBuf d_shift_hits; // the per-shift top-k lists of a transposed search
        DevBuf d_ov_tab, d_ov_exclude; // overlap search: the (query, clip, split) entries, the clips to skip
        // search within sets: the sets' slots and the regrouping tables of a call; its queries in the
        // order of their sets; their hits and moments in that order
        DevBuf d_within_tab, d_within_q, d_within_out;
        // self-join (selfjoin.hip): the (row, clip, split) entries of a pass, its rows' counts and first
        // positions, the passes' numbering of their (row group, clip) pairs; the local self-join (localjoin.hip, section 26)
        // keeps its own table, rows and numbering in the same three, and its count of disagreeing walks in d_local_flag
        DevBuf d_sj_tab, d_sj_rows, d_sj_pairs;
        DevBuf d_sj_x_off; // the join with recordings outside the index (section 23): their offsets
        // voting search on the device: the workspaces of one group of windows, carved from one buffer;
        // the first window and first hashprint of every query of the call
        DevBuf d_votes_ws, d_votes_tab;
        // warped search (dtw.hip): the queries' offsets, the caller's pairs, the boundary rows of the
        // workgroups, the pairs' hits, the top lists (the plain search's candidates, launch_topk's hits), a path's choices
        DevBuf d_dtw_q_off, d_dtw_pairs, d_dtw_bnd, d_dtw_hits, d_dtw_top, d_dtw_choices;
        // local search (local.hip): launch_topk's hits of a group of queries; the count of winners whose
        // walk disagreed with the scan
        DevBuf d_local_top, d_local_flag;
        // removal in place (k_index.hip): the staging buffer of one chunk; the moves of the last
        // removal on the device and the host copy their upload reads, which moves_ev says has been read
        DevBuf d_stage, d_moves;
        std::vector<hpfw_index_move> moves;
        Event moves_ev;
        bool moves_pending = false;
    } index;
    // filter learning (learn.hip)
    struct Learn {
        // accum_cov of ParallelCollector (parallel_collector.h:76), upper tiles only
        DevBuf d_cov;
        DevBuf d_cov_ws; // scratch of the covariance kernels
        DevBuf d_cov_tiles;
        int64_t cov_files = 0;
        // HashprintHandle configurations other than the default (hpfw_gpu_cfg_*): filter operand images by config
        std::map<std::vector<int>, DevBuf> cfg_fpack;
        DevBuf d_cfg_proj;
        struct CfgCov {
            DevBuf d_accum;
            DevBuf d_tiles;
            int64_t clips = 0;
        };
        std::map<std::vector<int>, CfgCov> cfg_cov; // accum_cov of other configurations, by (rows, context)
        DevBuf d_cfg_cov_ws;
    } learn;
    // Mel front-end (learn.hip): tables (owned by `owned`), workspaces
    struct Mel {
        bool ready = false;
        hpfw::HostPlan plan;
        hpfw::RowsArgs rows;
        const float *d_win = nullptr, *d_cpack = nullptr;
        std::vector<DevBuf> owned;
        DevBuf d_work, d_small;
    } mel;
    DevBuf d_cqwork; // chirp-z bands too long for the LDS (k_cq_big.hip)
    // the size classes of the chirp-z stage run side by side (run_front): their workgroups differ in LDS footprint and
    // one class alone leaves part of every CU's LDS and issue slots unused
    static constexpr int kCqSide = 4;
    Stream cq_side[kCqSide];
    Event cq_fork, cq_join[kCqSide];
    int cq_concurrent = 1; // HPFW_CQ_SERIAL=1 in the environment at creation: one class after the other on the caller's stream
    // The passes of a back-end group pipelined over the same lanes (extract.hip run_group_pipelined): the
    // forward chunks of pass p + 1 are queued behind the classes of pass p instead of behind their join and the per-pass
    // maximum, so they start under the tail of the largest class.  Pass p keeps its forward bins in X[p & 1] (two halves
    // of ws[1]); lane k's last chunk of pass p records pp_fwd[p & 1][k], its classes of pass p record pp_cq[p & 1][k].
    // Three lanes are in use, because a process has four hardware queues and streams that share one run one after the
    // other (the five streams of the class fork sit on three queues): the largest class alone on lane fwd_streams
    // (cq_side[fwd_streams - 1]), which carries no chunks, the second largest ahead of the chunks of the last forward lane, the others on the
    // caller's stream.  HPFW_PASS_PIPELINE=0 in the environment at creation: every pass joined, as run_front does.
    // HPFW_PASS_PLAN="<lane of each class, largest first>:<lanes of the chunks in turn>" (timing, tests): another plan,
    // lane 0 the caller's stream, lane k cq_side[k - 1]; "23401:01" spreads the classes over all five lanes
    Event pp_fwd[2][kCqSide + 1], pp_cq[2][kCqSide + 1];
    int pass_pipeline = 1;
    std::vector<int> pp_class_lane, pp_turns;
    // the forward transform of a large batch in chunks of fwd_chunk clips taken in turn by fwd_streams streams (the
    // caller's and side streams): column stage and row stage of a chunk back to back, so that the column stage's output
    // (5.3 MB per clip) is read back out of the Infinity Cache instead of HBM.  HPFW_FWD_CHUNK (0: one launch per stage
    // for the whole batch), HPFW_FWD_STREAMS (1..5) in the environment at creation
    int fwd_chunk = 16, fwd_streams = 2;
    int cols_variant = 0; // HPFW_COLS_VARIANT (tests, diagnosis): kernels.h ColsQArgs::variant
    // HPFW_PRUNE (tests, timing), a bit mask of what the transforms leave out because nothing reads it: 1 = the row stage's last-group
    // outputs outside the consumed windows (fft_rows.h LastEdges, where the plan finds that they fit); 0: the kernels without it
    unsigned prune = 1;
    bool db_fast = true;  // HPFW_DB_TERM=spec (tests, timing) clears it: dB terms by the specified sequence alone (db_spec.h)
    int bz_chunk = 32;  // the same for the chirp-z forward transform's three kernels (HPFW_BZ_CHUNK; 38.6 -> 39.6 k clips/s at 30 s)
    // staging of the host-buffer entry points: kept between calls (a one-file call is otherwise mostly
    // allocation and stream set-up)
    DevBuf stage_pcm[2];
    DevBuf stage_hp;
    Stream stage_copy, stage_comp;
    Event stage_copied[2], stage_consumed[2];
    DevBuf d_clipmax; // per-clip maximum magnitude (reference level of the dB conversion)
    // ordering of consecutive entry points that were handed different streams (the workspaces are shared): the stream of
    // the last call, and whether order_ev marks the end of its work (else the next call on another stream waits for that
    // stream on the host)
    Event order_ev;
    hipStream_t order_stream = nullptr;
    enum { kOrderNone, kOrderEvent, kOrderSync } order = kOrderNone;
    CallStatus call; // what Timed and the fan-outs of the call in progress report (ordered_call)
    // timing
    Event ev0, ev1;
    unsigned timing_mask = 0;
    std::vector<TimedLaunch> timed;
    std::vector<std::pair<Event, Event>> ev_pool;
    float k_ms[K_COUNT] = {0};
    int k_launches[K_COUNT] = {0};
    // AudioCombiner's inverted index (k_combiner.hip), created on first use
    std::unique_ptr<hpfw::Combiner> combiner;
    // exact cross-correlation (k_xcorr.hip, combiner.hip): the jobs and their parts on the device, r when the caller keeps none
    struct Xcorr {
        DevBuf d_tab, d_r;
    } xcorr;
    // sample-rate conversion (k_resample.hip, extract.hip): the device image of each rate's table, made on first use;
    // staging of the host entry point
    struct Resample {
        struct Table {
            int32_t L = 0, M = 0, T = 0;
            DevBuf d_taps;
        };
        std::map<int, Table> tables;
        DevBuf in, out;
    } rs;
    // time warp and mix (k_warp.hip, warp.hip): the device image of the table, made on first use; the tracks of the call in
    // progress with their reach
    struct Warp {
        DevBuf d_taps, d_tracks;
    } warp;
    // transposed queries (k_project_q.hip): the filter images of the shift list last used (cleared
    // with the filters)
    DevBuf d_shift_images;
    std::vector<int32_t> shift_images_of;
    // queries at another tempo (k_tempo.hip): the time-scaled dB spectrograms of a sub-batch of
    // (clip, tempo) pairs (kTempoBudget, or one pair where a pair is larger)
    DevBuf d_tempo;
    // windows of one recording (k_windows.hip): the windows of a pass gathered into clips back to back
    DevBuf d_windows;
};

// a workspace of at least `need` bytes (its contents are not kept when it grows)
int ensure(DevBuf &b, size_t need, hpfw_gpu *pool_owner = nullptr);

// Every entry point of a handle works in the handle's shared workspaces (ws[], d_clipmax, d_best, d_qa, the
// index itself ...) and only enqueues on the caller's stream.  Two calls on different streams (a torch
// side stream and the null stream, or the private non-blocking streams of the *_host entry points) would
// otherwise overlap on those buffers: each call first makes its stream wait for the event the previous
// call recorded, and records its own when it has enqueued its work.  A call whose record failed leaves no
// event: the next call on another stream waits for its stream on the host.
// ordered_call(h, s, body) returns body's status, else the first failure Timed or a fan-out's join reported
// during it, else the record's.  A failed wait returns before anything is queued.
inline int report(hpfw_gpu *h, hipError_t e, const char *what)
{
    if (e != hipSuccess && !h->call.rc) h->call = {HPFW_E_HIP, std::string(what) + ": " + hipGetErrorString(e)};
    return e != hipSuccess;
}

template <class Body>
int ordered_call(hpfw_gpu *h, hipStream_t s, Body &&body)
{
    if (h->order_stream != s) {
        if (h->order == hpfw_gpu::kOrderEvent) HIP_TRY(hipStreamWaitEvent(s, h->order_ev.get(), 0));
        if (h->order == hpfw_gpu::kOrderSync) HIP_TRY(hipStreamSynchronize(h->order_stream));
    }
    if (h->cache.plan_ev_pending) {
        HIP_TRY(hipStreamWaitEvent(s, h->cache.plan_ev.get(), 0));
        h->cache.plan_ev_pending = false; // (later calls on other streams are ordered after this one)
    }
    CallStatus outer = std::exchange(h->call, CallStatus{}); // (a call made inside another's body)
    int rc = body();
    const hipError_t recorded = hipEventRecord(h->order_ev.get(), s);
    h->order_stream = s;
    h->order = recorded == hipSuccess ? hpfw_gpu::kOrderEvent : hpfw_gpu::kOrderSync;
    CallStatus mine = std::exchange(h->call, std::move(outer));
    if (!rc && mine.rc) rc = fail(mine.rc, mine.msg);
    if (!rc && recorded != hipSuccess) rc = fail(HPFW_E_HIP, std::string("hipEventRecord: ") + hipGetErrorString(recorded));
    return rc;
}

// the span of the launches in its scope, when h->timing_mask selects `kind`
struct Timed {
    hpfw_gpu *h;
    int kind;
    hipStream_t s;
    bool on = false;
    Event a, b;
    Timed(hpfw_gpu *h_, int kind_, hipStream_t s_) : h(h_), kind(kind_), s(s_)
    {
        if (!((h->timing_mask >> kind) & 1u)) return;
        if (h->ev_pool.empty()) {
            if (report(h, a.create(hipEventDefault), "timing event") || report(h, b.create(hipEventDefault), "timing event")) return;
        } else {
            a = std::move(h->ev_pool.back().first);
            b = std::move(h->ev_pool.back().second);
            h->ev_pool.pop_back();
        }
        on = !report(h, hipEventRecord(a.get(), s), "timing event record");
    }
    ~Timed()
    {
        if (on && !report(h, hipEventRecord(b.get(), s), "timing event record")) h->timed.push_back({kind, std::move(a), std::move(b)});
    }
};

inline int check_launch(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(HPFW_E_HIP, std::string("launch of ") + what + ": " + hipGetErrorString(e));
    return 0;
}

// The device side of an entry point on host buffers (the null stream): take() allocates a buffer, uploads its input or
// sets its bytes, and names the host buffer it goes back to; run() makes the call, waits for the whole device if asked,
// and downloads (blocking copies).  Every step after a failure does nothing; the buffers are freed on every exit.  A failed
// allocation is HPFW_E_NOMEM.
struct HostTrip {
    int rc = 0;
    std::vector<std::pair<DevBuf, void *>> bufs; // (device buffer, host destination or null)
    // `bytes` of device memory: a copy of host `src` when given, else every byte `fill` when fill >= 0
    template <class T>
    T *take(size_t bytes, const void *src = nullptr, int fill = -1, void *dst = nullptr)
    {
        DevBuf &b = bufs.emplace_back(DevBuf(), dst).first;
        if (!rc && b.alloc(bytes) != hipSuccess) rc = fail(HPFW_E_NOMEM, "hipMalloc failed");
        if (!rc && ((src && hipMemcpy(b.get(), src, bytes, hipMemcpyHostToDevice) != hipSuccess) ||
                    (fill >= 0 && hipMemset(b.get(), fill, bytes) != hipSuccess)))
            rc = fail(HPFW_E_HIP, "H2D copy failed");
        return b.as<T>();
    }
    template <class Call>
    int run(bool wait, Call call)
    {
        if (!rc) rc = call();
        if (!rc && wait && hipDeviceSynchronize() != hipSuccess) rc = fail(HPFW_E_HIP, "kernel execution failed");
        for (auto &[b, dst] : bufs)
            if (!rc && dst && hipMemcpy(dst, b.get(), b.capacity(), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(HPFW_E_HIP, "D2H copy failed");
        return rc;
    }
};

// the host round trip of a search: the hashprints (elements Q) of query sets [0, n_sets) uploaded, their offsets rebased
// to 0, device(d_q, rel, d_out) queued on the null stream, the n_out hits it wrote downloaded
// (scored searches: the n_stats rows of moments the call wrote downloaded as well, device(d_q, rel, d_out, d_stats))
template <class Q, class Hit, class Device>
int search_round_trip_scored(const Q *q_hp, const int64_t *q_off, int64_t n_sets, int64_t n_out, Hit *out, int64_t n_stats,
                             hpfw_dist_stats *stats, Device device)
{
    const int64_t total = q_off[n_sets] - q_off[0];
    if (total < 0) return fail(HPFW_E_INVALID, "q_off must be non-decreasing");
    if (total && !q_hp) return fail(HPFW_E_INVALID, "null queries");
    std::vector<int64_t> rel((size_t)n_sets + 1);
    for (int64_t i = 0; i <= n_sets; ++i) rel[(size_t)i] = q_off[i] - q_off[0];
    HostTrip t;
    const Q *d_q = t.take<Q>((size_t)std::max<int64_t>(total, 1) * sizeof(Q), total ? q_hp + q_off[0] : nullptr);
    Hit *d_out = t.take<Hit>((size_t)n_out * sizeof(Hit), nullptr, -1, out);
    hpfw_dist_stats *d_stats = n_stats ? t.take<hpfw_dist_stats>((size_t)n_stats * sizeof(hpfw_dist_stats), nullptr, -1, stats) : nullptr;
    return t.run(true, [&] { return device(d_q, rel.data(), d_out, d_stats); });
}

template <class Q, class Hit, class Device>
int search_round_trip(const Q *q_hp, const int64_t *q_off, int64_t n_sets, int64_t n_out, Hit *out, Device device)
{
    return search_round_trip_scored(q_hp, q_off, n_sets, n_out, out, 0, nullptr,
                                    [&](const Q *d_q, const int64_t *rel, Hit *d_out, hpfw_dist_stats *) { return device(d_q, rel, d_out); });
}

// the index's offsets to the device when they changed since the last upload: on s, which the host then waits for
inline int upload_db_off(hpfw_gpu *h, hipStream_t s)
{
    if (!h->index.db_off_dirty) return 0;
    if (int rc = ensure(h->index.d_db_off, h->index.db_off.size() * 8)) return rc;
    HIP_TRY(hipMemcpyAsync(h->index.d_db_off.get(), h->index.db_off.data(), h->index.db_off.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    h->index.db_off_dirty = false;
    return 0;
}

// the hashprints of the index's longest clip
inline int64_t index_longest_clip(const hpfw_gpu *h)
{
    int64_t n_max = 0;
    for (size_t i = 0; i + 1 < h->index.db_off.size(); ++i) n_max = std::max(n_max, h->index.db_off[i + 1] - h->index.db_off[i]);
    return n_max;
}

// what hpfw::overlap_splits and hpfw::join_plan (join_plan.h) take as forced_splits and table_kb: the value of the
// variable, or "not set"
inline int64_t env_forced_splits(const char *env_name)
{
    const char *e = std::getenv(env_name);
    return e ? std::min<int64_t>(std::max(std::atoi(e), 1), 64) : 0;
}
inline int64_t env_table_kb(const char *env_name)
{
    const char *e = std::getenv(env_name);
    return e ? std::max<int64_t>(std::atoll(e), 0) : -1;
}

// the offsets of n_q queries: in order, no query longer than 16000 hashprints; *k_max: the longest.  A call with both faults is
// told of the order, or with in_turn (the search within sets) of the fault of its first faulty query
inline int check_q_off(const int64_t *q_off, int64_t n_q, int64_t *k_max, bool in_turn = false)
{
    *k_max = 0;
    for (int64_t i = 0; i < n_q; ++i) {
        if (q_off[i + 1] < q_off[i]) return fail(HPFW_E_INVALID, "q_off must be non-decreasing");
        *k_max = std::max(*k_max, q_off[i + 1] - q_off[i]);
        if (in_turn && *k_max > 16000) break;
    }
    if (*k_max > 16000) return fail(HPFW_E_UNSUPPORTED, "query longer than 16000 hashprints");
    return 0;
}

// the k smallest keys of each of ng rows of d_table [ng][n_clips] -> d_out [ng][k] (hpfw_hit).  One workgroup per query would
// crawl through the whole table of a large index for a few queries: those go in two steps, through d_topk_scratch
inline int search_topk_rows(hpfw_gpu *h, const uint64_t *d_table, int ng, int64_t n_clips, int k, void *d_out, hipStream_t s,
                            const int32_t *d_set = nullptr)
{
    if (n_clips >= 16384 && ng <= 64) {
        if (int rc = ensure(h->index.d_topk_scratch, hpfw::topk_scratch_bytes(ng, k))) return rc;
        hpfw::launch_topk_two_step(d_table, ng, (int)n_clips, k, h->index.clip_base, h->index.d_topk_scratch.get(), d_out, s, d_set);
    } else {
        hpfw::launch_topk(d_table, ng, (int)n_clips, k, h->index.clip_base, d_out, s, d_set);
    }
    return 0;
}

// search.hip: the passes of a search over its queries, inside ordered_call (the plain, overlap and local searches; the group
// size is search_plan.h's).  The index's and the queries' offsets go to the device, and with `expand` (the matrix-core scans)
// d_qa is sized for a pass and the lengths of every group of 32 queries of the call go to d_gk, once.  Every pass of at most
// qgroup queries (a multiple of 32) presets its ng rows of row_bytes in `table` to 0xff, then runs the steps in turn, each
// under its kind's timer and its launches checked under its label; with `expand` the pass's image of the queries is
// made ahead of the step marked `scan`, under its timer.
struct QueryGroup {
    int64_t g0;             // the pass's first query
    int ng;                 // and how many it has
    const int64_t *d_q_off; // [ng + 1] (device), the pass's first query at d_q_off[0]
    const void *d_qa;       // with expand: launch_expand_queries' image of the pass, kt_pad rows per group of 32 ...
    int kt_pad;
    const int *d_gk;        // ... and [2 per group] the group's longest query and its shortest non-empty one
    int k_min;              // with expand: the pass's shortest non-empty query (0: none)
};
struct SearchStep {
    int kind; // K_SCAN, K_TOPK
    const char *what;
    bool scan; // the scan: it reads the pass's image of the queries
    std::function<int(const QueryGroup &)> run;
};
int search_run_groups(hpfw_gpu *h, hipStream_t s, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int64_t k_max, int64_t qgroup,
                      bool expand, DevBuf &table, size_t row_bytes, const std::vector<SearchStep> &steps);

// selfjoin.hip: the passes of a join, inside ordered_call.  pair_first goes to d_sj_pairs, and the stream is waited for
// once (whatever else the caller enqueued from host memory has been read); d_sj_tab and d_sj_rows are sized for a pass of
// entry_bytes entries; every pass with pairs presets its table to 0xff, then runs scan under K_SCAN and select under
// K_TOPK, each launch checked under its label
struct JoinPass {
    int g0, n_groups;            // its row groups
    const uint32_t *d_pair_first;
    uint32_t n_pairs;            // > 0
    int splits;
    void *d_tab;
    int *d_row_count;            // [32 n_groups]
    int64_t *d_row_first;
};
int join_run_passes(hpfw_gpu *h, hipStream_t s, const hpfw::JoinPlan &plan, int64_t n_groups, int64_t n_cols, size_t entry_bytes,
                    const char *scan_what, const std::function<void(const JoinPass &)> &scan, const char *select_what,
                    const std::function<void(const JoinPass &)> &select);

// plans.hip
int get_plan(hpfw_gpu *h, int64_t n, DevPlan **out);
hipError_t init_plans(hpfw_gpu *h); // the table stream and event, HPFW_PLAN_TIMING (at the handle's creation)
void clear_plans(hpfw_gpu *h);      // every length's tables and host half (no work may be using them)
// extract.hip
// what launch_hashprints_q takes as `split` for n_clips clips of c columns: the handle's split with its workspace, or NULL
// where the call runs the nine-product kernel (shifted images, HPFW_Q_PRODUCTS=9)
int q_split(hpfw_gpu *h, int n_shifts, int64_t n_clips, int64_t c, hpfw::QSplit *qs, const hpfw::QSplit **use);
int pass_clips(hpfw_gpu *h, const DevPlan *dp, int64_t n_clips);
int ensure_ws(hpfw_gpu *h, const DevPlan *dp, int nb, int ns, int x_bufs = 1); // x_bufs: forward-bin buffers of nb clips in ws[1]
int run_front(hpfw_gpu *h, DevPlan *dp, const int16_t *d_pcm, int nb, int slot, bool finish_db, hipStream_t s);
// the device image of the table of `rate` (not 44 100 Hz, inside the range), made and cached on first use; the device is set
int rs_table(hpfw_gpu *h, int rate, hpfw_gpu::Resample::Table **out);

