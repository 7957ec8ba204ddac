// search.hip -- the index of hashprints, its top-k, transposed and overlap searches, the top-k searches within sets of
// clips, and the merges of the shards' hits and moments.  (The voting search is votes.hip, AudioCombiner's calls are combiner.hip.)
#include "handle.h"

// the passes of a search over its queries (handle.h)
int search_run_groups(hpfw_gpu *h, hipStream_t s, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int64_t k_max, int64_t qgroup,
                      bool expand, DevBuf &table, size_t row_bytes, const std::vector<SearchStep> &steps)
{
    int rc;
    if ((rc = upload_db_off(h, s))) return rc;
    if ((rc = ensure(h->index.d_q_off, (size_t)(n_q + 1) * 8))) return rc;
    HIP_TRY(hipMemcpyAsync(h->index.d_q_off.get(), q_off, (size_t)(n_q + 1) * 8, hipMemcpyHostToDevice, s));
    if ((rc = ensure(table, (size_t)qgroup * row_bytes))) return rc;
    const int kt_pad = hpfw::hamming_mfma_kt_pad((int)k_max);
    std::vector<int> gk;
    if (expand) {
        if ((rc = ensure(h->index.d_qa, (size_t)(qgroup / 32) * kt_pad * 1024))) return rc;
        gk = hpfw::search_group_lengths(q_off, n_q);
        if ((rc = ensure(h->index.d_gk, gk.size() * 4))) return rc;
        HIP_TRY(hipMemcpyAsync(h->index.d_gk.get(), gk.data(), gk.size() * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s)); // (gk has been read)
    }
    for (int64_t g0 = 0; g0 < n_q; g0 += qgroup) {
        QueryGroup g = {};
        g.g0 = g0;
        g.ng = (int)std::min<int64_t>(qgroup, n_q - g0);
        g.d_q_off = h->index.d_q_off.as<int64_t>() + g0;
        if (expand) {
            g.d_qa = h->index.d_qa.get();
            g.kt_pad = kt_pad;
            g.d_gk = h->index.d_gk.as<int>() + g0 / 32 * 2;
            g.k_min = hpfw::search_shortest_query(gk, g0 / 32, (g0 + g.ng + 31) / 32);
        }
        HIP_TRY(hipMemsetAsync(table.get(), 0xff, (size_t)g.ng * row_bytes, s));
        for (const SearchStep &step : steps) {
            {
                Timed t(h, step.kind, s);
                if (expand && step.scan) hpfw::launch_expand_queries(d_q_hp, g.d_q_off, g.ng, kt_pad, h->index.d_qa.get(), s);
                rc = step.run(g);
            }
            if (rc || (rc = check_launch(step.what))) return rc;
        }
    }
    return 0;
}

extern "C" {

// ---- index + search ----------------------------------------------------------------------------
int hpfw_gpu_index_clear(hpfw_gpu *h)
{
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    h->index.db_off.assign(1, 0);
    h->index.db_off_dirty = true;
    return 0;
}

// the index's hashprints into a buffer of `bytes` (more than the capacity)
static int index_regrow(hpfw_gpu *h, size_t bytes)
{
    const int64_t have = h->index.db_off.back();
    DevBuf nd;
    HIP_TRY(nd.alloc(bytes));
    // earlier appends may still be in flight on a non-blocking stream the null-stream copy below would
    // not wait for, and scans may still be reading the old buffer: growing is rare (capacity doubles, or
    // hpfw_gpu_index_reserve sizes the buffer once)
    HIP_TRY(hipDeviceSynchronize());
    if (have) HIP_TRY(hipMemcpy(nd.get(), h->index.d_db.get(), (size_t)have * 8, hipMemcpyDeviceToDevice));
    h->index.d_db = std::move(nd); // (the old buffer goes with nd)
    return 0;
}

static int index_add_impl(hpfw_gpu *h, const uint64_t *hp, const int64_t *offsets, int64_t n_clips, bool dev,
                          hipStream_t s)
{
    if (!h || !hp || !offsets || n_clips < 0) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    for (int64_t i = 0; i < n_clips; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(HPFW_E_INVALID, "offsets must be non-decreasing");
    const int64_t add = offsets[n_clips] - offsets[0];
    const int64_t have = h->index.db_off.back();
    return ordered_call(h, s, [&] {
        const size_t need = (size_t)(have + add) * 8;
        if (need > h->index.d_db.capacity())
            if (int rc = index_regrow(h, std::max({need, h->index.d_db.capacity() * 2, (size_t)8 << 16}))) return rc;
        uint64_t *dst = h->index.d_db.as<uint64_t>() + have;
        if (add) {
            if (dev)
                HIP_TRY(hipMemcpyAsync(dst, hp + offsets[0], (size_t)add * 8, hipMemcpyDeviceToDevice, s));
            else
                HIP_TRY(hipMemcpy(dst, hp + offsets[0], (size_t)add * 8, hipMemcpyHostToDevice));
        }
        for (int64_t i = 0; i < n_clips; ++i) h->index.db_off.push_back(have + (offsets[i + 1] - offsets[0]));
        h->index.db_off_dirty = true;
        return 0;
    });
}

int hpfw_gpu_index_add(hpfw_gpu *h, const uint64_t *hp, const int64_t *offsets, int64_t n_clips)
{
    return index_add_impl(h, hp, offsets, n_clips, false, nullptr);
}

int hpfw_gpu_index_add_device(hpfw_gpu *h, const uint64_t *d_hp, const int64_t *offsets, int64_t n_clips,
                              void *stream)
{
    return index_add_impl(h, d_hp, offsets, n_clips, true, (hipStream_t)stream);
}

int64_t hpfw_gpu_index_size(hpfw_gpu *h) { return h ? (int64_t)h->index.db_off.size() - 1 : 0; }

// the index back on the host (MemoryStorage::save, storage.h:67-75, dumps the whole db):
// offsets [n_clips + 1] always; hp [offsets[n_clips]] when hp != NULL and hp_cap is large enough
int hpfw_gpu_index_get(hpfw_gpu *h, int64_t *offsets, uint64_t *hp, int64_t hp_cap)
{
    if (!h || !offsets) return fail(HPFW_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    std::memcpy(offsets, h->index.db_off.data(), h->index.db_off.size() * sizeof(int64_t));
    if (!hp) return 0;
    const int64_t total = h->index.db_off.back();
    if (hp_cap < total) return fail(HPFW_E_INVALID, "hashprint buffer too small for the index");
    if (total) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(hp, h->index.d_db.get(), (size_t)total * 8, hipMemcpyDeviceToHost));
    }
    return 0;
}

int hpfw_gpu_index_set_clip_base(hpfw_gpu *h, uint32_t base)
{
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    h->index.clip_base = base;
    return 0;
}

// ---- removal in place (the plan and its order: index_plan.h, the kernels: k_index.hip) ----
// hashprints of a chunk: HPFW_INDEX_STAGE_KB (tests), HPFW_INDEX_STAGE_MB, else the default; read at every call
static int64_t index_chunk()
{
    for (const auto &[name, unit] : {std::pair<const char *, int64_t>{"HPFW_INDEX_STAGE_KB", 1024}, {"HPFW_INDEX_STAGE_MB", (int64_t)1 << 20}}) {
        const char *e = std::getenv(name);
        if (!e || !*e) continue;
        const long long v = std::atoll(e);
        if (v >= 1 && v <= ((long long)1 << 20)) return std::max<int64_t>((int64_t)v * unit / 8, 1);
    }
    return hpfw::kIndexChunkDefault;
}

int hpfw_gpu_index_remove(hpfw_gpu *h, const int64_t *clips, int64_t n, void *stream)
{
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    if (n < 0) return fail(HPFW_E_INVALID, "n must not be negative");
    if (n > 0 && !clips) return fail(HPFW_E_INVALID, "null clips");
    const int64_t n_clips = (int64_t)h->index.db_off.size() - 1;
    for (int64_t i = 0; i < n; ++i)
        if (clips[i] < 0 || clips[i] >= n_clips)
            return fail(HPFW_E_INVALID, "index_remove: clip " + std::to_string(clips[i]) + " outside [0, " + std::to_string(n_clips) + ")");
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int64_t> ids(clips, clips + n);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const int64_t chunk = index_chunk();
    std::vector<int64_t> new_off(h->index.db_off.size());
    std::vector<hpfw_index_move> moves;
    if (!hpfw::index_remove_plan(h->index.db_off.data(), n_clips, ids.data(), (int64_t)ids.size(), chunk, new_off.data(), &moves))
        return fail(HPFW_E_INVALID, "index_remove: no plan");
    if (new_off == h->index.db_off) return 0; // (every clip named was empty)
    HIP_TRY(hipSetDevice(h->device));
    // everything that can be refused is refused here, while the index is as it was
    bool staged = false;
    for (const hpfw_index_move &m : moves) staged = staged || m.staged;
    const size_t stage_bytes = (size_t)(chunk + 2) * 8; // (a chunk that begins at an odd hashprint waits one word in)
    if (staged && h->index.d_stage.capacity() < stage_bytes && h->index.d_stage.alloc(stage_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(HPFW_E_INVALID, "index_remove: no staging buffer of " + std::to_string(stage_bytes) + " bytes (HPFW_INDEX_STAGE_MB)");
    }
    if (!moves.empty()) {
        if (h->index.d_moves.capacity() < moves.size() * sizeof(hpfw_index_move) &&
            h->index.d_moves.alloc(std::max(moves.size() * sizeof(hpfw_index_move) * 2, (size_t)1 << 16)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(HPFW_E_INVALID, "index_remove: no device memory for the moves");
        }
        if (!h->index.moves_ev && h->index.moves_ev.create() != hipSuccess) return fail(HPFW_E_HIP, "index_remove: event");
        // the upload of the removal before may still be reading the host copy this one replaces
        if (h->index.moves_pending) HIP_TRY(hipEventSynchronize(h->index.moves_ev.get()));
        h->index.moves_pending = false;
    }
    return ordered_call(h, s, [&] {
        uint64_t *db = h->index.d_db.as<uint64_t>();
        if (!moves.empty()) {
            h->index.moves = std::move(moves);
            const std::vector<hpfw_index_move> &mv = h->index.moves;
            const hpfw_index_move *d_mv = h->index.d_moves.as<hpfw_index_move>();
            HIP_TRY(hipMemcpyAsync(h->index.d_moves.get(), mv.data(), mv.size() * sizeof(hpfw_index_move), hipMemcpyHostToDevice, s));
            h->index.moves_pending = hipEventRecord(h->index.moves_ev.get(), s) == hipSuccess;
            if (!h->index.moves_pending) HIP_TRY(hipStreamSynchronize(s));
            for (size_t i = 0; i < mv.size();) { // chunk after chunk, in launch order
                size_t j = i;
                while (j < mv.size() && mv[j].chunk == mv[i].chunk) ++j;
                const int64_t lo = mv[i].dst, hi = mv[j - 1].dst + mv[j - 1].len;
                if (mv[i].staged) {
                    uint64_t *stage = h->index.d_stage.as<uint64_t>();
                    const int64_t base = lo & ~(int64_t)1;
                    hpfw::launch_index_gather(stage, base, db, d_mv + i, (int64_t)(j - i), lo, hi, s);
                    hpfw::launch_index_copy(db, stage, base, lo, hi, s);
                } else {
                    hpfw::launch_index_gather(db, 0, db, d_mv + i, (int64_t)(j - i), lo, hi, s);
                }
                i = j;
            }
            if (int rc = check_launch("index_remove")) return rc;
        }
        h->index.db_off = std::move(new_off);
        h->index.db_off_dirty = true;
        return 0;
    });
}

int hpfw_gpu_index_reserve(hpfw_gpu *h, int64_t n_hashprints)
{
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    if (n_hashprints < 0 || n_hashprints > ((int64_t)1 << 58)) return fail(HPFW_E_INVALID, "index_reserve: n_hashprints outside 0 .. 2^58");
    if ((size_t)n_hashprints * 8 <= h->index.d_db.capacity()) return 0;
    HIP_TRY(hipSetDevice(h->device));
    return ordered_call(h, nullptr, [&] { return index_regrow(h, (size_t)n_hashprints * 8); });
}

int64_t hpfw_gpu_index_capacity(hpfw_gpu *h) { return h ? (int64_t)(h->index.d_db.capacity() / 8) : 0; }

int hpfw_gpu_index_remove_plan(const int64_t *offsets, int64_t n_clips, const int64_t *removed, int64_t n_removed, int64_t chunk,
                               int64_t *new_offsets, hpfw_index_move *moves, int64_t moves_cap, int64_t *n_moves)
{
    if (!offsets || !new_offsets || !n_moves) return fail(HPFW_E_INVALID, "null argument");
    std::vector<hpfw_index_move> mv;
    if (!hpfw::index_remove_plan(offsets, n_clips, removed, n_removed, chunk, new_offsets, &mv))
        return fail(HPFW_E_INVALID, "index_remove_plan: offsets must not decrease, removed must ascend strictly inside [0, n_clips), chunk >= 1");
    *n_moves = (int64_t)mv.size();
    if (!moves) return 0;
    if (moves_cap < *n_moves) return fail(HPFW_E_INVALID, "index_remove_plan: moves_cap below the number of pieces");
    std::copy(mv.begin(), mv.end(), moves);
    return 0;
}

int hpfw_gpu_index_remove_geometry(int64_t *tile, int64_t *chunk)
{
    if (!tile || !chunk) return fail(HPFW_E_INVALID, "null argument");
    *tile = hpfw::kIndexTile;
    *chunk = hpfw::kIndexChunkDefault;
    return 0;
}

// the clips a search is about: every slot of the index (d_set NULL), or the slots of one set --
// n_clips of them, the longest of n_max hashprints, d_set [n_clips] on the device
struct ClipView {
    int64_t n_clips, n_max;
    const int32_t *d_set;
};

static ClipView whole_index(const hpfw_gpu *h) { return {(int64_t)h->index.db_off.size() - 1, index_longest_clip(h), nullptr}; }

// the top-k search of n_q queries over the clips of v (inside an ordered_call); d_stats: NULL, or [n_q] rows that receive
// the moments of the per-clip best distances (k_stats.hip: one more reader of the table the scan wrote)
static int search_topk_view(hpfw_gpu *h, const ClipView &v, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int k,
                            hpfw_hit *d_out, hpfw_dist_stats *d_stats, hipStream_t s)
{
    if (n_q == 0) return 0;
    if (!d_q_hp) return fail(HPFW_E_INVALID, "null queries");
    const int64_t n_clips = v.n_clips, n_max = v.n_max;
    if (d_stats) HIP_TRY(hipMemsetAsync(d_stats, 0, (size_t)n_q * sizeof(hpfw_dist_stats), s));
    if (n_clips == 0) { // nothing indexed: every slot is "none"
        hpfw::launch_topk(nullptr, (int)n_q, 0, k, h->index.clip_base, d_out, s);
        return check_launch("topk");
    }
    int64_t k_max = 0;
    if (int rc = check_q_off(q_off, n_q, &k_max)) return rc;
    // d <= 64 k_max: the sum of squares stays below 2^64 while n_clips k_max^2 4096 does
    if (d_stats && (unsigned __int128)n_clips * (uint64_t)(k_max * k_max) * 4096 >= ((unsigned __int128)1 << 64))
        return fail(HPFW_E_UNSUPPORTED, "scored search: n_clips * k_max^2 * 4096 must stay below 2^64");
    const int64_t qgroup = hpfw::search_group_queries(n_q, n_clips, hpfw::kSearchTableEntries, hpfw::kSearchGridQueries, 8,
                                                      env_table_kb("HPFW_SEARCH_TABLE_KB"));
    // search_plan.h's choice (HPFW_SEARCH_POPC); fewer than 8 queries go one by one through the shifted-rows variant
    // (HPFW_SEARCH_MFMA / HPFW_SEARCH_SHIFT force the grouped / the shifted-rows kernel for any number of queries).
    // A group of 32 queries is one MFMA tile: with fewer than 8 queries most of its rows would be padding
    // and the popcount kernel (one workgroup per 8 queries) does less work.
    const bool popc = std::getenv("HPFW_SEARCH_POPC") != nullptr;
    const bool mfma = hpfw::search_on_matrix_cores(popc, hpfw::hamming_mfma_lds_bytes((int)k_max)) && k_max > 0 &&
                      (n_q >= 8 || std::getenv("HPFW_SEARCH_MFMA"));
    const bool few = (!mfma || std::getenv("HPFW_SEARCH_SHIFT")) && !popc && k_max > 0 && n_max > 0 &&
                     hpfw::hamming_shift_lds_bytes((int)k_max) <= hpfw::kScanLdsLimit;
    const bool grouped = mfma && !few && n_max > 0;
    auto args = [&](const QueryGroup &g) {
        hpfw::SearchArgs a;
        a.db = h->index.d_db.as<uint64_t>();
        a.db_off = h->index.d_db_off.as<int64_t>();
        a.n_clips = (int)n_clips;
        a.q = d_q_hp;
        a.q_off = g.d_q_off;
        a.n_q = g.ng;
        a.k_max = (int)k_max;
        a.best = h->index.d_best.as<uint64_t>(); // (the runner has sized the table)
        a.set = v.d_set;
        return a;
    };
    std::vector<SearchStep> steps;
    steps.push_back({K_SCAN, "hamming_scan", true, [&](const QueryGroup &g) {
                         const hpfw::SearchArgs a = args(g);
                         if (few) { // a handful of queries: one launch each, the tile rows are shifts of the query
                             if (int rc = ensure(h->index.d_qa, hpfw::hamming_shift_image_bytes((int)k_max))) return rc;
                             for (int i = 0; i < g.ng; ++i) {
                                 const int kq = (int)(q_off[g.g0 + i + 1] - q_off[g.g0 + i]);
                                 if (kq <= 0) continue;
                                 hpfw::launch_hamming_shift(a.db, a.db_off, (int)n_clips, (int)std::max<int64_t>(n_max - std::min<int64_t>(kq, n_max) + 1, 1),
                                                            d_q_hp + q_off[g.g0 + i], kq, h->index.d_qa.get(), a.best + (size_t)i * n_clips, s, v.d_set);
                             }
                         } else if (grouped) {
                             // offsets exist up to n_max - (shortest query): that many chunks of workgroups per clip
                             hpfw::launch_hamming_mfma(a, g.d_qa, g.kt_pad, g.d_gk, (int)std::max<int64_t>(n_max - std::min<int64_t>(g.k_min, n_max) + 1, 1), s);
                         } else {
                             hpfw::launch_hamming_scan(a, s);
                         }
                         return 0;
                     }});
    steps.push_back({K_TOPK, "topk", false,
                     [&](const QueryGroup &g) { return search_topk_rows(h, h->index.d_best.as<uint64_t>(), g.ng, n_clips, k, d_out + g.g0 * k, s, v.d_set); }});
    if (d_stats)
        steps.push_back({K_TOPK, "dist_stats", false, [&](const QueryGroup &g) {
                             hpfw::launch_dist_stats(h->index.d_best.as<uint64_t>(), h->index.d_db_off.as<int64_t>(), g.d_q_off, g.ng, (int)n_clips, d_stats + g.g0, s, v.d_set);
                             return 0;
                         }});
    return search_run_groups(h, s, d_q_hp, q_off, n_q, k_max, qgroup, grouped, h->index.d_best, (size_t)n_clips * 8, steps);
}

static int search_topk_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int k, hpfw_hit *d_out,
                              hpfw_dist_stats *d_stats, hipStream_t s)
{
    if (!h || !q_off || !d_out || n_q < 0 || k < 1 || k > 64) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    return ordered_call(h, s, [&] { return search_topk_view(h, whole_index(h), d_q_hp, q_off, n_q, k, d_out, d_stats, s); });
}

int hpfw_gpu_search_topk_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int k,
                                hpfw_hit *d_out, void *stream)
{
    return search_topk_device(h, d_q_hp, q_off, n_q, k, d_out, nullptr, (hipStream_t)stream);
}

int hpfw_gpu_search_topk_scored_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int k, hpfw_hit *d_out,
                                       hpfw_dist_stats *d_stats, void *stream)
{
    if (!d_stats) return fail(HPFW_E_INVALID, "null stats");
    return search_topk_device(h, d_q_hp, q_off, n_q, k, d_out, d_stats, (hipStream_t)stream);
}

// host buffers: stats NULL (plain) or [n_q]
static int search_topk_host(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int k, hpfw_hit *out,
                            hpfw_dist_stats *stats)
{
    if (!h || !q_off || !out || n_q < 0) return fail(HPFW_E_INVALID, "bad argument");
    if (k < 1 || k > 64) return fail(HPFW_E_INVALID, "k must be in 1..64");
    HIP_TRY(hipSetDevice(h->device));
    if (n_q == 0) return 0;
    return search_round_trip_scored(q_hp, q_off, n_q, n_q * k, out, stats ? n_q : 0, stats,
                                    [&](const uint64_t *d_q, const int64_t *rel, hpfw_hit *d_out, hpfw_dist_stats *d_stats) {
                                        return search_topk_device(h, d_q, rel, n_q, k, d_out, d_stats, nullptr);
                                    });
}

int hpfw_gpu_search_topk(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int k,
                         hpfw_hit *out)
{
    return search_topk_host(h, q_hp, q_off, n_q, k, out, nullptr);
}

int hpfw_gpu_search_topk_scored(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int k, hpfw_hit *out,
                                hpfw_dist_stats *stats)
{
    if (!stats) return fail(HPFW_E_INVALID, "null stats");
    return search_topk_host(h, q_hp, q_off, n_q, k, out, stats);
}

// ---- search within sets (the rule: include/hpfw_gpu.h) ---------------------------------------
// what can be refused without the handle's contents, before a device is touched; q_set has one entry per n_rep queries
static int within_check(const void *h, const int64_t *q_off, int64_t n_q, int k, const int64_t *set_off, int64_t n_sets,
                        const int32_t *set_clips, const int32_t *q_set, int n_rep, const void *out)
{
    if (!h || !q_off || !out || n_q < 0) return fail(HPFW_E_INVALID, "bad argument");
    if (k < 1 || k > 64) return fail(HPFW_E_INVALID, "k must be in 1..64");
    if (n_sets < 0) return fail(HPFW_E_INVALID, "within: n_sets must not be negative");
    if (n_sets > 0 && !set_off) return fail(HPFW_E_INVALID, "within: null set_off");
    if (n_sets > 0 && set_off[0] != 0) return fail(HPFW_E_INVALID, "within: set_off[0] must be 0");
    for (int64_t i = 0; i < n_sets; ++i)
        if (set_off[i + 1] < set_off[i]) return fail(HPFW_E_INVALID, "within: set_off must not decrease");
    if (n_sets > 0 && set_off[n_sets] > 0 && !set_clips) return fail(HPFW_E_INVALID, "within: null set_clips");
    for (int64_t i = 0; i < n_sets; ++i)
        for (int64_t p = set_off[i]; p < set_off[i + 1]; ++p)
            if (set_clips[p] < 0 || (p > set_off[i] && set_clips[p] <= set_clips[p - 1]))
                return fail(HPFW_E_INVALID, "within: set " + std::to_string(i) + " must hold clips >= 0 in strictly ascending order");
    if (!q_set) return fail(HPFW_E_INVALID, "within: null q_set");
    for (int64_t i = 0; i < n_q / n_rep; ++i)
        if (q_set[i] < -1 || q_set[i] >= n_sets)
            return fail(HPFW_E_INVALID, "within: q_set[" + std::to_string(i) + "] outside -1 .. n_sets - 1");
    int64_t k_max = 0;
    return check_q_off(q_off, n_q, &k_max, true);
}

// what the index decides, before a kernel runs
static int within_check_index(const hpfw_gpu *h, const int64_t *q_off, int64_t n_q, const int64_t *set_off, int64_t n_sets,
                              const int32_t *set_clips, const int32_t *q_set, int n_rep, bool scored)
{
    const int64_t n_slots = (int64_t)h->index.db_off.size() - 1;
    for (int64_t i = 0; i < n_sets; ++i) // (a set ascends: its last clip is its largest)
        if (set_off[i + 1] > set_off[i] && set_clips[set_off[i + 1] - 1] >= n_slots)
            return fail(HPFW_E_INVALID, "within: set " + std::to_string(i) + " names clip " + std::to_string(set_clips[set_off[i + 1] - 1]) +
                                            " of an index of " + std::to_string(n_slots));
    if (!scored) return 0;
    int64_t n = 0, k_max = 0; // the largest set a query names (the index for -1), the longest query
    for (int64_t i = 0; i < n_q; ++i) {
        const int32_t st = q_set[i / n_rep];
        n = std::max(n, st < 0 ? n_slots : set_off[st + 1] - set_off[st]);
        k_max = std::max(k_max, q_off[i + 1] - q_off[i]);
    }
    if ((unsigned __int128)n * (uint64_t)(k_max * k_max) * 4096 >= ((unsigned __int128)1 << 64))
        return fail(HPFW_E_UNSUPPORTED, "scored search: n_clips * k_max^2 * 4096 must stay below 2^64");
    return 0;
}

// The top-k search of n_q queries, query i within set q_set[i / n_rep] (-1: the whole index).  The queries are put in the
// order of their sets (stable), every set's range goes through search_topk_view over that set's slots -- its table is as wide
// as the set, its launches cover the set's clips and follow its longest clip -- and the rows of hits and moments are
// scattered back to the caller's order.  A call without a restricted query is the unrestricted call on the caller's buffers.
static int search_topk_within_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int k, const int64_t *set_off,
                                     int64_t n_sets, const int32_t *set_clips, const int32_t *q_set, int n_rep, hpfw_hit *d_out,
                                     hpfw_dist_stats *d_stats, hipStream_t s)
{
    if (int rc = within_check(h, q_off, n_q, k, set_off, n_sets, set_clips, q_set, n_rep, d_out)) return rc;
    if (int rc = within_check_index(h, q_off, n_q, set_off, n_sets, set_clips, q_set, n_rep, d_stats != nullptr)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    return ordered_call(h, s, [&] {
        if (n_q == 0) return 0;
        if (!d_q_hp) return fail(HPFW_E_INVALID, "null queries");
        // the caller's queries by set, -1 first: order[r] is the query at place r
        std::vector<int64_t> order((size_t)n_q);
        for (int64_t i = 0; i < n_q; ++i) order[(size_t)i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return q_set[a / n_rep] < q_set[b / n_rep]; });
        if (q_set[order.back() / n_rep] < 0) return search_topk_view(h, whole_index(h), d_q_hp, q_off, n_q, k, d_out, d_stats, s);
        // one table of 8-byte words on the device: order [n_q], the queries' first hashprints [n_q], their offsets in the new
        // order [n_q + 1]; behind it the sets' slots
        const int64_t n_ids = set_off[n_sets];
        std::vector<int64_t> tab((size_t)n_q * 3 + 1);
        int64_t *src_off = tab.data() + n_q, *new_off = src_off + n_q;
        new_off[0] = 0;
        for (int64_t r = 0; r < n_q; ++r) {
            tab[(size_t)r] = order[(size_t)r];
            src_off[r] = q_off[order[(size_t)r]];
            new_off[r + 1] = new_off[r] + (q_off[order[(size_t)r] + 1] - q_off[order[(size_t)r]]);
        }
        int rc;
        const size_t tab_bytes = tab.size() * 8, hit_bytes = (size_t)n_q * k * sizeof(hpfw_hit);
        if ((rc = ensure(h->index.d_within_tab, tab_bytes + (size_t)std::max<int64_t>(n_ids, 1) * 4))) return rc;
        if ((rc = ensure(h->index.d_within_q, (size_t)std::max<int64_t>(new_off[n_q], 1) * 8))) return rc;
        if ((rc = ensure(h->index.d_within_out, hit_bytes + (d_stats ? (size_t)n_q * sizeof(hpfw_dist_stats) : 0)))) return rc;
        const int64_t *d_tab = h->index.d_within_tab.as<int64_t>();
        const int32_t *d_ids = reinterpret_cast<const int32_t *>(h->index.d_within_tab.as<char>() + tab_bytes);
        uint64_t *d_q = h->index.d_within_q.as<uint64_t>();
        hpfw_hit *d_hits = h->index.d_within_out.as<hpfw_hit>();
        hpfw_dist_stats *d_st = d_stats ? reinterpret_cast<hpfw_dist_stats *>(h->index.d_within_out.as<char>() + hit_bytes) : nullptr;
        HIP_TRY(hipMemcpyAsync(h->index.d_within_tab.get(), tab.data(), tab_bytes, hipMemcpyHostToDevice, s));
        if (n_ids) HIP_TRY(hipMemcpyAsync(h->index.d_within_tab.as<char>() + tab_bytes, set_clips, (size_t)n_ids * 4, hipMemcpyHostToDevice, s));
        hpfw::launch_within_gather(d_q_hp, d_tab + n_q, d_tab + 2 * n_q, n_q, d_q, s);
        if ((rc = check_launch("within_gather"))) return rc;
        for (int64_t r0 = 0; r0 < n_q;) {
            const int32_t st = q_set[order[(size_t)r0] / n_rep];
            int64_t r1 = r0;
            while (r1 < n_q && q_set[order[(size_t)r1] / n_rep] == st) ++r1;
            ClipView v;
            if (st < 0) {
                v = whole_index(h);
            } else {
                v = {set_off[st + 1] - set_off[st], 0, d_ids + set_off[st]};
                for (int64_t p = set_off[st]; p < set_off[st + 1]; ++p)
                    v.n_max = std::max(v.n_max, h->index.db_off[(size_t)set_clips[p] + 1] - h->index.db_off[(size_t)set_clips[p]]);
            }
            if ((rc = search_topk_view(h, v, d_q, new_off + r0, r1 - r0, k, d_hits + r0 * k, d_st ? d_st + r0 : nullptr, s))) return rc;
            r0 = r1;
        }
        static_assert(sizeof(hpfw_hit) % 8 == 0 && sizeof(hpfw_dist_stats) % 8 == 0, "the scatter moves 8-byte words");
        hpfw::launch_within_scatter(reinterpret_cast<const uint64_t *>(d_hits), d_tab, n_q, k * (int)(sizeof(hpfw_hit) / 8),
                                    reinterpret_cast<uint64_t *>(d_out), s);
        if (d_stats)
            hpfw::launch_within_scatter(reinterpret_cast<const uint64_t *>(d_st), d_tab, n_q, (int)(sizeof(hpfw_dist_stats) / 8),
                                        reinterpret_cast<uint64_t *>(d_stats), s);
        if ((rc = check_launch("within_scatter"))) return rc;
        HIP_TRY(hipStreamSynchronize(s)); // (the caller's set arrays and the tables above have been read)
        return 0;
    });
}

int hpfw_gpu_search_topk_within_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int k, const int64_t *set_off,
                                       int64_t n_sets, const int32_t *set_clips, const int32_t *q_set, hpfw_hit *d_out,
                                       hpfw_dist_stats *d_stats, void *stream)
{
    return search_topk_within_device(h, d_q_hp, q_off, n_q, k, set_off, n_sets, set_clips, q_set, 1, d_out, d_stats, (hipStream_t)stream);
}

int hpfw_gpu_search_topk_within(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int k, const int64_t *set_off,
                                int64_t n_sets, const int32_t *set_clips, const int32_t *q_set, hpfw_hit *out, hpfw_dist_stats *stats)
{
    if (int rc = within_check(h, q_off, n_q, k, set_off, n_sets, set_clips, q_set, 1, out)) return rc;
    if (int rc = within_check_index(h, q_off, n_q, set_off, n_sets, set_clips, q_set, 1, stats != nullptr)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    if (n_q == 0) return 0;
    return search_round_trip_scored(q_hp, q_off, n_q, n_q * k, out, stats ? n_q : 0, stats,
                                    [&](const uint64_t *d_q, const int64_t *rel, hpfw_hit *d_out, hpfw_dist_stats *d_stats) {
                                        return search_topk_within_device(h, d_q, rel, n_q, k, set_off, n_sets, set_clips, q_set, 1, d_out,
                                                                         d_stats, nullptr);
                                    });
}

// d_stats: NULL, or [n_q][n_shifts] rows, one per query set
// within: NULL, or the sets of the call (q_set: one entry per query, for its n_shifts variants)
struct WithinSets {
    const int64_t *set_off;
    int64_t n_sets;
    const int32_t *set_clips, *q_set;
};

static int search_topk_transposed_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int n_shifts, int k,
                                         hpfw_shift_hit *d_out, hpfw_dist_stats *d_stats, hipStream_t s, const WithinSets *within = nullptr)
{
    if (!h || !q_off || !d_out || n_q < 0 || k < 1 || k > 64 || n_shifts < 1 || n_shifts > hpfw::kMaxShifts)
        return fail(HPFW_E_INVALID, "bad argument");
    if (within) { // (refused here, while nothing has been touched)
        if (int rc = within_check(h, q_off, n_q * n_shifts, k, within->set_off, within->n_sets, within->set_clips, within->q_set, n_shifts, d_out)) return rc;
        if (int rc = within_check_index(h, q_off, n_q * n_shifts, within->set_off, within->n_sets, within->set_clips, within->q_set, n_shifts, d_stats != nullptr)) return rc;
    }
    HIP_TRY(hipSetDevice(h->device));
    return ordered_call(h, s, [&] {
        if (n_q == 0) return 0;
        int rc;
        // the per-shift lists: n_q * n_shifts queries in one pass of the existing scan, then one workgroup per query merges them
        if ((rc = ensure(h->index.d_shift_hits, (size_t)n_q * n_shifts * k * sizeof(hpfw_hit)))) return rc;
        hpfw_hit *d_lists = h->index.d_shift_hits.as<hpfw_hit>();
        rc = within ? search_topk_within_device(h, d_q_hp, q_off, n_q * n_shifts, k, within->set_off, within->n_sets, within->set_clips,
                                                within->q_set, n_shifts, d_lists, d_stats, s)
                    : search_topk_device(h, d_q_hp, q_off, n_q * n_shifts, k, d_lists, d_stats, s);
        if (rc) return rc;
        {
            Timed t(h, K_TOPK, s);
            hpfw::launch_topk_merge_shifts(h->index.d_shift_hits.get(), (int)n_q, n_shifts, k, d_out, s);
        }
        return check_launch("topk_merge_shifts");
    });
}

int hpfw_gpu_search_topk_transposed_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int n_shifts, int k,
                                           hpfw_shift_hit *d_out, void *stream)
{
    return search_topk_transposed_device(h, d_q_hp, q_off, n_q, n_shifts, k, d_out, nullptr, (hipStream_t)stream);
}

int hpfw_gpu_search_topk_transposed_scored_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int n_shifts,
                                                  int k, hpfw_shift_hit *d_out, hpfw_dist_stats *d_stats, void *stream)
{
    if (!d_stats) return fail(HPFW_E_INVALID, "null stats");
    return search_topk_transposed_device(h, d_q_hp, q_off, n_q, n_shifts, k, d_out, d_stats, (hipStream_t)stream);
}

static int search_topk_transposed_host(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int n_shifts, int k,
                                       hpfw_shift_hit *out, hpfw_dist_stats *stats, const WithinSets *within = nullptr)
{
    if (!h || !q_off || !out || n_q < 0 || n_shifts < 1 || n_shifts > hpfw::kMaxShifts) return fail(HPFW_E_INVALID, "bad argument");
    if (k < 1 || k > 64) return fail(HPFW_E_INVALID, "k must be in 1..64");
    if (within) {
        if (int rc = within_check(h, q_off, n_q * n_shifts, k, within->set_off, within->n_sets, within->set_clips, within->q_set, n_shifts, out)) return rc;
        if (int rc = within_check_index(h, q_off, n_q * n_shifts, within->set_off, within->n_sets, within->set_clips, within->q_set, n_shifts, stats != nullptr)) return rc;
    }
    HIP_TRY(hipSetDevice(h->device));
    if (n_q == 0) return 0;
    return search_round_trip_scored(q_hp, q_off, n_q * n_shifts, n_q * k, out, stats ? n_q * n_shifts : 0, stats,
                                    [&](const uint64_t *d_q, const int64_t *rel, hpfw_shift_hit *d_out, hpfw_dist_stats *d_stats) {
                                        return search_topk_transposed_device(h, d_q, rel, n_q, n_shifts, k, d_out, d_stats, nullptr, within);
                                    });
}

int hpfw_gpu_search_topk_transposed_within_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int n_shifts, int k,
                                                  const int64_t *set_off, int64_t n_sets, const int32_t *set_clips, const int32_t *q_set,
                                                  hpfw_shift_hit *d_out, hpfw_dist_stats *d_stats, void *stream)
{
    const WithinSets w{set_off, n_sets, set_clips, q_set};
    return search_topk_transposed_device(h, d_q_hp, q_off, n_q, n_shifts, k, d_out, d_stats, (hipStream_t)stream, &w);
}

int hpfw_gpu_search_topk_transposed_within(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int n_shifts, int k,
                                           const int64_t *set_off, int64_t n_sets, const int32_t *set_clips, const int32_t *q_set,
                                           hpfw_shift_hit *out, hpfw_dist_stats *stats)
{
    const WithinSets w{set_off, n_sets, set_clips, q_set};
    return search_topk_transposed_host(h, q_hp, q_off, n_q, n_shifts, k, out, stats, &w);
}

int hpfw_gpu_search_topk_transposed(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int n_shifts, int k,
                                    hpfw_shift_hit *out)
{
    return search_topk_transposed_host(h, q_hp, q_off, n_q, n_shifts, k, out, nullptr);
}

int hpfw_gpu_search_topk_transposed_scored(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int n_shifts, int k,
                                           hpfw_shift_hit *out, hpfw_dist_stats *stats)
{
    if (!stats) return fail(HPFW_E_INVALID, "null stats");
    return search_topk_transposed_host(h, q_hp, q_off, n_q, n_shifts, k, out, stats);
}

// ---- overlap search (k_search_overlap.hip) ------------------------------------
// what can be refused without the handle, before anything runs; *k_max: the longest query
static int overlap_check(const void *h, const int64_t *q_off, int64_t n_q, const int32_t *exclude, int min_overlap, int k, const void *out,
                         int64_t *k_max)
{
    if (!h || !q_off || !out || n_q < 0) return fail(HPFW_E_INVALID, "bad argument");
    if (k < 1 || k > 64) return fail(HPFW_E_INVALID, "k must be in 1..64");
    if (min_overlap < 1 || min_overlap > 16000) return fail(HPFW_E_INVALID, "min_overlap must be in 1..16000");
    if (int rc = check_q_off(q_off, n_q, k_max)) return rc;
    for (int64_t i = 0; exclude && i < n_q; ++i)
        if (exclude[i] < -1) return fail(HPFW_E_INVALID, "exclude: an entry below -1 (query " + std::to_string(i) + ")");
    return 0;
}

// what overlap_check leaves to the handle: the clips that `exclude` names exist
static int overlap_check_exclude(const hpfw_gpu *h, const int32_t *exclude, int64_t n_q)
{
    const int64_t n_clips = (int64_t)h->index.db_off.size() - 1;
    for (int64_t i = 0; exclude && i < n_q; ++i)
        if (exclude[i] >= n_clips) return fail(HPFW_E_INVALID, "exclude: an entry at or above the number of clips (query " + std::to_string(i) + ")");
    return 0;
}

// d_stats: NULL, or [n_q] rows that receive the moments of the per-clip rates (k_stats.hip: one more reader of the table)
static int search_overlap_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, const int32_t *exclude,
                                 int min_overlap, int k, hpfw_overlap_hit *d_out, hpfw_dist_stats *d_stats, hipStream_t s)
{
    int64_t k_max = 0;
    if (int rc = overlap_check(h, q_off, n_q, exclude, min_overlap, k, d_out, &k_max)) return rc;
    if (n_q > 0 && !d_q_hp) return fail(HPFW_E_INVALID, "null queries");
    if (int rc = overlap_check_exclude(h, exclude, n_q)) return rc;
    const int64_t n_clips = (int64_t)h->index.db_off.size() - 1;
    HIP_TRY(hipSetDevice(h->device));
    return ordered_call(h, s, [&] {
        if (n_q == 0) return 0;
        int rc;
        if (d_stats) HIP_TRY(hipMemsetAsync(d_stats, 0, (size_t)n_q * sizeof(hpfw_dist_stats), s));
        if (n_clips == 0) { // nothing indexed: every slot is "none"
            for (int64_t g0 = 0; g0 < n_q; g0 += 1 << 20)
                hpfw::launch_overlap_select(nullptr, (int)std::min<int64_t>(1 << 20, n_q - g0), 0, 1, nullptr, k, h->index.clip_base, d_out + g0 * k, s);
            return check_launch("overlap_select");
        }
        if (exclude) {
            if ((rc = ensure(h->index.d_ov_exclude, (size_t)n_q * 4))) return rc;
            HIP_TRY(hipMemcpyAsync(h->index.d_ov_exclude.get(), exclude, (size_t)n_q * 4, hipMemcpyHostToDevice, s));
        }
        const bool mfma = hpfw::search_on_matrix_cores(std::getenv("HPFW_OVERLAP_POPC") != nullptr, hpfw::hamming_mfma_lds_bytes((int)k_max));
        const int64_t n_max = index_longest_clip(h);
        // the chunks of a (group, clip) pair go to `splits` workgroups
        const int64_t chunks = std::max<int64_t>((n_max + k_max - 2 * min_overlap) / hpfw::kOverlapChunk + 1, 1);
        const int64_t pairs = n_clips * (mfma ? (n_q + 31) / 32 : n_q);
        const int splits = (int)hpfw::overlap_splits(chunks, pairs, env_forced_splits("HPFW_OVERLAP_SPLITS"));
        if ((int64_t)n_clips * splits > 0x7fffffff) return fail(HPFW_E_UNSUPPORTED, "overlap search: too many clips");
        const int64_t qgroup = hpfw::search_group_queries(n_q, n_clips * splits, hpfw::kOverlapTableEntries, hpfw::kPopcGridQueries, 16,
                                                          env_table_kb("HPFW_OVERLAP_TABLE_KB"));
        const uint64_t *db = h->index.d_db.as<uint64_t>();
        auto skip = [&](const QueryGroup &g) { return exclude ? h->index.d_ov_exclude.as<int32_t>() + g.g0 : nullptr; };
        std::vector<SearchStep> steps;
        if (k_max > 0)
            steps.push_back({K_SCAN, "overlap scan", true, [&](const QueryGroup &g) {
                                 const int64_t *db_off = h->index.d_db_off.as<int64_t>();
                                 if (mfma)
                                     hpfw::launch_overlap_mfma(db, db_off, (int)n_clips, g.d_q_off, g.ng, g.d_qa, g.kt_pad, g.d_gk, (int)k_max, min_overlap,
                                                               splits, h->index.d_ov_tab.get(), s);
                                 else
                                     hpfw::launch_overlap_popc(db, db_off, (int)n_clips, d_q_hp, g.d_q_off, g.ng, min_overlap, splits, h->index.d_ov_tab.get(), s);
                                 return 0;
                             }});
        steps.push_back({K_TOPK, "overlap_select", false, [&](const QueryGroup &g) {
                             hpfw::launch_overlap_select(h->index.d_ov_tab.get(), g.ng, (int)n_clips, splits, skip(g), k, h->index.clip_base, d_out + g.g0 * k, s);
                             return 0;
                         }});
        if (d_stats) // (the select kernel has folded every clip's splits into its first entry)
            steps.push_back({K_TOPK, "overlap_stats", false, [&](const QueryGroup &g) {
                                 hpfw::launch_overlap_stats(h->index.d_ov_tab.get(), g.ng, (int)n_clips, splits, skip(g), d_stats + g.g0, s);
                                 return 0;
                             }});
        if ((rc = search_run_groups(h, s, d_q_hp, q_off, n_q, k_max, qgroup, mfma && k_max > 0, h->index.d_ov_tab, (size_t)n_clips * splits * 16, steps)))
            return rc;
        if (exclude) HIP_TRY(hipStreamSynchronize(s)); // (the caller's array has been read)
        return 0;
    });
}

int hpfw_gpu_search_overlap_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, const int32_t *exclude,
                                   int min_overlap, int k, hpfw_overlap_hit *d_out, void *stream)
{
    return search_overlap_device(h, d_q_hp, q_off, n_q, exclude, min_overlap, k, d_out, nullptr, (hipStream_t)stream);
}

int hpfw_gpu_search_overlap_scored_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, const int32_t *exclude,
                                          int min_overlap, int k, hpfw_overlap_hit *d_out, hpfw_dist_stats *d_stats, void *stream)
{
    if (!d_stats) return fail(HPFW_E_INVALID, "null stats");
    return search_overlap_device(h, d_q_hp, q_off, n_q, exclude, min_overlap, k, d_out, d_stats, (hipStream_t)stream);
}

// host buffers: stats NULL (plain) or [n_q]
static int search_overlap_host(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, const int32_t *exclude, int min_overlap,
                               int k, hpfw_overlap_hit *out, hpfw_dist_stats *stats)
{
    int64_t k_max = 0;
    if (int rc = overlap_check(h, q_off, n_q, exclude, min_overlap, k, out, &k_max)) return rc;
    if (n_q > 0 && q_off[n_q] > q_off[0] && !q_hp) return fail(HPFW_E_INVALID, "null queries");
    if (int rc = overlap_check_exclude(h, exclude, n_q)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    if (n_q == 0) return 0;
    return search_round_trip_scored(q_hp, q_off, n_q, n_q * k, out, stats ? n_q : 0, stats,
                                    [&](const uint64_t *d_q, const int64_t *rel, hpfw_overlap_hit *d_out, hpfw_dist_stats *d_stats) {
                                        return search_overlap_device(h, d_q, rel, n_q, exclude, min_overlap, k, d_out, d_stats, nullptr);
                                    });
}

int hpfw_gpu_search_overlap(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, const int32_t *exclude, int min_overlap,
                            int k, hpfw_overlap_hit *out)
{
    return search_overlap_host(h, q_hp, q_off, n_q, exclude, min_overlap, k, out, nullptr);
}

int hpfw_gpu_search_overlap_scored(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, const int32_t *exclude,
                                   int min_overlap, int k, hpfw_overlap_hit *out, hpfw_dist_stats *stats)
{
    if (!stats) return fail(HPFW_E_INVALID, "null stats");
    return search_overlap_host(h, q_hp, q_off, n_q, exclude, min_overlap, k, out, stats);
}

int hpfw_gpu_merge_topk(const hpfw_hit *in, int n_shards, int64_t n_q, int k, hpfw_hit *out)
{
    if (!in || !out || n_shards < 1 || n_q < 0 || k < 1) return fail(HPFW_E_INVALID, "bad argument");
    std::vector<hpfw_hit> all((size_t)n_shards * k);
    for (int64_t q = 0; q < n_q; ++q) {
        for (int s = 0; s < n_shards; ++s)
            for (int t = 0; t < k; ++t) all[(size_t)s * k + t] = in[((size_t)s * n_q + q) * k + t];
        std::stable_sort(all.begin(), all.end(), [](const hpfw_hit &a, const hpfw_hit &b) {
            if (a.dist != b.dist) return a.dist < b.dist;
            return a.clip < b.clip;
        });
        for (int t = 0; t < k; ++t) out[(size_t)q * k + t] = all[(size_t)t];
    }
    return 0;
}

// one kernel serves both kinds of hit: the key (dist, clip) is the first two words of either, the rest is payload
static_assert(sizeof(hpfw_hit) == 16 && sizeof(hpfw_shift_hit) == 16, "the merge kernel moves 16-byte records");
static_assert(offsetof(hpfw_hit, dist) == 0 && offsetof(hpfw_hit, clip) == 4 && offsetof(hpfw_shift_hit, dist) == 0 &&
                  offsetof(hpfw_shift_hit, clip) == 4,
              "the merge kernel reads the key (dist, clip) from the first two words");
static_assert(sizeof(hpfw_dist_stats) == 24 && offsetof(hpfw_dist_stats, sum_sq) == 8 && offsetof(hpfw_dist_stats, n) == 16,
              "the sum kernel reads rows of 24 bytes");

int hpfw_gpu_merge_topk_device(hpfw_gpu *h, const void *d_in, int n_shards, int64_t n_q, int k, void *d_out, void *stream)
{
    if (!h || !d_in || !d_out || n_shards < 1 || n_shards > 64 || n_q < 0 || n_q > 0x7fffffff || ((uintptr_t)d_in | (uintptr_t)d_out) % 16)
        return fail(HPFW_E_INVALID, "bad argument");
    if (k < 1 || k > 64) return fail(HPFW_E_INVALID, "k must be in 1..64");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        if (n_q == 0) return 0;
        {
            Timed t(h, K_TOPK, s);
            hpfw::launch_topk_merge_shards(d_in, n_shards, n_q, k, d_out, s);
        }
        return check_launch("topk_merge_shards");
    });
}

int hpfw_gpu_sum_stats_device(hpfw_gpu *h, const hpfw_dist_stats *d_in, int n_shards, int64_t rows, hpfw_dist_stats *d_out, void *stream)
{
    if (!h || !d_in || !d_out || n_shards < 1 || n_shards > 64 || rows < 0 || rows > (int64_t)0x7fffffff * 256 ||
        ((uintptr_t)d_in | (uintptr_t)d_out) % 8)
        return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        if (rows == 0) return 0;
        {
            Timed t(h, K_TOPK, s);
            hpfw::launch_sum_stats(d_in, n_shards, rows, d_out, s);
        }
        return check_launch("sum_stats");
    });
}

} // extern "C"
