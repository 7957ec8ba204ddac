// search.hip -- the index of hashprints and its searches (top-k, transposed, voting), and AudioCombiner's exact-hash
// index (k_combiner.hip).
#include "handle.h"

namespace {
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
int upload_db_off(hpfw_gpu *h, hipStream_t s)
{
    if (!h->index.db_off_dirty) return 0;
    if (int rc = ensure(h->index.d_db_off, h->index.db_off.size() * 8)) return rc;
    HIP_TRY(hipMemcpyAsync(h->index.d_db_off.get(), h->index.db_off.data(), h->index.db_off.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    h->index.db_off_dirty = false;
    return 0;
}
} // namespace

extern "C" {

// ---- index + search ----------------------------------------------------------------------------
int hpfw_gpu_index_clear(hpfw_gpu *h)
{
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    h->index.db_off.assign(1, 0);
    h->index.db_off_dirty = true;
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
        if (need > h->index.d_db.capacity()) {
            DevBuf nd;
            HIP_TRY(nd.alloc(std::max({need, h->index.d_db.capacity() * 2, (size_t)8 << 16})));
            // earlier appends may still be in flight on a non-blocking stream the null-stream copy below would
            // not wait for, and scans may still be reading the old buffer: growing is rare (capacity doubles)
            HIP_TRY(hipDeviceSynchronize());
            if (have) HIP_TRY(hipMemcpy(nd.get(), h->index.d_db.get(), (size_t)have * 8, hipMemcpyDeviceToDevice));
            h->index.d_db = std::move(nd); // (the old buffer goes with nd)
        }
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

// the top-k search of n_q queries; d_stats: NULL, or [n_q] rows that receive the moments of the per-clip best distances
// (k_stats.hip: one more reader of the table the scan wrote)
static int search_topk_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int k, hpfw_hit *d_out,
                              hpfw_dist_stats *d_stats, hipStream_t s)
{
    if (!h || !q_off || !d_out || n_q < 0 || k < 1 || k > 64) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    return ordered_call(h, s, [&] {
        if (n_q == 0) return 0;
        if (!d_q_hp) return fail(HPFW_E_INVALID, "null queries");
        const int64_t n_clips = (int64_t)h->index.db_off.size() - 1;
        int rc;
        if (d_stats) HIP_TRY(hipMemsetAsync(d_stats, 0, (size_t)n_q * sizeof(hpfw_dist_stats), s));
        if (n_clips == 0) { // nothing indexed: every slot is "none"
            hpfw::launch_topk(nullptr, (int)n_q, 0, k, h->index.clip_base, d_out, s);
            return check_launch("topk");
        }
        if ((rc = upload_db_off(h, s))) return rc;
        int64_t k_max = 0;
        for (int64_t i = 0; i < n_q; ++i) {
            if (q_off[i + 1] < q_off[i]) return fail(HPFW_E_INVALID, "q_off must be non-decreasing");
            k_max = std::max(k_max, q_off[i + 1] - q_off[i]);
        }
        if (k_max > 16000) return fail(HPFW_E_UNSUPPORTED, "query longer than 16000 hashprints");
        // d <= 64 k_max: the sum of squares stays below 2^64 while n_clips k_max^2 4096 does
        if (d_stats && (unsigned __int128)n_clips * (uint64_t)(k_max * k_max) * 4096 >= ((unsigned __int128)1 << 64))
            return fail(HPFW_E_UNSUPPORTED, "scored search: n_clips * k_max^2 * 4096 must stay below 2^64");
        if ((rc = ensure(h->index.d_q_off, (size_t)(n_q + 1) * 8))) return rc;
        HIP_TRY(hipMemcpyAsync(h->index.d_q_off.get(), q_off, (size_t)(n_q + 1) * 8, hipMemcpyHostToDevice, s));
        // queries are processed in groups so the (query, clip) table stays below 1 GiB
        int64_t qgroup = std::max<int64_t>(32, ((int64_t)1 << 27) / n_clips / 32 * 32);
        qgroup = std::min<int64_t>(qgroup, (n_q + 31) / 32 * 32);
        qgroup = std::min<int64_t>(qgroup, (int64_t)65535 * 8 / 32 * 32); // the scans put groups of 8 / 32 queries along gridDim.y
        if ((rc = ensure(h->index.d_best, (size_t)qgroup * n_clips * 8))) return rc;
        // The scan runs on the matrix cores (k_search_mfma.hip) unless the window does not fit the LDS
        // (queries of several thousand hashprints) or HPFW_SEARCH_POPC asks for the xor/popcount kernel; fewer than
        // 8 queries go one by one through the shifted-rows variant (HPFW_SEARCH_MFMA / HPFW_SEARCH_SHIFT force
        // the grouped / the shifted-rows kernel for any number of queries).
        // A group of 32 queries is one MFMA tile: with fewer than 8 queries most of its rows would be padding
        // and the popcount kernel (one workgroup per 8 queries) does less work.
        const bool mfma = !std::getenv("HPFW_SEARCH_POPC") && hpfw::hamming_mfma_lds_bytes((int)k_max) <= 160 * 1024 &&
                          k_max > 0 && (n_q >= 8 || std::getenv("HPFW_SEARCH_MFMA"));
        const int kt_pad = hpfw::hamming_mfma_kt_pad((int)k_max);
        int64_t n_max = 0;
        for (int64_t i = 0; i < n_clips; ++i) n_max = std::max(n_max, h->index.db_off[i + 1] - h->index.db_off[i]);
        if (mfma) {
            if ((rc = ensure(h->index.d_qa, (size_t)(qgroup / 32) * kt_pad * 1024))) return rc;
            if ((rc = ensure(h->index.d_gk, (size_t)(qgroup / 32) * 8))) return rc;
        }
        std::vector<int> gk;
        for (int64_t g0 = 0; g0 < n_q; g0 += qgroup) {
            const int ng = (int)std::min<int64_t>(qgroup, n_q - g0);
            HIP_TRY(hipMemsetAsync(h->index.d_best.get(), 0xff, (size_t)ng * n_clips * 8, s));
            hpfw::SearchArgs a;
            a.db = h->index.d_db.as<uint64_t>();
            a.db_off = h->index.d_db_off.as<int64_t>();
            a.n_clips = (int)n_clips;
            a.q = d_q_hp;
            a.q_off = h->index.d_q_off.as<int64_t>() + g0;
            a.n_q = ng;
            a.k_max = (int)k_max;
            a.best = h->index.d_best.as<uint64_t>();
            const bool few = (!mfma || std::getenv("HPFW_SEARCH_SHIFT")) && !std::getenv("HPFW_SEARCH_POPC") && k_max > 0 && n_max > 0 &&
                             hpfw::hamming_shift_lds_bytes((int)k_max) <= 160 * 1024;
            if (few) { // a handful of queries: one launch each, the tile rows are shifts of the query
                if ((rc = ensure(h->index.d_qa, hpfw::hamming_shift_image_bytes((int)k_max)))) return rc;
                Timed t(h, K_SCAN, s);
                for (int i = 0; i < ng; ++i) {
                    const int kq = (int)(q_off[g0 + i + 1] - q_off[g0 + i]);
                    if (kq <= 0) continue;
                    hpfw::launch_hamming_shift(a.db, a.db_off, (int)n_clips, (int)std::max<int64_t>(n_max - std::min<int64_t>(kq, n_max) + 1, 1),
                                               d_q_hp + q_off[g0 + i], kq, h->index.d_qa.get(), a.best + (size_t)i * n_clips, s);
                }
            } else if (mfma && n_max > 0) {
                gk.assign((size_t)(ng + 31) / 32 * 2, 0); // per group: longest query, shortest non-empty query
                int kmin_all = 0;
                for (int i = 0; i < ng; ++i) {
                    const int kq = (int)(q_off[g0 + i + 1] - q_off[g0 + i]);
                    int &mx = gk[(size_t)i / 32 * 2], &mn = gk[(size_t)i / 32 * 2 + 1];
                    mx = std::max(mx, kq);
                    if (kq > 0) mn = mn == 0 ? kq : std::min(mn, kq);
                    if (kq > 0) kmin_all = kmin_all == 0 ? kq : std::min(kmin_all, kq);
                }
                HIP_TRY(hipMemcpyAsync(h->index.d_gk.get(), gk.data(), gk.size() * 4, hipMemcpyHostToDevice, s));
                HIP_TRY(hipStreamSynchronize(s)); // gk is reused by the next group of queries
                Timed t(h, K_SCAN, s);
                hpfw::launch_expand_queries(d_q_hp, a.q_off, ng, kt_pad, h->index.d_qa.get(), s);
                // offsets exist up to n_max - (shortest query): that many chunks of workgroups per clip
                hpfw::launch_hamming_mfma(a, h->index.d_qa.get(), kt_pad, h->index.d_gk.as<int>(), (int)std::max<int64_t>(n_max - std::min<int64_t>(kmin_all, n_max) + 1, 1), s);
            } else {
                Timed t(h, K_SCAN, s);
                hpfw::launch_hamming_scan(a, s);
            }
            if ((rc = check_launch("hamming_scan"))) return rc;
            {
                Timed t(h, K_TOPK, s);
                if (n_clips >= 16384 && ng <= 64) { // one workgroup per query would crawl through the whole table
                    if ((rc = ensure(h->index.d_topk_scratch, hpfw::topk_scratch_bytes(ng, k)))) return rc;
                    hpfw::launch_topk_two_step(a.best, ng, (int)n_clips, k, h->index.clip_base, h->index.d_topk_scratch.get(), d_out + g0 * k, s);
                } else {
                    hpfw::launch_topk(a.best, ng, (int)n_clips, k, h->index.clip_base, d_out + g0 * k, s);
                }
            }
            if ((rc = check_launch("topk"))) return rc;
            if (d_stats) {
                Timed t(h, K_TOPK, s);
                hpfw::launch_dist_stats(a.best, a.db_off, a.q_off, ng, (int)n_clips, d_stats + g0, s);
            }
            if (d_stats && (rc = check_launch("dist_stats"))) return rc;
        }
        return 0;
    });
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

// d_stats: NULL, or [n_q][n_shifts] rows, one per query set
static int search_topk_transposed_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int n_shifts, int k,
                                         hpfw_shift_hit *d_out, hpfw_dist_stats *d_stats, hipStream_t s)
{
    if (!h || !q_off || !d_out || n_q < 0 || k < 1 || k > 64 || n_shifts < 1 || n_shifts > hpfw::kMaxShifts)
        return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    return ordered_call(h, s, [&] {
        if (n_q == 0) return 0;
        int rc;
        // the per-shift lists: n_q * n_shifts queries in one pass of the existing scan, then one workgroup per query merges them
        if ((rc = ensure(h->index.d_shift_hits, (size_t)n_q * n_shifts * k * sizeof(hpfw_hit)))) return rc;
        if ((rc = search_topk_device(h, d_q_hp, q_off, n_q * n_shifts, k, h->index.d_shift_hits.as<hpfw_hit>(), d_stats, s))) return rc;
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
                                       hpfw_shift_hit *out, hpfw_dist_stats *stats)
{
    if (!h || !q_off || !out || n_q < 0 || n_shifts < 1 || n_shifts > hpfw::kMaxShifts) return fail(HPFW_E_INVALID, "bad argument");
    if (k < 1 || k > 64) return fail(HPFW_E_INVALID, "k must be in 1..64");
    HIP_TRY(hipSetDevice(h->device));
    if (n_q == 0) return 0;
    return search_round_trip_scored(q_hp, q_off, n_q * n_shifts, n_q * k, out, stats ? n_q * n_shifts : 0, stats,
                                    [&](const uint64_t *d_q, const int64_t *rel, hpfw_shift_hit *d_out, hpfw_dist_stats *d_stats) {
                                        return search_topk_transposed_device(h, d_q, rel, n_q, n_shifts, k, d_out, d_stats, nullptr);
                                    });
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
    *k_max = 0;
    for (int64_t i = 0; i < n_q; ++i) {
        if (q_off[i + 1] < q_off[i]) return fail(HPFW_E_INVALID, "q_off must be non-decreasing");
        *k_max = std::max(*k_max, q_off[i + 1] - q_off[i]);
    }
    if (*k_max > 16000) return fail(HPFW_E_UNSUPPORTED, "query longer than 16000 hashprints");
    for (int64_t i = 0; exclude && i < n_q; ++i)
        if (exclude[i] < -1) return fail(HPFW_E_INVALID, "exclude: an entry below -1 (query " + std::to_string(i) + ")");
    return 0;
}

// d_stats: NULL, or [n_q] rows that receive the moments of the per-clip rates (k_stats.hip: one more reader of the table)
static int search_overlap_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, const int32_t *exclude,
                                 int min_overlap, int k, hpfw_overlap_hit *d_out, hpfw_dist_stats *d_stats, hipStream_t s)
{
    int64_t k_max = 0;
    if (int rc = overlap_check(h, q_off, n_q, exclude, min_overlap, k, d_out, &k_max)) return rc;
    if (n_q > 0 && !d_q_hp) return fail(HPFW_E_INVALID, "null queries");
    const int64_t n_clips = (int64_t)h->index.db_off.size() - 1;
    for (int64_t i = 0; exclude && i < n_q; ++i)
        if (exclude[i] >= n_clips) return fail(HPFW_E_INVALID, "exclude: an entry at or above the number of clips (query " + std::to_string(i) + ")");
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
        if ((rc = upload_db_off(h, s))) return rc;
        if ((rc = ensure(h->index.d_q_off, (size_t)(n_q + 1) * 8))) return rc;
        HIP_TRY(hipMemcpyAsync(h->index.d_q_off.get(), q_off, (size_t)(n_q + 1) * 8, hipMemcpyHostToDevice, s));
        if (exclude) {
            if ((rc = ensure(h->index.d_ov_exclude, (size_t)n_q * 4))) return rc;
            HIP_TRY(hipMemcpyAsync(h->index.d_ov_exclude.get(), exclude, (size_t)n_q * 4, hipMemcpyHostToDevice, s));
        }
        // The scan runs on the matrix cores unless the window does not fit the LDS (the bound of the plain search) or
        // HPFW_OVERLAP_POPC asks for the xor/popcount kernel.
        const bool mfma = !std::getenv("HPFW_OVERLAP_POPC") && hpfw::hamming_mfma_lds_bytes((int)k_max) <= 160 * 1024;
        int64_t n_max = 0;
        for (int64_t i = 0; i < n_clips; ++i) n_max = std::max(n_max, h->index.db_off[i + 1] - h->index.db_off[i]);
        // A clip's lags come in chunks of 1024; with few (group, clip) pairs the chunks of a clip go to `splits` workgroups,
        // each with an entry of its own (HPFW_OVERLAP_SPLITS: that many, for tests of either shape)
        const int64_t chunks = std::max<int64_t>((n_max + k_max - 2 * min_overlap) / hpfw::kOverlapChunk + 1, 1);
        const int64_t pairs = n_clips * (mfma ? (n_q + 31) / 32 : n_q);
        int64_t splits = std::min<int64_t>({chunks, (2048 + pairs - 1) / pairs, 64});
        if (const char *e = std::getenv("HPFW_OVERLAP_SPLITS")) splits = std::min<int64_t>(std::max(std::atoi(e), 1), 64);
        // queries are processed in groups so the table stays below 1 GiB
        int64_t qgroup = std::max<int64_t>(32, ((int64_t)1 << 26) / (n_clips * splits) / 32 * 32);
        qgroup = std::min<int64_t>(qgroup, (n_q + 31) / 32 * 32);
        qgroup = std::min<int64_t>(qgroup, 65504); // the popcount kernel puts one query per gridDim.y
        if ((int64_t)n_clips * splits > 0x7fffffff) return fail(HPFW_E_UNSUPPORTED, "overlap search: too many clips");
        if ((rc = ensure(h->index.d_ov_tab, (size_t)qgroup * n_clips * splits * 16))) return rc;
        const int kt_pad = hpfw::hamming_mfma_kt_pad((int)k_max);
        if (mfma) {
            if ((rc = ensure(h->index.d_qa, (size_t)(qgroup / 32) * kt_pad * 1024))) return rc;
            if ((rc = ensure(h->index.d_gk, (size_t)(qgroup / 32) * 4))) return rc;
        }
        std::vector<int> gk;
        for (int64_t g0 = 0; g0 < n_q; g0 += qgroup) {
            const int ng = (int)std::min<int64_t>(qgroup, n_q - g0);
            HIP_TRY(hipMemsetAsync(h->index.d_ov_tab.get(), 0xff, (size_t)ng * n_clips * splits * 16, s));
            const uint64_t *db = h->index.d_db.as<uint64_t>();
            const int64_t *db_off = h->index.d_db_off.as<int64_t>(), *d_q_off = h->index.d_q_off.as<int64_t>() + g0;
            if (mfma && k_max > 0) {
                gk.assign((size_t)(ng + 31) / 32, 0);
                for (int i = 0; i < ng; ++i) gk[(size_t)i / 32] = std::max(gk[(size_t)i / 32], (int)(q_off[g0 + i + 1] - q_off[g0 + i]));
                HIP_TRY(hipMemcpyAsync(h->index.d_gk.get(), gk.data(), gk.size() * 4, hipMemcpyHostToDevice, s));
                HIP_TRY(hipStreamSynchronize(s)); // gk is reused by the next group of queries
                Timed t(h, K_SCAN, s);
                hpfw::launch_expand_queries(d_q_hp, d_q_off, ng, kt_pad, h->index.d_qa.get(), s);
                hpfw::launch_overlap_mfma(db, db_off, (int)n_clips, d_q_off, ng, h->index.d_qa.get(), kt_pad, h->index.d_gk.as<int>(), (int)k_max,
                                          min_overlap, (int)splits, h->index.d_ov_tab.get(), s);
            } else if (k_max > 0) {
                Timed t(h, K_SCAN, s);
                hpfw::launch_overlap_popc(db, db_off, (int)n_clips, d_q_hp, d_q_off, ng, min_overlap, (int)splits, h->index.d_ov_tab.get(), s);
            }
            if ((rc = check_launch("overlap scan"))) return rc;
            {
                Timed t(h, K_TOPK, s);
                hpfw::launch_overlap_select(h->index.d_ov_tab.get(), ng, (int)n_clips, (int)splits,
                                            exclude ? h->index.d_ov_exclude.as<int32_t>() + g0 : nullptr, k, h->index.clip_base, d_out + g0 * k, s);
            }
            if ((rc = check_launch("overlap_select"))) return rc;
            if (d_stats) { // (the select kernel has folded every clip's splits into its first entry)
                Timed t(h, K_TOPK, s);
                hpfw::launch_overlap_stats(h->index.d_ov_tab.get(), ng, (int)n_clips, (int)splits,
                                           exclude ? h->index.d_ov_exclude.as<int32_t>() + g0 : nullptr, d_stats + g0, s);
            }
            if (d_stats && (rc = check_launch("overlap_stats"))) return rc;
        }
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
    const int64_t n_clips = (int64_t)h->index.db_off.size() - 1;
    for (int64_t i = 0; exclude && i < n_q; ++i)
        if (exclude[i] >= n_clips) return fail(HPFW_E_INVALID, "exclude: an entry at or above the number of clips (query " + std::to_string(i) + ")");
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

// ---- AudioCombiner: exact-hash index + offset votes (k_combiner.hip) --------------------------------
static hpfw::Combiner *combiner_of(hpfw_gpu *h)
{
    if (!h->combiner) h->combiner.reset(new hpfw::Combiner());
    return h->combiner.get();
}

int hpfw_gpu_combiner_clear(hpfw_gpu *h)
{
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    combiner_of(h)->clear();
    return 0;
}

static int combiner_add_impl(hpfw_gpu *h, const uint16_t *hp, const int64_t *offsets, int64_t n_rec, bool dev, hipStream_t s)
{
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    return ordered_call(h, s, [&] {
        std::string why;
        const int rc = combiner_of(h)->add(hp, dev, offsets, n_rec, s, why);
        return rc ? fail(rc, why) : 0;
    });
}

int hpfw_gpu_combiner_add(hpfw_gpu *h, const uint16_t *hp, const int64_t *offsets, int64_t n_rec)
{
    return combiner_add_impl(h, hp, offsets, n_rec, false, nullptr);
}

int hpfw_gpu_combiner_add_device(hpfw_gpu *h, const uint16_t *d_hp, const int64_t *offsets, int64_t n_rec, void *stream)
{
    return combiner_add_impl(h, d_hp, offsets, n_rec, true, (hipStream_t)stream);
}

int64_t hpfw_gpu_combiner_size(hpfw_gpu *h) { return h && h->combiner ? h->combiner->size() : 0; }

int hpfw_gpu_combiner_get(hpfw_gpu *h, int64_t *val_start, uint32_t *rec, uint32_t *off, int64_t cap)
{
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    std::string why;
    const int rc = combiner_of(h)->get(val_start, rec, off, cap, why);
    return rc ? fail(rc, why) : 0;
}

static int combiner_search_device(hpfw_gpu *h, const uint16_t *d_q, const int64_t *q_off, const int32_t *exclude, int64_t n_q,
                                  hpfw_combine_result *d_find, int k, hpfw_align_hit *d_align, hipStream_t s)
{
    if (!h || !q_off || n_q < 0 || (!d_find && !d_align)) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    return ordered_call(h, s, [&] {
        std::string why;
        const int rc = combiner_of(h)->search(d_q, q_off, exclude, n_q, d_find, k, d_align, s, why);
        return rc ? fail(rc, why) : 0;
    });
}

// host buffers: queries in, results out, synchronises
static int combiner_search_host(hpfw_gpu *h, const uint16_t *q_hp, const int64_t *q_off, const int32_t *exclude, int64_t n_q,
                                hpfw_combine_result *find_out, int k, hpfw_align_hit *align_out)
{
    if (!h || !q_off || n_q < 0 || (!find_out && !align_out)) return fail(HPFW_E_INVALID, "bad argument");
    if (align_out && (k < 1 || k > 64)) return fail(HPFW_E_INVALID, "k must be in 1..64");
    HIP_TRY(hipSetDevice(h->device));
    if (n_q == 0) return 0;
    if (find_out)
        return search_round_trip(q_hp, q_off, n_q, n_q, find_out, [&](const uint16_t *d_q, const int64_t *rel, hpfw_combine_result *d_out) {
            return combiner_search_device(h, d_q, rel, exclude, n_q, d_out, k, nullptr, nullptr);
        });
    return search_round_trip(q_hp, q_off, n_q, n_q * k, align_out, [&](const uint16_t *d_q, const int64_t *rel, hpfw_align_hit *d_out) {
        return combiner_search_device(h, d_q, rel, exclude, n_q, nullptr, k, d_out, nullptr);
    });
}

int hpfw_gpu_combiner_find_device(hpfw_gpu *h, const uint16_t *d_q_hp, const int64_t *q_off, const int32_t *exclude, int64_t n_q,
                                  hpfw_combine_result *d_out, void *stream)
{
    if (!d_out) return fail(HPFW_E_INVALID, "null output");
    return combiner_search_device(h, d_q_hp, q_off, exclude, n_q, d_out, 0, nullptr, (hipStream_t)stream);
}

int hpfw_gpu_combiner_find(hpfw_gpu *h, const uint16_t *q_hp, const int64_t *q_off, const int32_t *exclude, int64_t n_q,
                           hpfw_combine_result *out)
{
    if (!out) return fail(HPFW_E_INVALID, "null output");
    return combiner_search_host(h, q_hp, q_off, exclude, n_q, out, 0, nullptr);
}

int hpfw_gpu_combiner_align_device(hpfw_gpu *h, const uint16_t *d_q_hp, const int64_t *q_off, const int32_t *exclude, int64_t n_q,
                                   int k, hpfw_align_hit *d_out, void *stream)
{
    if (!d_out || k < 1 || k > 64) return fail(HPFW_E_INVALID, "null output or k outside 1..64");
    return combiner_search_device(h, d_q_hp, q_off, exclude, n_q, nullptr, k, d_out, (hipStream_t)stream);
}

int hpfw_gpu_combiner_align(hpfw_gpu *h, const uint16_t *q_hp, const int64_t *q_off, const int32_t *exclude, int64_t n_q, int k,
                            hpfw_align_hit *out)
{
    if (!out) return fail(HPFW_E_INVALID, "null output");
    return combiner_search_host(h, q_hp, q_off, exclude, n_q, nullptr, k, out);
}

// ---- sample-accurate offsets: exact cross-correlation of PCM16 (k_xcorr.hip), the Mel front end's kept frames ----
// n_pcm < 0: the buffer's size is not known (the device entry point)
static int xcorr_device(hpfw_gpu *h, const int16_t *d_pcm, int64_t n_pcm, const hpfw_xcorr_job *jobs, int64_t n_jobs, int64_t *d_r,
                        hpfw_xcorr_peak *d_peaks, hipStream_t s)
{
    if (!h || n_jobs < 0 || (n_jobs > 0 && (!d_pcm || !jobs || !d_peaks))) return fail(HPFW_E_INVALID, "xcorr: null argument");
    for (int64_t i = 0; i < n_jobs; ++i)
        if (const char *why = hpfw::xcorr_check(jobs[i], n_pcm)) return fail(HPFW_E_INVALID, std::string(why) + " (job " + std::to_string(i) + ")");
    HIP_TRY(hipSetDevice(h->device));
    if (n_jobs == 0) return 0;
    const char *mode = std::getenv("HPFW_XCORR");
    const bool valu_only = mode && !std::strcmp(mode, "valu");
    return ordered_call(h, s, [&] {
        // passes of jobs: the parts and (when the caller keeps no r) the lags of a pass are bounded
        constexpr int64_t kMaxItems = (int64_t)1 << 20, kMaxLags = (int64_t)1 << 24;
        std::vector<hpfw::XcJob> tab;
        std::vector<hpfw::XcItem> mfma, valu;
        int64_t r_done = 0; // lags of the passes before this one
        for (int64_t j0 = 0; j0 < n_jobs;) {
            tab.clear();
            mfma.clear();
            valu.clear();
            int64_t j1 = j0, lags = 0;
            for (; j1 < n_jobs && (j1 == j0 || ((int64_t)(mfma.size() + valu.size()) < kMaxItems && lags < kMaxLags)); ++j1) {
                tab.push_back(hpfw::xcorr_plan_job(jobs[j1], (int32_t)(j1 - j0), (d_r ? r_done : 0) + lags, valu_only, mfma, valu));
                lags += hpfw::xcorr_lags(jobs[j1]);
            }
            const size_t jb = tab.size() * sizeof(hpfw::XcJob), mb = mfma.size() * sizeof(hpfw::XcItem), vb = valu.size() * sizeof(hpfw::XcItem);
            if (j0 > 0) HIP_TRY(hipStreamSynchronize(s)); // the pass before this one still reads the tables
            if (int rc = ensure(h->xcorr.d_tab, jb + mb + vb)) return rc;
            if (!d_r)
                if (int rc = ensure(h->xcorr.d_r, (size_t)lags * 8)) return rc;
            char *d_tab = h->xcorr.d_tab.as<char>();
            HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), jb, hipMemcpyHostToDevice, s));
            if (mb) HIP_TRY(hipMemcpyAsync(d_tab + jb, mfma.data(), mb, hipMemcpyHostToDevice, s));
            if (vb) HIP_TRY(hipMemcpyAsync(d_tab + jb + mb, valu.data(), vb, hipMemcpyHostToDevice, s));
            HIP_TRY(hipStreamSynchronize(s)); // (the host vectors are reused or die)
            hpfw::launch_xcorr(d_pcm, (const hpfw::XcJob *)d_tab, j1 - j0, (const hpfw::XcItem *)(d_tab + jb), (int64_t)mfma.size(),
                               (const hpfw::XcItem *)(d_tab + jb + mb), (int64_t)valu.size(), d_r ? d_r : h->xcorr.d_r.as<int64_t>(),
                               d_peaks + j0, s);
            if (int rc = check_launch("xcorr")) return rc;
            r_done += lags;
            j0 = j1;
        }
        return 0;
    });
}

int hpfw_gpu_xcorr_pcm16(hpfw_gpu *h, const int16_t *d_pcm, const hpfw_xcorr_job *jobs, int64_t n_jobs, int64_t *d_r,
                         hpfw_xcorr_peak *d_peaks, void *stream)
{
    return xcorr_device(h, d_pcm, -1, jobs, n_jobs, d_r, d_peaks, (hipStream_t)stream);
}

int hpfw_gpu_xcorr_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_pcm, const hpfw_xcorr_job *jobs, int64_t n_jobs, int64_t *r,
                              hpfw_xcorr_peak *peaks)
{
    if (!h || n_jobs < 0 || n_pcm < 0 || (n_jobs > 0 && (!pcm || !jobs || !peaks))) return fail(HPFW_E_INVALID, "xcorr: null argument");
    int64_t lags = 0;
    for (int64_t i = 0; i < n_jobs; ++i) { // (before anything is allocated; the device entry point checks again)
        if (const char *why = hpfw::xcorr_check(jobs[i], n_pcm)) return fail(HPFW_E_INVALID, std::string(why) + " (job " + std::to_string(i) + ")");
        lags += hpfw::xcorr_lags(jobs[i]);
    }
    HIP_TRY(hipSetDevice(h->device));
    if (n_jobs == 0) return 0;
    HostTrip t;
    const int16_t *d_pcm = t.take<int16_t>((size_t)std::max<int64_t>(n_pcm, 1) * 2, n_pcm ? pcm : nullptr);
    int64_t *d_r = r ? t.take<int64_t>((size_t)lags * 8, nullptr, -1, r) : nullptr;
    hpfw_xcorr_peak *d_peaks = t.take<hpfw_xcorr_peak>((size_t)n_jobs * sizeof(hpfw_xcorr_peak), nullptr, -1, peaks);
    return t.run(true, [&] { return xcorr_device(h, d_pcm, n_pcm, jobs, n_jobs, d_r, d_peaks, nullptr); });
}

int hpfw_gpu_mel_kept_frames_pcm16_host(hpfw_gpu *h, const int16_t *pcm, int64_t n_samples, int64_t n_clips, int32_t *frames,
                                        int64_t stride, int32_t *n_kept)
{
    if (!h || !pcm || !frames || !n_kept || n_clips < 0 || n_samples < 1) return fail(HPFW_E_INVALID, "bad argument");
    const int64_t nf = hpfw::mel_frames(n_samples), n_blk = (n_samples + hpfw::kMelHop - 1) / hpfw::kMelHop;
    if (stride < nf) return fail(HPFW_E_INVALID, "stride smaller than hpfw_gpu_mel_frames(n_samples)");
    if (n_clips > 65535) return fail(HPFW_E_INVALID, "more than 65535 clips in one call");
    HIP_TRY(hipSetDevice(h->device));
    if (n_clips == 0) return 0;
    HostTrip t;
    const int16_t *d_pcm = t.take<int16_t>((size_t)n_clips * n_samples * 2, pcm);
    int64_t *d_blk = t.take<int64_t>((size_t)n_clips * n_blk * 8);
    int *d_pos = t.take<int>((size_t)n_clips * nf * 4);
    int32_t *d_frames = t.take<int32_t>((size_t)n_clips * stride * 4, nullptr, -1, frames);
    int32_t *d_count = t.take<int32_t>((size_t)n_clips * 4, nullptr, -1, n_kept);
    return t.run(true, [&] {
        return ordered_call(h, nullptr, [&] {
            hpfw::launch_mel_kept_frames(d_pcm, n_samples, (int)n_clips, d_blk, d_pos, d_count, d_frames, stride, nullptr);
            return check_launch("mel kept frames");
        });
    });
}

// ---- voting search (AnnStorage semantics, exact neighbours) ------------------------------------
namespace {
constexpr int kVoteWin = 64, kVoteNn = 5;

// keys [n_win][5] of the windows of all queries, sorted per window; w_first[q] = first window of query q
int knn_windows_impl(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, std::vector<uint64_t> &keys,
                     std::vector<int64_t> &w_first)
{
    HIP_TRY(hipSetDevice(h->device));
    w_first.assign((size_t)n_q + 1, 0);
    std::vector<int64_t> w_start;
    for (int64_t q = 0; q < n_q; ++q) {
        if (q_off[q + 1] < q_off[q]) return fail(HPFW_E_INVALID, "q_off must be non-decreasing");
        const int64_t k = q_off[q + 1] - q_off[q];
        for (int64_t i = 0; i + kVoteWin <= k; ++i) w_start.push_back(q_off[q] - q_off[0] + i);
        w_first[(size_t)q + 1] = (int64_t)w_start.size();
    }
    const int64_t n_win = (int64_t)w_start.size();
    keys.assign((size_t)n_win * kVoteNn, ~0ull);
    const int64_t n_clips = (int64_t)h->index.db_off.size() - 1;
    int64_t n_max = 0;
    for (int64_t i = 0; i < n_clips; ++i) n_max = std::max(n_max, h->index.db_off[i + 1] - h->index.db_off[i]);
    if (n_win == 0 || n_max < kVoteWin) return 0;
    // one launch: groups of 32 windows along gridDim.y (at most 65535)
    if (n_win > (int64_t)65535 * 32) return fail(HPFW_E_UNSUPPORTED, "too many query windows in one call (limit 2097120)");
    return ordered_call(h, nullptr, [&] {
        if (int rc = upload_db_off(h, nullptr)) return rc;
        const int64_t total = q_off[n_q] - q_off[0];
        const int kt_pad = hpfw::hamming_mfma_kt_pad(kVoteWin);
        const size_t n_groups = (size_t)(n_win + 31) / 32;
        std::vector<uint64_t> slots((size_t)n_win * 8);
        HostTrip t;
        const uint64_t *d_q = t.take<uint64_t>((size_t)total * 8, q_hp + q_off[0]);
        const int64_t *d_ws = t.take<int64_t>((size_t)n_win * 8, w_start.data());
        uint64_t *d_slots = t.take<uint64_t>(slots.size() * 8, nullptr, 0xff, slots.data());
        void *d_qa = t.take<void>(n_groups * kt_pad * 1024);
        const int rc = t.run(false, [&] { // (the blocking copy of the slots waits for the kernels)
            hpfw::launch_expand_windows(d_q, d_ws, (int)n_win, kVoteWin, kt_pad, d_qa, nullptr);
            hpfw::launch_knn_windows(h->index.d_db.as<uint64_t>(), h->index.d_db_off.as<int64_t>(), (int)n_clips, (int)(n_max - kVoteWin + 1), d_qa,
                                     kt_pad, (int)n_win, kVoteWin, kVoteNn, d_slots, nullptr);
            return check_launch("knn_windows");
        });
        if (rc) return rc;
        for (int64_t w = 0; w < n_win; ++w) { // the device keeps the 5 smallest keys unsorted
            uint64_t *s5 = &slots[(size_t)w * 8];
            std::sort(s5, s5 + kVoteNn);
            for (int r = 0; r < kVoteNn; ++r) keys[(size_t)w * kVoteNn + r] = s5[r];
        }
        return 0;
    });
}
} // namespace

int hpfw_gpu_knn_windows(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, uint64_t *keys,
                         int64_t keys_cap)
{
    if (!h || !q_hp || !q_off || !keys || n_q < 0) return fail(HPFW_E_INVALID, "bad argument");
    std::vector<uint64_t> k;
    std::vector<int64_t> wf;
    int rc = knn_windows_impl(h, q_hp, q_off, n_q, k, wf);
    if (rc) return rc;
    if ((int64_t)k.size() > keys_cap) return fail(HPFW_E_INVALID, "keys buffer too small");
    std::memcpy(keys, k.data(), k.size() * 8);
    return 0;
}

int hpfw_gpu_search_votes(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, hpfw_vote *out)
{
    if (!h || !q_hp || !q_off || !out || n_q < 0) return fail(HPFW_E_INVALID, "bad argument");
    std::vector<uint64_t> keys;
    std::vector<int64_t> wf;
    int rc = knn_windows_impl(h, q_hp, q_off, n_q, keys, wf);
    if (rc) return rc;
    struct Bucket {
        int64_t clip, off;
        float cnt;
    };
    std::vector<Bucket> buckets;
    for (int64_t q = 0; q < n_q; ++q) {
        hpfw_vote best = {0xffffffffu, 0, 0, 0.0f, 0.0f}; // annoy_storage.h:43
        buckets.clear();
        for (int64_t w = wf[(size_t)q]; w < wf[(size_t)q + 1]; ++w) {
            const int64_t i = w - wf[(size_t)q];
            for (int r = 0; r < kVoteNn; ++r) {
                const uint64_t key = keys[(size_t)w * kVoteNn + r];
                if (key == ~0ull) continue;
                const uint64_t d = key >> 40;
                const int64_t pos = (int64_t)(key & (((uint64_t)1 << 40) - 1));
                const int64_t clip = (int64_t)(std::upper_bound(h->index.db_off.begin(), h->index.db_off.end(), pos) - h->index.db_off.begin()) - 1;
                const int64_t off = i - (pos - h->index.db_off[(size_t)clip]);
                size_t s = 0;
                while (s < buckets.size() && !(buckets[s].clip == clip && buckets[s].off == off)) ++s;
                if (s == buckets.size()) buckets.push_back({clip, off, 0.0f});
                buckets[s].cnt = (float)((double)buckets[s].cnt + 1.0 / (double)(float)(d + 1)); // :53
                if (buckets[s].cnt > best.cnt) {                                                  // :55-59
                    best.clip = h->index.clip_base + (uint32_t)clip;
                    best.offset = off;
                    best.cnt = buckets[s].cnt;
                }
            }
        }
        out[q] = best;
    }
    return 0;
}

// ---- voting search on the device (kernels: k_votes.hip, k_merge.hip) ----------------------------
namespace {
// The workspaces of one group of windows: the group size is this bound over an ESTIMATE of a window's bytes, so the bound is
// approximate.  The sort's own workspace is whatever hipcub asks for the group's events (a pair's copy plus histograms: the
// 60 + 132 bytes per window allowed for it below are not checked against it), every part is rounded up to 256 bytes, and a single
// query with more windows than a group is a group of its own, larger than the bound.
constexpr size_t kVotesBound = (size_t)256 << 20;
// what a window takes of them: its start, its row of the expanded image, 8 slots, 5 keys, and per event two sort keys, two
// values, the post-event value and the sort's own copy of a pair
constexpr size_t kVotesWindowBytes = 8 + 2560 + 64 + 40 + 5 * (8 + 8 + 4 + 4 + 4) + 5 * (8 + 4) + 132; // (132: the sort's histograms, alignment)
static_assert(kVotesWindowBytes == 3004, "the group size of DESIGN.md section 19");
constexpr int64_t kVotesGroupQueries = 65536;     // 16 bits of the sort key
constexpr int64_t kVotesLaunchWindows = (int64_t)65535 * 32;

// windows per group: the bound, or less where HPFW_VOTES_GROUP_WINDOWS says so (tests: several groups from small inputs)
int64_t votes_group_windows()
{
    int64_t n = (int64_t)(kVotesBound / kVotesWindowBytes);
    if (const char *e = std::getenv("HPFW_VOTES_GROUP_WINDOWS")) {
        const long long v = std::atoll(e);
        if (v >= 1) n = std::min<int64_t>(n, v);
    }
    return n;
}

struct VotesGroup {
    int64_t q0, n_q, w0, n_win; // whole queries [q0, q0 + n_q), their windows [w0, w0 + n_win)
};

// w_first [n_q + 1] -> groups of whole queries of at most `limit` windows (a query with more is a group of its own)
void votes_groups(const int64_t *wf, int64_t n_q, int64_t limit, std::vector<VotesGroup> &gs)
{
    gs.clear();
    for (int64_t q = 0; q < n_q;) {
        VotesGroup g = {q, 0, wf[q], 0};
        while (q < n_q && g.n_q < kVotesGroupQueries && (g.n_q == 0 || wf[q + 1] - g.w0 <= limit)) {
            g.n_win = wf[++q] - g.w0;
            ++g.n_q;
        }
        gs.push_back(g);
    }
}

int bit_length(uint64_t v)
{
    int b = 0;
    for (; v; v >>= 1) ++b;
    return b;
}

// what every group of a call shares: the groups, the key layout of the sort, the workspaces carved from d_votes_ws for the
// largest group, the call's tables on the device
struct VotesCall {
    std::vector<VotesGroup> groups;
    int64_t n_q = 0, stride = 1;
    int ubits = 0, qbits = 0;
    const int64_t *d_w_first = nullptr, *d_q_off = nullptr;
    int64_t *w_start = nullptr;
    void *qa = nullptr, *slots = nullptr, *temp = nullptr;
    uint64_t *keys = nullptr, *sort_keys = nullptr, *sorted_keys = nullptr;
    uint32_t *sort_vals = nullptr, *sorted_vals = nullptr;
    float *post = nullptr;
    size_t temp_bytes = 0;
};

// knn: the call scans the index (window starts, image, slots); own_keys: it keeps the keys itself; tally: it votes.
// pos_bound: above every position a key can hold.  Uploads w_first (and q_off) and waits for the copy.
int votes_prepare(hpfw_gpu *h, const int64_t *wf, const int64_t *q_off, int64_t n_q, bool knn, bool own_keys, bool tally, int64_t n_clips,
                  int64_t pos_bound, hipStream_t s, VotesCall &c)
{
    c.n_q = n_q;
    votes_groups(wf, n_q, votes_group_windows(), c.groups);
    int64_t win_max = 0, q_max = 1;
    for (int64_t q = 0; q < n_q; ++q) c.stride = std::max(c.stride, wf[q + 1] - wf[q]);
    for (const VotesGroup &g : c.groups) {
        win_max = std::max(win_max, g.n_win);
        q_max = std::max(q_max, g.n_q);
    }
    if (win_max > kVotesLaunchWindows) return fail(HPFW_E_UNSUPPORTED, "too many windows in one query (limit 2097120)");
    c.ubits = bit_length((uint64_t)pos_bound + (uint64_t)c.stride * (uint64_t)(n_clips + 1));
    c.qbits = bit_length((uint64_t)q_max - 1);
    if (tally && c.ubits + c.qbits > 64) return fail(HPFW_E_UNSUPPORTED, "voting search: the index and the query are too large for one sort key");
    const int64_t n_ev = win_max * 5;
    if (tally && n_ev) {
        c.temp_bytes = hpfw::vote_sort_temp_bytes(n_ev, c.ubits + c.qbits);
        if (!c.temp_bytes) return fail(HPFW_E_HIP, "voting search: the sort's workspace query failed");
    }
    const auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    const int kt_pad = hpfw::hamming_mfma_kt_pad(kVoteWin);
    const size_t b_ws = knn ? al((size_t)win_max * 8) : 0, b_qa = knn ? al((size_t)((win_max + 31) / 32) * kt_pad * 1024) : 0,
                 b_slots = knn ? al((size_t)win_max * 64) : 0, b_keys = own_keys ? al((size_t)n_ev * 8) : 0,
                 b_k = tally ? al((size_t)n_ev * 8) : 0, b_v = tally ? al((size_t)n_ev * 4) : 0, b_temp = tally ? al(c.temp_bytes) : 0;
    const size_t total = b_ws + b_qa + b_slots + b_keys + 2 * b_k + 3 * b_v + b_temp;
    if (int rc = ensure(h->index.d_votes_ws, std::max<size_t>(total, 256))) return rc;
    char *p = h->index.d_votes_ws.as<char>();
    const auto take = [&p](size_t b) {
        char *r = p;
        p += b;
        return (void *)r;
    };
    c.w_start = (int64_t *)take(b_ws);
    c.qa = take(b_qa);
    c.slots = take(b_slots);
    c.keys = (uint64_t *)take(b_keys);
    c.sort_keys = (uint64_t *)take(b_k);
    c.sorted_keys = (uint64_t *)take(b_k);
    c.sort_vals = (uint32_t *)take(b_v);
    c.sorted_vals = (uint32_t *)take(b_v);
    c.post = (float *)take(b_v);
    c.temp = take(b_temp);
    const size_t row = (size_t)(n_q + 1) * 8;
    if (int rc = ensure(h->index.d_votes_tab, 2 * row)) return rc;
    int64_t *tab = h->index.d_votes_tab.as<int64_t>();
    HIP_TRY(hipMemcpyAsync(tab, wf, row, hipMemcpyHostToDevice, s));
    if (q_off) HIP_TRY(hipMemcpyAsync(tab + n_q + 1, q_off, row, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s)); // the host arrays are the caller's, and the table is reused by the next call
    c.d_w_first = tab;
    c.d_q_off = tab + n_q + 1;
    return 0;
}

// the keys [n_win][5] of a group's windows against the handle's index, ascending per window
int votes_knn_group(hpfw_gpu *h, const VotesCall &c, const VotesGroup &g, const uint64_t *d_q_hp, int64_t n_clips, int64_t n_max,
                    uint64_t *d_keys, hipStream_t s)
{
    if (g.n_win == 0) return 0;
    if (n_clips == 0 || n_max < kVoteWin) { // no item of 64 hashprints: padding alone
        HIP_TRY(hipMemsetAsync(d_keys, 0xff, (size_t)g.n_win * kVoteNn * 8, s));
        return 0;
    }
    const int kt_pad = hpfw::hamming_mfma_kt_pad(kVoteWin);
    HIP_TRY(hipMemsetAsync(c.slots, 0xff, (size_t)g.n_win * 64, s));
    {
        Timed t(h, K_SCAN, s);
        hpfw::launch_window_starts(c.d_w_first + g.q0, c.d_q_off + g.q0, (int)g.n_q, g.w0, g.n_win, c.w_start, s);
        hpfw::launch_expand_windows(d_q_hp, c.w_start, (int)g.n_win, kVoteWin, kt_pad, c.qa, s);
        hpfw::launch_knn_windows(h->index.d_db.as<uint64_t>(), h->index.d_db_off.as<int64_t>(), (int)n_clips, (int)(n_max - kVoteWin + 1), c.qa,
                                 kt_pad, (int)g.n_win, kVoteWin, kVoteNn, c.slots, s);
    }
    if (int rc = check_launch("knn_windows")) return rc;
    {
        Timed t(h, K_TOPK, s);
        hpfw::launch_sort_knn_slots(c.slots, g.n_win, d_keys, s);
    }
    return check_launch("sort_knn_slots");
}

// the votes of a group's queries from its keys
int votes_tally_group(hpfw_gpu *h, const VotesCall &c, const VotesGroup &g, const uint64_t *d_keys, const int64_t *d_db_off, int64_t n_clips,
                      uint32_t clip_base, hpfw_vote *d_out, hipStream_t s)
{
    hpfw::VoteTallyArgs a = {};
    a.keys = d_keys;
    a.w_first = c.d_w_first + g.q0;
    a.w_base = g.w0;
    a.n_win = g.n_win;
    a.n_q = (int)g.n_q;
    a.db_off = d_db_off;
    a.n_clips = n_clips;
    a.clip_base = clip_base;
    a.stride = c.stride;
    a.ubits = c.ubits;
    a.qbits = c.qbits;
    a.sort_keys = c.sort_keys;
    a.sorted_keys = c.sorted_keys;
    a.sort_vals = c.sort_vals;
    a.sorted_vals = c.sorted_vals;
    a.post = c.post;
    a.out = d_out + g.q0;
    hipError_t e;
    {
        Timed t(h, K_TOPK, s);
        e = hpfw::launch_vote_tally(a, c.temp, c.temp_bytes, s);
    }
    if (e != hipSuccess) return fail(HPFW_E_HIP, std::string("vote tally: ") + hipGetErrorString(e));
    return check_launch("vote tally");
}

// w_first of the queries q_off describes; false where q_off decreases
bool votes_windows_of(const int64_t *q_off, int64_t n_q, std::vector<int64_t> &wf)
{
    wf.assign((size_t)n_q + 1, 0);
    for (int64_t q = 0; q < n_q; ++q) {
        const int64_t k = q_off[q + 1] - q_off[q];
        if (k < 0) return false;
        wf[(size_t)q + 1] = wf[(size_t)q] + std::max<int64_t>(k - (kVoteWin - 1), 0);
    }
    return true;
}

int64_t index_longest_clip(const hpfw_gpu *h)
{
    int64_t n_max = 0;
    for (size_t i = 0; i + 1 < h->index.db_off.size(); ++i) n_max = std::max(n_max, h->index.db_off[i + 1] - h->index.db_off[i]);
    return n_max;
}
} // namespace

int hpfw_gpu_knn_windows_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, uint64_t *d_keys, int64_t keys_cap,
                                void *stream)
{
    if (!h || !q_off || n_q < 0 || keys_cap < 0) return fail(HPFW_E_INVALID, "bad argument");
    std::vector<int64_t> wf;
    if (!votes_windows_of(q_off, n_q, wf)) return fail(HPFW_E_INVALID, "q_off must be non-decreasing");
    const int64_t n_win = wf.back();
    if (n_win * kVoteNn > keys_cap) return fail(HPFW_E_INVALID, "keys buffer too small");
    if (n_win > 0 && (!d_q_hp || !d_keys)) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        if (n_win == 0) return 0;
        const int64_t n_clips = (int64_t)h->index.db_off.size() - 1, n_max = index_longest_clip(h);
        int rc;
        if ((rc = upload_db_off(h, s))) return rc;
        VotesCall c;
        if ((rc = votes_prepare(h, wf.data(), q_off, n_q, true, false, false, n_clips, h->index.db_off.back(), s, c))) return rc;
        for (const VotesGroup &g : c.groups)
            if ((rc = votes_knn_group(h, c, g, d_q_hp, n_clips, n_max, d_keys + g.w0 * kVoteNn, s))) return rc;
        return 0;
    });
}

int hpfw_gpu_vote_windows_device(hpfw_gpu *h, const uint64_t *d_keys, const int64_t *w_first, int64_t n_q, const int64_t *d_db_off,
                                 int64_t n_clips, uint32_t clip_base, hpfw_vote *d_out, void *stream)
{
    if (!h || !w_first || n_q < 0 || n_clips < 0 || n_clips > 0xffffffffll || (n_q > 0 && !d_out) || (n_clips > 0 && !d_db_off))
        return fail(HPFW_E_INVALID, "bad argument");
    for (int64_t q = 0; q < n_q; ++q)
        if (w_first[q + 1] < w_first[q]) return fail(HPFW_E_INVALID, "w_first must be non-decreasing");
    if (w_first[n_q] > w_first[0] && !d_keys) return fail(HPFW_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        if (n_q == 0) return 0;
        std::vector<int64_t> wf((size_t)n_q + 1);
        for (int64_t q = 0; q <= n_q; ++q) wf[(size_t)q] = w_first[q] - w_first[0];
        int rc;
        VotesCall c;
        if ((rc = votes_prepare(h, wf.data(), nullptr, n_q, false, false, true, n_clips, (int64_t)1 << 40, s, c))) return rc;
        for (const VotesGroup &g : c.groups)
            if ((rc = votes_tally_group(h, c, g, d_keys + (w_first[0] + g.w0) * kVoteNn, d_db_off, n_clips, clip_base, d_out, s))) return rc;
        return 0;
    });
}

int hpfw_gpu_search_votes_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, hpfw_vote *d_out, void *stream)
{
    if (!h || !q_off || n_q < 0 || (n_q > 0 && !d_out)) return fail(HPFW_E_INVALID, "bad argument");
    std::vector<int64_t> wf;
    if (!votes_windows_of(q_off, n_q, wf)) return fail(HPFW_E_INVALID, "q_off must be non-decreasing");
    if (wf.back() > 0 && !d_q_hp) return fail(HPFW_E_INVALID, "null queries");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        if (n_q == 0) return 0;
        const int64_t n_clips = (int64_t)h->index.db_off.size() - 1, n_max = index_longest_clip(h);
        int rc;
        if ((rc = upload_db_off(h, s))) return rc;
        VotesCall c;
        if ((rc = votes_prepare(h, wf.data(), q_off, n_q, true, true, true, n_clips, h->index.db_off.back(), s, c))) return rc;
        for (const VotesGroup &g : c.groups) {
            if ((rc = votes_knn_group(h, c, g, d_q_hp, n_clips, n_max, c.keys, s))) return rc;
            if ((rc = votes_tally_group(h, c, g, c.keys, h->index.d_db_off.as<int64_t>(), n_clips, h->index.clip_base, d_out, s))) return rc;
        }
        return 0;
    });
}

int hpfw_gpu_merge_knn_device(hpfw_gpu *h, const uint64_t *d_in, const int64_t *pos_base, int n_shards, int64_t n_win, uint64_t *d_out,
                              void *stream)
{
    if (!h || !pos_base || n_shards < 1 || n_shards > 64 || n_win < 0 || (n_win > 0 && (!d_in || !d_out)))
        return fail(HPFW_E_INVALID, "bad argument");
    for (int i = 0; i < n_shards; ++i)
        if (pos_base[i] < 0 || pos_base[i] >= ((int64_t)1 << 40) || (i > 0 && pos_base[i] < pos_base[i - 1]))
            return fail(HPFW_E_INVALID, "pos_base must be non-negative, non-decreasing and below 2^40");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    return ordered_call(h, s, [&] {
        if (n_win == 0) return 0;
        {
            Timed t(h, K_TOPK, s);
            hpfw::launch_knn_merge_shards(d_in, pos_base, n_shards, n_win, d_out, s);
        }
        return check_launch("knn_merge_shards");
    });
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
