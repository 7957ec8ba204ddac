// dtw.hip -- the warped search (k_dtw.hip): pairs, top-k over the index or over the plain search's
// candidates, and the path of one pair.  Device forms on the caller's stream, host forms through the shared round trip.
#include "handle.h"

static_assert(sizeof(hpfw_dtw_hit) == 16 && offsetof(hpfw_dtw_hit, dist) == 0 && offsetof(hpfw_dtw_hit, clip) == 4 &&
                  offsetof(hpfw_dtw_hit, start) == 8 && offsetof(hpfw_dtw_hit, end) == 12,
              "the kernels write {dist, clip, start, end}");

namespace {

constexpr int64_t kGroupPairs = (int64_t)1 << 22; // pairs of one pass of a search: 64 MiB of hits, 32 MiB of table

// what can be refused of a set of queries without the handle; *k_max: the longest query
int dtw_check_queries(const void *h, const int64_t *q_off, int64_t n_q, const void *out, int64_t *k_max)
{
    if (!h || !q_off || !out) return fail(HPFW_E_INVALID, "null argument");
    if (n_q < 0) return fail(HPFW_E_INVALID, "n_q must not be negative");
    return check_q_off(q_off, n_q, k_max);
}

int dtw_check_pairs(const int32_t *pairs, int64_t n_pairs)
{
    if (n_pairs < 0) return fail(HPFW_E_INVALID, "n_pairs must not be negative");
    if (n_pairs > 0 && !pairs) return fail(HPFW_E_INVALID, "null pairs");
    for (int64_t p = 0; p < 2 * n_pairs; ++p)
        if (pairs[p] < 0) return fail(HPFW_E_INVALID, "pairs: a negative index (pair " + std::to_string(p / 2) + ")");
    return 0;
}

// ... and once the index is known
int dtw_check_pairs_index(const hpfw_gpu *h, const int32_t *pairs, int64_t n_pairs, int64_t n_q)
{
    const int64_t n_clips = (int64_t)h->index.db_off.size() - 1;
    for (int64_t p = 0; p < n_pairs; ++p)
        if (pairs[2 * p] >= n_q || pairs[2 * p + 1] >= n_clips)
            return fail(HPFW_E_INVALID, "pairs: an index at or above the number of queries or clips (pair " + std::to_string(p) + ")");
    return 0;
}

int dtw_check_search(int candidates, int k)
{
    if (k < 1 || k > 64) return fail(HPFW_E_INVALID, "k must be in 1..64");
    if (candidates != 0 && (candidates < k || candidates > 64)) return fail(HPFW_E_INVALID, "candidates must be 0 or in k..64");
    return 0;
}

// workgroups of a pairs launch and their boundary rows: at most 64 MiB of them
int dtw_slots(hpfw_gpu *h, int64_t n_pairs, int64_t k_max, int *slots)
{
    const int64_t cap = std::min<int64_t>(4096, std::max<int64_t>(256, ((int64_t)1 << 22) / std::max<int64_t>(k_max, 1)));
    *slots = (int)std::max<int64_t>(1, std::min(n_pairs, cap));
    return ensure(h->index.d_dtw_bnd, (size_t)*slots * std::max<int64_t>(k_max, 1) * sizeof(uint4));
}

hpfw::DtwArgs dtw_args(hpfw_gpu *h, const uint64_t *d_q_hp, int k_max)
{
    hpfw::DtwArgs a{};
    a.db = h->index.d_db.as<uint64_t>();
    a.db_off = h->index.d_db_off.as<int64_t>();
    a.q = d_q_hp;
    a.q_off = h->index.d_dtw_q_off.as<int64_t>();
    a.k_max = k_max;
    a.bnd = h->index.d_dtw_bnd.as<uint4>();
    return a;
}

// no clip may have 2^31 columns or more: starts and ends are int32
int dtw_check_index(hpfw_gpu *h)
{
    if (index_longest_clip(h) > 0x7fffffff) return fail(HPFW_E_UNSUPPORTED, "warped search: a clip of 2^31 hashprints or more");
    return 0;
}

int dtw_upload_q_off(hpfw_gpu *h, const int64_t *q_off, int64_t n_q, hipStream_t s)
{
    if (int rc = ensure(h->index.d_dtw_q_off, (size_t)(n_q + 1) * 8)) return rc;
    HIP_TRY(hipMemcpyAsync(h->index.d_dtw_q_off.get(), q_off, (size_t)(n_q + 1) * 8, hipMemcpyHostToDevice, s));
    return 0;
}

int dtw_pairs_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, const int32_t *pairs, int64_t n_pairs,
                     hpfw_dtw_hit *d_out, hipStream_t s)
{
    int64_t k_max = 0;
    if (int rc = dtw_check_queries(h, q_off, n_q, d_out, &k_max)) return rc;
    if (int rc = dtw_check_pairs(pairs, n_pairs)) return rc;
    if (int rc = dtw_check_pairs_index(h, pairs, n_pairs, n_q)) return rc;
    if (n_pairs == 0) return 0;
    if (q_off[n_q] > q_off[0] && !d_q_hp) return fail(HPFW_E_INVALID, "null queries");
    if (int rc = dtw_check_index(h)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    return ordered_call(h, s, [&] {
        int rc, slots;
        if ((rc = upload_db_off(h, s))) return rc;
        if ((rc = dtw_upload_q_off(h, q_off, n_q, s))) return rc;
        if ((rc = ensure(h->index.d_dtw_pairs, (size_t)n_pairs * 8))) return rc;
        HIP_TRY(hipMemcpyAsync(h->index.d_dtw_pairs.get(), pairs, (size_t)n_pairs * 8, hipMemcpyHostToDevice, s));
        if ((rc = dtw_slots(h, n_pairs, k_max, &slots))) return rc;
        hpfw::DtwArgs a = dtw_args(h, d_q_hp, (int)k_max);
        a.pairs = h->index.d_dtw_pairs.as<int32_t>();
        a.n_pairs = n_pairs;
        a.out = d_out;
        {
            Timed t(h, K_SCAN, s);
            hpfw::launch_dtw_pairs(a, slots, false, s);
        }
        if ((rc = check_launch("dtw_pairs"))) return rc;
        HIP_TRY(hipStreamSynchronize(s)); // (the caller's arrays have been read)
        return 0;
    });
}

int search_dtw_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int candidates, int k, hpfw_dtw_hit *d_out,
                      hipStream_t s)
{
    int64_t k_max = 0;
    if (int rc = dtw_check_queries(h, q_off, n_q, d_out, &k_max)) return rc;
    if (int rc = dtw_check_search(candidates, k)) return rc;
    if (n_q == 0) return 0;
    if (q_off[n_q] > q_off[0] && !d_q_hp) return fail(HPFW_E_INVALID, "null queries");
    if (int rc = dtw_check_index(h)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    return ordered_call(h, s, [&] {
        int rc, slots;
        const int64_t n_clips = (int64_t)h->index.db_off.size() - 1;
        if (n_clips > 0x7fffffff) return fail(HPFW_E_UNSUPPORTED, "warped search: too many clips");
        const uint32_t base = h->index.clip_base;
        if (n_clips > 0 && (rc = upload_db_off(h, s))) return rc;
        const int64_t per_q = candidates ? candidates : n_clips;
        const int64_t qgroup = std::min<int64_t>(std::max<int64_t>(kGroupPairs / std::max<int64_t>(per_q, 1), 1), 65536);
        if ((rc = ensure(h->index.d_dtw_hits, (size_t)std::max<int64_t>(std::min(qgroup, n_q) * per_q, 1) * sizeof(hpfw_dtw_hit)))) return rc;
        if ((rc = ensure(h->index.d_dtw_top, (size_t)std::min(qgroup, n_q) * std::max(candidates, k) * sizeof(hpfw_hit)))) return rc;
        if ((rc = dtw_upload_q_off(h, q_off, n_q, s))) return rc;
        for (int64_t g0 = 0; g0 < n_q; g0 += qgroup) {
            const int64_t ng = std::min(qgroup, n_q - g0), n_pairs = ng * per_q;
            hpfw_hit *d_top = h->index.d_dtw_top.as<hpfw_hit>();
            // the plain search's hits first (it works in buffers of its own)
            if (candidates && (rc = hpfw_gpu_search_topk_device(h, d_q_hp, q_off + g0, ng, candidates, d_top, s))) return rc;
            hpfw::DtwArgs a = dtw_args(h, d_q_hp, (int)k_max);
            a.q_first = g0;
            a.per_q = per_q;
            a.clip_base = base;
            a.cand = candidates ? d_top : nullptr;
            a.n_pairs = n_pairs;
            a.out = h->index.d_dtw_hits.get();
            if (!candidates && n_pairs) {
                if ((rc = ensure(h->index.d_best, (size_t)n_pairs * 8))) return rc;
                a.table = h->index.d_best.as<uint64_t>();
            }
            if (n_pairs) {
                if ((rc = dtw_slots(h, n_pairs, k_max, &slots))) return rc;
                a.bnd = h->index.d_dtw_bnd.as<uint4>();
                Timed t(h, K_SCAN, s);
                hpfw::launch_dtw_pairs(a, slots, false, s);
            }
            if ((rc = check_launch("dtw_pairs"))) return rc;
            Timed t(h, K_TOPK, s);
            if (candidates) {
                hpfw::launch_dtw_rank(a.out, ng, candidates, k, base, d_out + g0 * k, s);
            } else {
                if ((rc = search_topk_rows(h, a.table, (int)ng, n_clips, k, d_top, s))) return rc;
                hpfw::launch_dtw_finish(d_top, a.out, ng, k, per_q, base, d_out + g0 * k, s);
            }
            if ((rc = check_launch("dtw top-k"))) return rc;
        }
        return 0;
    });
}

// what the path call refuses without the handle
int dtw_check_path(const void *h, const void *q, int64_t k_q, int32_t clip, const void *path, const void *hit)
{
    if (!h || !path || !hit) return fail(HPFW_E_INVALID, "null argument");
    if (k_q < 0) return fail(HPFW_E_INVALID, "k_q must not be negative");
    if (k_q > 0 && !q) return fail(HPFW_E_INVALID, "null query");
    if (clip < 0) return fail(HPFW_E_INVALID, "a negative clip index");
    if (k_q > 16000) return fail(HPFW_E_UNSUPPORTED, "query longer than 16000 hashprints");
    return 0;
}

// ... and once the index is known; *n: the clip's columns
int dtw_check_path_index(const hpfw_gpu *h, int64_t k_q, int32_t clip, int64_t *n)
{
    const int64_t n_clips = (int64_t)h->index.db_off.size() - 1;
    if (clip >= n_clips) return fail(HPFW_E_INVALID, "a clip index at or above the number of clips");
    *n = h->index.db_off[(size_t)clip + 1] - h->index.db_off[(size_t)clip];
    if (*n > 0x7fffffff || k_q * *n > hpfw::kDtwPathCells)
        return fail(HPFW_E_UNSUPPORTED, "warped path: more than 2^31 cells (" + std::to_string(k_q) + " x " + std::to_string(*n) + ")");
    return 0;
}

int dtw_path_device(hpfw_gpu *h, const uint64_t *d_q_hp, int64_t k_q, int32_t clip, int32_t *d_path, hpfw_dtw_hit *d_hit, hipStream_t s)
{
    if (int rc = dtw_check_path(h, d_q_hp, k_q, clip, d_path, d_hit)) return rc;
    int64_t n = 0;
    if (int rc = dtw_check_path_index(h, k_q, clip, &n)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    return ordered_call(h, s, [&] {
        int rc, slots;
        if ((rc = upload_db_off(h, s))) return rc;
        const int64_t q_off[2] = {0, k_q};
        const int32_t pair[2] = {0, clip};
        if ((rc = dtw_upload_q_off(h, q_off, 1, s))) return rc;
        if ((rc = ensure(h->index.d_dtw_pairs, 8))) return rc;
        HIP_TRY(hipMemcpyAsync(h->index.d_dtw_pairs.get(), pair, 8, hipMemcpyHostToDevice, s));
        const int64_t n_blocks = std::max<int64_t>((n + hpfw::kDtwBlock - 1) / hpfw::kDtwBlock, 1);
        if ((rc = ensure(h->index.d_dtw_choices, (size_t)std::max<int64_t>(k_q, 1) * n_blocks * 64 * sizeof(uint16_t)))) return rc;
        if ((rc = dtw_slots(h, 1, k_q, &slots))) return rc;
        hpfw::DtwArgs a = dtw_args(h, d_q_hp, (int)k_q);
        a.pairs = h->index.d_dtw_pairs.as<int32_t>();
        a.n_pairs = 1;
        a.choices = h->index.d_dtw_choices.as<uint16_t>();
        a.out = d_hit;
        {
            Timed t(h, K_SCAN, s);
            hpfw::launch_dtw_pairs(a, 1, true, s);
            if (k_q > 0) hpfw::launch_dtw_backtrack(a.choices, (int)k_q, (int)n_blocks, d_hit, d_path, s);
        }
        if ((rc = check_launch("dtw_path"))) return rc;
        HIP_TRY(hipStreamSynchronize(s)); // (q_off and the pair live on this frame)
        return 0;
    });
}

} // namespace

extern "C" {

int hpfw_gpu_dtw_geometry(int32_t *strip, int32_t *block)
{
    if (!strip || !block) return fail(HPFW_E_INVALID, "null argument");
    *strip = hpfw::kDtwStrip;
    *block = hpfw::kDtwBlock;
    return 0;
}

int hpfw_gpu_dtw_pairs_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, const int32_t *pairs, int64_t n_pairs,
                              hpfw_dtw_hit *d_out, void *stream)
{
    return dtw_pairs_device(h, d_q_hp, q_off, n_q, pairs, n_pairs, d_out, (hipStream_t)stream);
}

int hpfw_gpu_dtw_pairs(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, const int32_t *pairs, int64_t n_pairs,
                       hpfw_dtw_hit *out)
{
    int64_t k_max = 0;
    if (int rc = dtw_check_queries(h, q_off, n_q, out, &k_max)) return rc;
    if (int rc = dtw_check_pairs(pairs, n_pairs)) return rc;
    if (n_q > 0 && q_off[n_q] > q_off[0] && !q_hp) return fail(HPFW_E_INVALID, "null queries");
    if (int rc = dtw_check_pairs_index(h, pairs, n_pairs, n_q)) return rc;
    if (n_pairs == 0) return 0;
    HIP_TRY(hipSetDevice(h->device));
    return search_round_trip(q_hp, q_off, n_q, n_pairs, out, [&](const uint64_t *d_q, const int64_t *rel, hpfw_dtw_hit *d_out) {
        return dtw_pairs_device(h, d_q, rel, n_q, pairs, n_pairs, d_out, nullptr);
    });
}

int hpfw_gpu_search_dtw_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int candidates, int k,
                               hpfw_dtw_hit *d_out, void *stream)
{
    return search_dtw_device(h, d_q_hp, q_off, n_q, candidates, k, d_out, (hipStream_t)stream);
}

int hpfw_gpu_search_dtw(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int candidates, int k, hpfw_dtw_hit *out)
{
    int64_t k_max = 0;
    if (int rc = dtw_check_queries(h, q_off, n_q, out, &k_max)) return rc;
    if (int rc = dtw_check_search(candidates, k)) return rc;
    if (n_q > 0 && q_off[n_q] > q_off[0] && !q_hp) return fail(HPFW_E_INVALID, "null queries");
    HIP_TRY(hipSetDevice(h->device));
    if (n_q == 0) return 0;
    return search_round_trip(q_hp, q_off, n_q, n_q * k, out, [&](const uint64_t *d_q, const int64_t *rel, hpfw_dtw_hit *d_out) {
        return search_dtw_device(h, d_q, rel, n_q, candidates, k, d_out, nullptr);
    });
}

int hpfw_gpu_dtw_path_device(hpfw_gpu *h, const uint64_t *d_q_hp, int64_t k_q, int32_t clip, int32_t *d_path, hpfw_dtw_hit *d_hit,
                             void *stream)
{
    return dtw_path_device(h, d_q_hp, k_q, clip, d_path, d_hit, (hipStream_t)stream);
}

int hpfw_gpu_dtw_path(hpfw_gpu *h, const uint64_t *q_hp, int64_t k_q, int32_t clip, int32_t *path, hpfw_dtw_hit *hit)
{
    if (int rc = dtw_check_path(h, q_hp, k_q, clip, path, hit)) return rc;
    int64_t n = 0;
    if (int rc = dtw_check_path_index(h, k_q, clip, &n)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    HostTrip t;
    const uint64_t *d_q = t.take<uint64_t>((size_t)std::max<int64_t>(k_q, 1) * 8, k_q ? q_hp : nullptr);
    int32_t *d_path = t.take<int32_t>((size_t)std::max<int64_t>(k_q, 1) * 4, nullptr, 0xff, nullptr);
    hpfw_dtw_hit *d_hit = t.take<hpfw_dtw_hit>(sizeof(hpfw_dtw_hit), nullptr, -1, hit);
    int rc = t.run(true, [&] { return dtw_path_device(h, d_q, k_q, clip, d_path, d_hit, nullptr); });
    if (!rc && k_q > 0 && hipMemcpy(path, d_path, (size_t)k_q * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(HPFW_E_HIP, "D2H copy failed");
    return rc;
}

} // extern "C"
