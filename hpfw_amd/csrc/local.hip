// local.hip -- the local search (k_search_local.hip): per query the k clips with the best-scoring run
// of consecutive hashprints on any diagonal, and the run's ends.  Device form on the caller's stream, host form through the
// shared round trip.
#include "handle.h"

static_assert(sizeof(hpfw_local_hit) == 24 && offsetof(hpfw_local_hit, score) == 0 && offsetof(hpfw_local_hit, clip) == 4 &&
                  offsetof(hpfw_local_hit, lag) == 8 && offsetof(hpfw_local_hit, q_start) == 12 && offsetof(hpfw_local_hit, length) == 16 &&
                  offsetof(hpfw_local_hit, dist) == 20,
              "the kernels write {score, clip, lag, q_start, length, dist}");

namespace {

// what can be refused without the handle, before anything runs; *k_max: the longest query
int local_check(const void *h, const int64_t *q_off, int64_t n_q, int max_rate, int k, const void *out, int64_t *k_max)
{
    if (!h || !q_off || !out || n_q < 0) return fail(HPFW_E_INVALID, "bad argument");
    if (k < 1 || k > 64) return fail(HPFW_E_INVALID, "k must be in 1..64");
    if (max_rate < 1 || max_rate > 31) return fail(HPFW_E_INVALID, "max_rate must be in 1..31");
    return check_q_off(q_off, n_q, k_max);
}

int search_local_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int max_rate, int k, hpfw_local_hit *d_out,
                        hipStream_t s)
{
    int64_t k_max = 0;
    if (int rc = local_check(h, q_off, n_q, max_rate, k, d_out, &k_max)) return rc;
    if (n_q > 0 && !d_q_hp) return fail(HPFW_E_INVALID, "null queries");
    const int64_t n_clips = (int64_t)h->index.db_off.size() - 1;
    const int64_t n_max = index_longest_clip(h);
    if (n_max > 0x7fffffff - 2 * hpfw::kLocalLagBias) return fail(HPFW_E_UNSUPPORTED, "local search: a clip of 2^31 hashprints or so");
    HIP_TRY(hipSetDevice(h->device));
    return ordered_call(h, s, [&] {
        if (n_q == 0) return 0;
        int rc;
        if (n_clips == 0 || n_max == 0 || k_max == 0) { // nothing to compare: every slot is "none"
            hpfw::launch_local_ends(nullptr, nullptr, nullptr, nullptr, nullptr, n_q, k, max_rate, h->index.clip_base, d_out, nullptr, s);
            return check_launch("local_ends");
        }
        if ((rc = ensure(h->index.d_local_flag, 4))) return rc;
        HIP_TRY(hipMemsetAsync(h->index.d_local_flag.get(), 0, 4, s));
        const bool mfma = hpfw::search_on_matrix_cores(std::getenv("HPFW_LOCAL_POPC") != nullptr, hpfw::hamming_mfma_lds_bytes((int)k_max));
        // lags 1 - k_max .. n_max - 1 in chunks
        const int64_t chunks = (n_max + k_max - 2) / hpfw::kLocalChunk + 1;
        if (n_clips * chunks > 0x7fffffff) return fail(HPFW_E_UNSUPPORTED, "local search: too many clips");
        const int64_t qgroup = hpfw::search_group_queries(n_q, n_clips, hpfw::kLocalTableEntries, hpfw::kPopcGridQueries, 8,
                                                          env_table_kb("HPFW_LOCAL_TABLE_KB"));
        if ((rc = ensure(h->index.d_local_top, (size_t)qgroup * k * sizeof(hpfw_hit)))) return rc;
        const uint64_t *db = h->index.d_db.as<uint64_t>();
        rc = search_run_groups(
            h, s, d_q_hp, q_off, n_q, k_max, qgroup, mfma, h->index.d_best, (size_t)n_clips * 8,
            {{K_SCAN, "local scan", true,
              [&](const QueryGroup &g) {
                  const int64_t *db_off = h->index.d_db_off.as<int64_t>();
                  uint64_t *d_best = h->index.d_best.as<uint64_t>();
                  if (mfma)
                      hpfw::launch_local_mfma(db, db_off, (int)n_clips, g.d_q_off, g.ng, g.d_qa, g.kt_pad, g.d_gk, (int)k_max, max_rate, (int)chunks, d_best, s);
                  else
                      hpfw::launch_local_popc(db, db_off, (int)n_clips, d_q_hp, g.d_q_off, g.ng, max_rate, (int)chunks, d_best, s);
                  return 0;
              }},
             {K_TOPK, "local top-k", false, [&](const QueryGroup &g) {
                  void *d_top = h->index.d_local_top.get();
                  if (int rc2 = search_topk_rows(h, h->index.d_best.as<uint64_t>(), g.ng, n_clips, k, d_top, s)) return rc2;
                  hpfw::launch_local_ends(d_top, db, h->index.d_db_off.as<int64_t>(), d_q_hp, g.d_q_off, g.ng, k, max_rate, h->index.clip_base,
                                          d_out + g.g0 * k, h->index.d_local_flag.as<unsigned>(), s);
                  return 0;
              }}});
        if (rc) return rc;
        // the walk of every winner gave the scan's score (and q_off has been read)
        unsigned disagree = 0;
        HIP_TRY(hipMemcpyAsync(&disagree, h->index.d_local_flag.get(), 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (disagree) return fail(HPFW_E_HIP, "local search: scan and walk disagree on " + std::to_string(disagree) + " scores");
        return 0;
    });
}

} // namespace

extern "C" {

int hpfw_gpu_search_local_device(hpfw_gpu *h, const uint64_t *d_q_hp, const int64_t *q_off, int64_t n_q, int max_rate, int k,
                                 hpfw_local_hit *d_out, void *stream)
{
    return search_local_device(h, d_q_hp, q_off, n_q, max_rate, k, d_out, (hipStream_t)stream);
}

int hpfw_gpu_search_local(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, int max_rate, int k, hpfw_local_hit *out)
{
    int64_t k_max = 0;
    if (int rc = local_check(h, q_off, n_q, max_rate, k, out, &k_max)) return rc;
    if (n_q > 0 && q_off[n_q] > q_off[0] && !q_hp) return fail(HPFW_E_INVALID, "null queries");
    HIP_TRY(hipSetDevice(h->device));
    if (n_q == 0) return 0;
    return search_round_trip(q_hp, q_off, n_q, n_q * k, out, [&](const uint64_t *d_q, const int64_t *rel, hpfw_local_hit *d_out) {
        return search_local_device(h, d_q, rel, n_q, max_rate, k, d_out, nullptr);
    });
}

} // extern "C"
