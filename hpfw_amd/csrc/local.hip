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
    *k_max = 0;
    for (int64_t i = 0; i < n_q; ++i) {
        if (q_off[i + 1] < q_off[i]) return fail(HPFW_E_INVALID, "q_off must be non-decreasing");
        *k_max = std::max(*k_max, q_off[i + 1] - q_off[i]);
    }
    if (*k_max > 16000) return fail(HPFW_E_UNSUPPORTED, "query longer than 16000 hashprints");
    return 0;
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
        if ((rc = upload_db_off(h, s))) return rc;
        if ((rc = ensure(h->index.d_q_off, (size_t)(n_q + 1) * 8))) return rc;
        HIP_TRY(hipMemcpyAsync(h->index.d_q_off.get(), q_off, (size_t)(n_q + 1) * 8, hipMemcpyHostToDevice, s));
        if ((rc = ensure(h->index.d_local_flag, 4))) return rc;
        HIP_TRY(hipMemsetAsync(h->index.d_local_flag.get(), 0, 4, s));
        // The scan runs on the matrix cores unless the window does not fit the LDS (the bound of the plain search) or
        // HPFW_LOCAL_POPC asks for the xor/popcount kernel.
        const bool mfma = !std::getenv("HPFW_LOCAL_POPC") && hpfw::hamming_mfma_lds_bytes((int)k_max) <= 160 * 1024;
        // lags 1 - k_max .. n_max - 1 in chunks
        const int64_t chunks = (n_max + k_max - 2) / hpfw::kLocalChunk + 1;
        if (n_clips * chunks > 0x7fffffff) return fail(HPFW_E_UNSUPPORTED, "local search: too many clips");
        // queries are processed in groups so the table stays below 512 MiB
        int64_t qgroup = std::max<int64_t>(32, ((int64_t)1 << 26) / n_clips / 32 * 32);
        qgroup = std::min<int64_t>(qgroup, (n_q + 31) / 32 * 32);
        qgroup = std::min<int64_t>(qgroup, 65504); // the popcount kernel puts one query per gridDim.y
        if ((rc = ensure(h->index.d_best, (size_t)qgroup * n_clips * 8))) return rc;
        if ((rc = ensure(h->index.d_local_top, (size_t)qgroup * k * sizeof(hpfw_hit)))) return rc;
        const int kt_pad = hpfw::hamming_mfma_kt_pad((int)k_max);
        if (mfma) {
            if ((rc = ensure(h->index.d_qa, (size_t)(qgroup / 32) * kt_pad * 1024))) return rc;
            if ((rc = ensure(h->index.d_gk, (size_t)(qgroup / 32) * 4))) return rc;
        }
        std::vector<int> gk;
        const uint64_t *db = h->index.d_db.as<uint64_t>();
        const int64_t *db_off = h->index.d_db_off.as<int64_t>();
        uint64_t *d_best = h->index.d_best.as<uint64_t>();
        for (int64_t g0 = 0; g0 < n_q; g0 += qgroup) {
            const int ng = (int)std::min<int64_t>(qgroup, n_q - g0);
            const int64_t *d_q_off = h->index.d_q_off.as<int64_t>() + g0;
            HIP_TRY(hipMemsetAsync(d_best, 0xff, (size_t)ng * n_clips * 8, s));
            if (mfma) {
                gk.assign((size_t)(ng + 31) / 32, 0);
                for (int i = 0; i < ng; ++i) gk[(size_t)i / 32] = std::max(gk[(size_t)i / 32], (int)(q_off[g0 + i + 1] - q_off[g0 + i]));
                HIP_TRY(hipMemcpyAsync(h->index.d_gk.get(), gk.data(), gk.size() * 4, hipMemcpyHostToDevice, s));
                HIP_TRY(hipStreamSynchronize(s)); // gk is reused by the next group of queries
                Timed t(h, K_SCAN, s);
                hpfw::launch_expand_queries(d_q_hp, d_q_off, ng, kt_pad, h->index.d_qa.get(), s);
                hpfw::launch_local_mfma(db, db_off, (int)n_clips, d_q_off, ng, h->index.d_qa.get(), kt_pad, h->index.d_gk.as<int>(), (int)k_max,
                                        max_rate, (int)chunks, d_best, s);
            } else {
                Timed t(h, K_SCAN, s);
                hpfw::launch_local_popc(db, db_off, (int)n_clips, d_q_hp, d_q_off, ng, max_rate, (int)chunks, d_best, s);
            }
            if ((rc = check_launch("local scan"))) return rc;
            {
                Timed t(h, K_TOPK, s);
                void *d_top = h->index.d_local_top.get();
                if (n_clips >= 16384 && ng <= 64) { // (as the plain search chooses)
                    if ((rc = ensure(h->index.d_topk_scratch, hpfw::topk_scratch_bytes(ng, k)))) return rc;
                    hpfw::launch_topk_two_step(d_best, ng, (int)n_clips, k, h->index.clip_base, h->index.d_topk_scratch.get(), d_top, s);
                } else {
                    hpfw::launch_topk(d_best, ng, (int)n_clips, k, h->index.clip_base, d_top, s);
                }
                hpfw::launch_local_ends(d_top, db, db_off, d_q_hp, d_q_off, ng, k, max_rate, h->index.clip_base, d_out + g0 * k,
                                        h->index.d_local_flag.as<unsigned>(), s);
            }
            if ((rc = check_launch("local top-k"))) return rc;
        }
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
