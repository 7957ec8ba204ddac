// localjoin.hip -- the local self-join (k_localjoin.hip): the passages that recordings of the index
// share.  The entry points, their checks and the passes over the row groups, which are the catalogue self-join's
// (selfjoin.hip): the calls of a handle are ordered, so this join works in that join's table, rows and pair numbering.
#include "handle.h"

static_assert(sizeof(hpfw_passage_pair) == 32 && offsetof(hpfw_passage_pair, a) == 0 && offsetof(hpfw_passage_pair, b) == 4 &&
                  offsetof(hpfw_passage_pair, score) == 8 && offsetof(hpfw_passage_pair, lag) == 12 &&
                  offsetof(hpfw_passage_pair, a_start) == 16 && offsetof(hpfw_passage_pair, length) == 20 &&
                  offsetof(hpfw_passage_pair, dist) == 24 && offsetof(hpfw_passage_pair, pad) == 28,
              "the kernels write {a, b, score, lag, a_start, length, dist, pad}");

namespace {

// what can be refused without the handle's contents, before a device is touched
int localjoin_check(const void *h, int max_rate, int min_score, const void *out, int64_t cap, const void *count)
{
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    if (max_rate < 1 || max_rate > 31) return fail(HPFW_E_INVALID, "localjoin: max_rate must be in 1..31");
    if (min_score < 1) return fail(HPFW_E_INVALID, "localjoin: min_score must be at least 1");
    if (cap < 0) return fail(HPFW_E_INVALID, "localjoin: cap must not be negative");
    if (cap > 0 && !out) return fail(HPFW_E_INVALID, "localjoin: null out");
    if (!count) return fail(HPFW_E_INVALID, "localjoin: null count");
    return 0;
}

int localjoin_length_check(const hpfw_gpu *h)
{
    if (index_longest_clip(h) > hpfw::kSelfjoinMaxLen)
        return fail(HPFW_E_UNSUPPORTED, "localjoin: a recording of the index has more than 262143 hashprints");
    return 0;
}

// the passes, inside ordered_call: a pass's table is [its rows][the index's clips][splits]
int localjoin_passes(hpfw_gpu *h, hipStream_t s, int max_rate, int min_score, hpfw_passage_pair *d_out, int64_t cap, int64_t *d_count)
{
    int rc;
    HIP_TRY(hipMemsetAsync(d_count, 0, 8, s));
    const int64_t n_clips = (int64_t)h->index.db_off.size() - 1;
    const int64_t n_max = index_longest_clip(h);
    // a run that scores min_score has at least min_len positions: the shortest overlap of a lag worth scanning
    const int64_t min_len = ((int64_t)min_score + max_rate - 1) / max_rate;
    if (n_clips < 2 || n_max < min_len) return 0; // no pair has a run to report
    if ((rc = upload_db_off(h, s))) return rc;
    const bool popc = std::getenv("HPFW_LOCALJOIN_POPC") != nullptr;
    // the pairs (row group, b): b above the group's first row
    const int64_t n_groups = (n_clips + 31) / 32;
    auto group_pairs = [&](int64_t g) { return std::max<int64_t>(n_clips - 32 * g - 1, 0); };
    // the chunks of a pair go to `splits` workgroups
    const int64_t chunks = (2 * n_max - 2 * min_len) / hpfw::kSelfjoinChunk + 1;
    int64_t pairs = 0;
    for (int64_t g = 0; g < n_groups; ++g) pairs += group_pairs(g);
    int64_t splits = overlap_splits(chunks, pairs, "HPFW_LOCALJOIN_SPLITS");
    // row groups are processed in passes so that the table stays at or below 2^26 entries (512 MiB; HPFW_LOCALJOIN_TABLE_KB:
    // that many KiB, at least one row group's, for tests of more than one pass)
    int64_t budget = (int64_t)1 << 26;
    if (const char *e = std::getenv("HPFW_LOCALJOIN_TABLE_KB")) budget = std::min(std::max<int64_t>(std::atoll(e) * 128, 32 * n_clips), budget);
    splits = std::min(splits, budget / (32 * n_clips));
    const int64_t pass_groups = std::min(n_groups, budget / (32 * n_clips * splits));
    const int64_t n_passes = (n_groups + pass_groups - 1) / pass_groups;
    // every pass numbers its pairs from 0: pair_first [pass_groups + 1] per pass
    std::vector<uint32_t> pair_first((size_t)(n_passes * (pass_groups + 1)), 0);
    for (int64_t p = 0; p < n_passes; ++p) {
        uint32_t *pf = pair_first.data() + p * (pass_groups + 1);
        for (int64_t i = 0; i < pass_groups; ++i) pf[i + 1] = pf[i] + (uint32_t)(p * pass_groups + i < n_groups ? group_pairs(p * pass_groups + i) : 0);
    }
    if ((rc = ensure(h->index.d_sj_pairs, pair_first.size() * 4))) return rc;
    HIP_TRY(hipMemcpyAsync(h->index.d_sj_pairs.get(), pair_first.data(), pair_first.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s)); // (pair_first has been read)
    if ((rc = ensure(h->index.d_sj_tab, (size_t)(32 * pass_groups * n_clips * splits) * 8))) return rc;
    if ((rc = ensure(h->index.d_sj_rows, (size_t)(32 * pass_groups) * (8 + 4)))) return rc;
    if ((rc = ensure(h->index.d_local_flag, 4))) return rc;
    HIP_TRY(hipMemsetAsync(h->index.d_local_flag.get(), 0, 4, s));
    int64_t *d_row_first = h->index.d_sj_rows.as<int64_t>();
    int *d_row_count = reinterpret_cast<int *>(d_row_first + 32 * pass_groups);
    const uint64_t *db = h->index.d_db.as<uint64_t>();
    const int64_t *db_off = h->index.d_db_off.as<int64_t>();
    for (int64_t p = 0; p < n_passes; ++p) {
        const int64_t g0 = p * pass_groups, ng = std::min(pass_groups, n_groups - g0);
        const uint32_t *d_pf = h->index.d_sj_pairs.as<uint32_t>() + p * (pass_groups + 1);
        const uint32_t n_pairs = pair_first[(size_t)(p * (pass_groups + 1) + ng)];
        if (n_pairs == 0) continue; // (the last group is the last clip alone)
        HIP_TRY(hipMemsetAsync(h->index.d_sj_tab.get(), 0xff, (size_t)(32 * ng * n_clips * splits) * 8, s));
        {
            Timed t(h, K_SCAN, s);
            hpfw::launch_localjoin_scan(popc, db, db_off, (int)n_clips, (int)g0, (int)ng, d_pf, n_pairs, (int)min_len, max_rate, (int)splits,
                                        h->index.d_sj_tab.get(), s);
        }
        if ((rc = check_launch("localjoin scan"))) return rc;
        {
            Timed t(h, K_TOPK, s);
            hpfw::launch_localjoin_select(h->index.d_sj_tab.get(), (int)n_clips, (int)splits, (int)(32 * g0), (int)(32 * ng), min_score,
                                          d_row_count, d_row_first, h->index.clip_base, d_out, cap, d_count, s);
        }
        if ((rc = check_launch("localjoin select"))) return rc;
    }
    if (cap == 0) return 0;
    {
        Timed t(h, K_TOPK, s);
        hpfw::launch_localjoin_ends(db, db_off, max_rate, h->index.clip_base, d_out, cap, d_count, h->index.d_local_flag.as<unsigned>(), s);
    }
    if ((rc = check_launch("localjoin ends"))) return rc;
    // the walk of every written pair gave the scan's score
    unsigned disagree = 0;
    HIP_TRY(hipMemcpyAsync(&disagree, h->index.d_local_flag.get(), 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (disagree) return fail(HPFW_E_HIP, "localjoin: scan and walk disagree on " + std::to_string(disagree) + " scores");
    return 0;
}

} // namespace

extern "C" {

int hpfw_gpu_localjoin_geometry(int32_t *slice, int32_t *chunk)
{
    if (!slice || !chunk) return fail(HPFW_E_INVALID, "null argument");
    *slice = hpfw::kSelfjoinSlice;
    *chunk = hpfw::kSelfjoinChunk;
    return 0;
}

int hpfw_gpu_index_localjoin_device(hpfw_gpu *h, int max_rate, int min_score, hpfw_passage_pair *d_out, int64_t cap, int64_t *d_count,
                                    void *stream)
{
    if (int rc = localjoin_check(h, max_rate, min_score, d_out, cap, d_count)) return rc;
    if (int rc = localjoin_length_check(h)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_clips = (int64_t)h->index.db_off.size() - 1;
    if (n_clips * 32 > ((int64_t)1 << 26)) return fail(HPFW_E_UNSUPPORTED, "localjoin: more than 2097152 clips");
    HIP_TRY(hipSetDevice(h->device));
    return ordered_call(h, s, [&] { return localjoin_passes(h, s, max_rate, min_score, d_out, cap, d_count); });
}

int hpfw_gpu_index_localjoin(hpfw_gpu *h, int max_rate, int min_score, hpfw_passage_pair *out, int64_t cap, int64_t *count)
{
    if (int rc = localjoin_check(h, max_rate, min_score, out, cap, count)) return rc;
    if (int rc = localjoin_length_check(h)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    HostTrip t;
    hpfw_passage_pair *d_out = cap ? t.take<hpfw_passage_pair>((size_t)cap * sizeof(hpfw_passage_pair), nullptr, 0, out) : nullptr;
    int64_t *d_count = t.take<int64_t>(8, nullptr, -1, count);
    return t.run(true, [&] { return hpfw_gpu_index_localjoin_device(h, max_rate, min_score, d_out, cap, d_count, nullptr); });
}

} // extern "C"
