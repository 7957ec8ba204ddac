// localjoin.hip -- the local self-join (k_localjoin.hip): the passages that recordings of the index
// share.  The entry points, their checks and the passes over the row groups, which are the catalogue self-join's: the plan
// is join_plan.h's and the loop selfjoin.hip's join_run_passes.  The calls of a handle are ordered, so this join works in
// that join's table, rows and pair numbering.
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
    // the pairs (row group, b): b above the group's first row (n_clips >= 2: group 0 has one).  The table stays at or below
    // 512 MiB
    const int64_t n_groups = (n_clips + 31) / 32;
    const hpfw::JoinPlan plan =
        hpfw::join_plan(n_groups, [&](int64_t g) { return hpfw::selfjoin_group_pairs(n_clips, g); }, n_clips, n_max, min_len, hpfw::kSelfjoinChunk, 8,
                        env_forced_splits("HPFW_LOCALJOIN_SPLITS"), env_table_kb("HPFW_LOCALJOIN_TABLE_KB"));
    if ((rc = ensure(h->index.d_local_flag, 4))) return rc;
    HIP_TRY(hipMemsetAsync(h->index.d_local_flag.get(), 0, 4, s));
    const uint64_t *db = h->index.d_db.as<uint64_t>();
    const int64_t *db_off = h->index.d_db_off.as<int64_t>();
    rc = join_run_passes(
        h, s, plan, n_groups, n_clips, 8, "localjoin scan",
        [&](const JoinPass &p) {
            hpfw::launch_localjoin_scan(popc, db, db_off, (int)n_clips, p.g0, p.n_groups, p.d_pair_first, p.n_pairs, (int)min_len, max_rate,
                                        p.splits, p.d_tab, s);
        },
        "localjoin select",
        [&](const JoinPass &p) {
            hpfw::launch_localjoin_select(p.d_tab, (int)n_clips, p.splits, 32 * p.g0, 32 * p.n_groups, min_score, p.d_row_count, p.d_row_first,
                                          h->index.clip_base, d_out, cap, d_count, s);
        });
    if (rc || cap == 0) return rc;
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
