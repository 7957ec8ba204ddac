// selfjoin.hip -- the index joined with itself (k_selfjoin.hip) and with recordings that are not in it
// (section 23): the entry points, their checks and the passes over the row groups.
#include "handle.h"

// what can be refused without the handle's contents, before a device is touched
static int selfjoin_check(const void *h, int min_overlap, int rate_num, int rate_den, const void *out, int64_t cap, const void *count)
{
    if (!h) return fail(HPFW_E_INVALID, "null handle");
    if (rate_den < 1 || rate_den > 1024) return fail(HPFW_E_INVALID, "selfjoin: rate_den must be in 1..1024");
    if (rate_num < 0 || rate_num > 64 * rate_den) return fail(HPFW_E_INVALID, "selfjoin: rate_num must be in 0..64 rate_den");
    if (min_overlap < 1 || min_overlap > hpfw::kSelfjoinMaxLen) return fail(HPFW_E_INVALID, "selfjoin: min_overlap must be in 1..262143");
    if (cap < 0) return fail(HPFW_E_INVALID, "selfjoin: cap must not be negative");
    if (cap > 0 && !out) return fail(HPFW_E_INVALID, "selfjoin: null out");
    if (!count) return fail(HPFW_E_INVALID, "selfjoin: null count");
    return 0;
}

static int selfjoin_length_check(const hpfw_gpu *h)
{
    if (index_longest_clip(h) > hpfw::kSelfjoinMaxLen)
        return fail(HPFW_E_UNSUPPORTED, "selfjoin: a recording of the index has more than 262143 hashprints");
    return 0;
}

// what the join refuses of its recordings without the handle's contents; *longest: the longest of them
static int join_check(const void *x_hp, const int64_t *x_off, int64_t n_x, int among_new, int64_t *longest)
{
    if (!x_off) return fail(HPFW_E_INVALID, "join: null x_off");
    if (n_x < 0) return fail(HPFW_E_INVALID, "join: n_x must not be negative");
    if (among_new < 0 || among_new > 1) return fail(HPFW_E_INVALID, "join: among_new must be 0 or 1");
    *longest = 0;
    for (int64_t i = 0; i < n_x; ++i) {
        if (x_off[i + 1] < x_off[i]) return fail(HPFW_E_INVALID, "join: x_off must be non-decreasing");
        *longest = std::max(*longest, x_off[i + 1] - x_off[i]);
    }
    if (x_off[n_x] > x_off[0] && !x_hp) return fail(HPFW_E_INVALID, "join: null hashprints");
    if (*longest > hpfw::kSelfjoinMaxLen) return fail(HPFW_E_UNSUPPORTED, "join: a recording has more than 262143 hashprints");
    return 0;
}

// the recordings outside the index that a join brings (null: the self-join)
struct JoinSide {
    const uint64_t *d_hp;
    const int64_t *off; // host, [n + 1]
    int64_t n, longest;
    int among_new;
};

// The passes of either join, inside ordered_call.  The rows are the 32-row groups of the index's slots (the join: then the
// externals), a pass's table is [its rows][columns][splits] with the index's clips as columns (the join: the externals).
// The plan of the passes is join_plan.h's, their loop join_run_passes below, shared with the local self-join (localjoin.hip).
static int join_passes(hpfw_gpu *h, hipStream_t s, const JoinSide *x, int min_overlap, int rate_num, int rate_den, hpfw_dup_pair *d_out,
                       int64_t cap, int64_t *d_count)
{
    int rc;
    HIP_TRY(hipMemsetAsync(d_count, 0, 8, s));
    const int64_t n_index = (int64_t)h->index.db_off.size() - 1;
    const int64_t n_clips = n_index + (x ? x->n : 0);                           // the rows
    const int64_t n_cols = x ? x->n : n_index, col0 = x ? n_index : 0;
    const int64_t n_max = std::max(index_longest_clip(h), x ? x->longest : 0); // the longest row
    if (n_clips < 2 || n_cols < 1 || (x ? x->longest : n_max) < min_overlap) return 0; // no pair has a candidate
    if ((rc = upload_db_off(h, s))) return rc;
    const bool popc = std::getenv("HPFW_SELFJOIN_POPC") != nullptr;
    // the pairs (row group, b): b above the group's first row (the join: an external, hpfw_gpu_join_plan); no pairs: an empty
    // index joined without among_new.  The table stays at or below 1 GiB
    const int64_t n_groups = ((x && !x->among_new ? n_index : n_clips) + 31) / 32;
    const hpfw::JoinPlan plan = hpfw::join_plan(
        n_groups,
        [&](int64_t g) { return x ? hpfw::join_group_pairs(n_index, x->n, x->among_new, g) : hpfw::selfjoin_group_pairs(n_clips, g); }, n_cols,
        n_max, min_overlap, hpfw::kSelfjoinChunk, 16, env_forced_splits("HPFW_SELFJOIN_SPLITS"), env_table_kb("HPFW_SELFJOIN_TABLE_KB"));
    if (x && plan.pairs) { // (join_run_passes waits for the stream: the caller's offsets have been read)
        if ((rc = ensure(h->index.d_sj_x_off, (size_t)(x->n + 1) * 8))) return rc;
        HIP_TRY(hipMemcpyAsync(h->index.d_sj_x_off.get(), x->off, (size_t)(x->n + 1) * 8, hipMemcpyHostToDevice, s));
    }
    const uint64_t *db = h->index.d_db.as<uint64_t>();
    const int64_t *db_off = h->index.d_db_off.as<int64_t>();
    return join_run_passes(
        h, s, plan, n_groups, n_cols, 16, "selfjoin scan",
        [&](const JoinPass &p) {
            if (x)
                hpfw::launch_join_scan(popc, db, db_off, (int)n_index, x->d_hp, h->index.d_sj_x_off.as<int64_t>(), (int)x->n, x->among_new, p.g0,
                                       p.n_groups, p.d_pair_first, p.n_pairs, min_overlap, p.splits, p.d_tab, s);
            else
                hpfw::launch_selfjoin_scan(popc, db, db_off, (int)n_clips, p.g0, p.n_groups, p.d_pair_first, p.n_pairs, min_overlap, p.splits,
                                           p.d_tab, s);
        },
        "selfjoin select",
        [&](const JoinPass &p) {
            hpfw::launch_selfjoin_select(p.d_tab, (int)n_cols, (int)col0, p.splits, 32 * p.g0, 32 * p.n_groups, (uint32_t)rate_num,
                                         (uint32_t)rate_den, p.d_row_count, p.d_row_first, h->index.clip_base, d_out, cap, d_count, s);
        });
}

int join_run_passes(hpfw_gpu *h, hipStream_t s, const hpfw::JoinPlan &plan, int64_t n_groups, int64_t n_cols, size_t entry_bytes,
                    const char *scan_what, const std::function<void(const JoinPass &)> &scan, const char *select_what,
                    const std::function<void(const JoinPass &)> &select)
{
    int rc;
    if (plan.pairs == 0) return 0;
    const int64_t pass_groups = plan.pass_groups;
    if ((rc = ensure(h->index.d_sj_pairs, plan.pair_first.size() * 4))) return rc;
    HIP_TRY(hipMemcpyAsync(h->index.d_sj_pairs.get(), plan.pair_first.data(), plan.pair_first.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s)); // (pair_first has been read)
    if ((rc = ensure(h->index.d_sj_tab, (size_t)(32 * pass_groups * n_cols * plan.splits) * entry_bytes))) return rc;
    if ((rc = ensure(h->index.d_sj_rows, (size_t)(32 * pass_groups) * (8 + 4)))) return rc;
    int64_t *d_row_first = h->index.d_sj_rows.as<int64_t>();
    int *d_row_count = reinterpret_cast<int *>(d_row_first + 32 * pass_groups);
    for (int64_t p = 0; p < plan.n_passes; ++p) {
        const int64_t g0 = p * pass_groups, ng = std::min(pass_groups, n_groups - g0);
        JoinPass pass = {};
        pass.g0 = (int)g0;
        pass.n_groups = (int)ng;
        pass.d_pair_first = h->index.d_sj_pairs.as<uint32_t>() + p * (pass_groups + 1);
        pass.n_pairs = plan.pass(p)[ng];
        pass.splits = (int)plan.splits;
        pass.d_tab = h->index.d_sj_tab.get();
        pass.d_row_count = d_row_count;
        pass.d_row_first = d_row_first;
        if (pass.n_pairs == 0) continue; // (the last group is the last clip alone)
        HIP_TRY(hipMemsetAsync(pass.d_tab, 0xff, (size_t)(32 * ng * n_cols * plan.splits) * entry_bytes, s));
        {
            Timed t(h, K_SCAN, s);
            scan(pass);
        }
        if ((rc = check_launch(scan_what))) return rc;
        {
            Timed t(h, K_TOPK, s);
            select(pass);
        }
        if ((rc = check_launch(select_what))) return rc;
    }
    return 0;
}

extern "C" {

int hpfw_gpu_selfjoin_geometry(int32_t *slice, int32_t *chunk)
{
    if (!slice || !chunk) return fail(HPFW_E_INVALID, "null argument");
    *slice = hpfw::kSelfjoinSlice;
    *chunk = hpfw::kSelfjoinChunk;
    return 0;
}

int hpfw_gpu_index_selfjoin_device(hpfw_gpu *h, int min_overlap, int rate_num, int rate_den, hpfw_dup_pair *d_out, int64_t cap,
                                   int64_t *d_count, void *stream)
{
    if (int rc = selfjoin_check(h, min_overlap, rate_num, rate_den, d_out, cap, d_count)) return rc;
    if (int rc = selfjoin_length_check(h)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_clips = (int64_t)h->index.db_off.size() - 1;
    if (n_clips * 32 > ((int64_t)1 << 26)) return fail(HPFW_E_UNSUPPORTED, "selfjoin: more than 2097152 clips");
    HIP_TRY(hipSetDevice(h->device));
    return ordered_call(h, s, [&] { return join_passes(h, s, nullptr, min_overlap, rate_num, rate_den, d_out, cap, d_count); });
}

int hpfw_gpu_index_selfjoin(hpfw_gpu *h, int min_overlap, int rate_num, int rate_den, hpfw_dup_pair *out, int64_t cap, int64_t *count)
{
    if (int rc = selfjoin_check(h, min_overlap, rate_num, rate_den, out, cap, count)) return rc;
    if (int rc = selfjoin_length_check(h)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    HostTrip t;
    hpfw_dup_pair *d_out = cap ? t.take<hpfw_dup_pair>((size_t)cap * sizeof(hpfw_dup_pair), nullptr, 0, out) : nullptr;
    int64_t *d_count = t.take<int64_t>(8, nullptr, -1, count);
    return t.run(true, [&] { return hpfw_gpu_index_selfjoin_device(h, min_overlap, rate_num, rate_den, d_out, cap, d_count, nullptr); });
}

int hpfw_gpu_join_plan(int64_t n_clips, int64_t n_x, int among_new, int64_t group0, int64_t n_groups, uint32_t *pair_first)
{
    if (n_clips < 0 || n_x < 0 || group0 < 0 || n_groups < 0) return fail(HPFW_E_INVALID, "join plan: a negative count");
    if (among_new < 0 || among_new > 1) return fail(HPFW_E_INVALID, "join: among_new must be 0 or 1");
    if (!pair_first) return fail(HPFW_E_INVALID, "null argument");
    if (n_clips + n_x > ((int64_t)1 << 21)) return fail(HPFW_E_UNSUPPORTED, "join: more than 2097152 recordings");
    if (!hpfw::join_pair_first(group0, n_groups, [&](int64_t g) { return hpfw::join_group_pairs(n_clips, n_x, among_new, g); }, pair_first))
        return fail(HPFW_E_UNSUPPORTED, "join plan: more than 2^32 - 1 pairs in a pass");
    return 0;
}

int hpfw_gpu_index_join_device(hpfw_gpu *h, const uint64_t *d_x_hp, const int64_t *x_off, int64_t n_x, int among_new, int min_overlap,
                               int rate_num, int rate_den, hpfw_dup_pair *d_out, int64_t cap, int64_t *d_count, void *stream)
{
    JoinSide x = {d_x_hp, x_off, n_x, 0, among_new};
    if (int rc = selfjoin_check(h, min_overlap, rate_num, rate_den, d_out, cap, d_count)) return rc;
    if (int rc = join_check(d_x_hp, x_off, n_x, among_new, &x.longest)) return rc;
    if (int rc = selfjoin_length_check(h)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_index = (int64_t)h->index.db_off.size() - 1;
    if (n_index + n_x > ((int64_t)1 << 21)) return fail(HPFW_E_UNSUPPORTED, "join: more than 2097152 recordings in the index and the batch");
    HIP_TRY(hipSetDevice(h->device));
    return ordered_call(h, s, [&] { return join_passes(h, s, &x, min_overlap, rate_num, rate_den, d_out, cap, d_count); });
}

int hpfw_gpu_index_join(hpfw_gpu *h, const uint64_t *x_hp, const int64_t *x_off, int64_t n_x, int among_new, int min_overlap, int rate_num,
                        int rate_den, hpfw_dup_pair *out, int64_t cap, int64_t *count)
{
    int64_t longest = 0;
    if (int rc = selfjoin_check(h, min_overlap, rate_num, rate_den, out, cap, count)) return rc;
    if (int rc = join_check(x_hp, x_off, n_x, among_new, &longest)) return rc;
    if (int rc = selfjoin_length_check(h)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    const int64_t total = x_off[n_x] - x_off[0];
    std::vector<int64_t> rel((size_t)n_x + 1);
    for (int64_t i = 0; i <= n_x; ++i) rel[(size_t)i] = x_off[i] - x_off[0];
    HostTrip t;
    const uint64_t *d_x = t.take<uint64_t>((size_t)std::max<int64_t>(total, 1) * 8, total ? x_hp + x_off[0] : nullptr);
    hpfw_dup_pair *d_out = cap ? t.take<hpfw_dup_pair>((size_t)cap * sizeof(hpfw_dup_pair), nullptr, 0, out) : nullptr;
    int64_t *d_count = t.take<int64_t>(8, nullptr, -1, count);
    return t.run(true, [&] {
        return hpfw_gpu_index_join_device(h, d_x, rel.data(), n_x, among_new, min_overlap, rate_num, rate_den, d_out, cap, d_count, nullptr);
    });
}

} // extern "C"
