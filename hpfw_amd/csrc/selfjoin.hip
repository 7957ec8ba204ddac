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
    // the pairs (row group, b): b above the group's first row (the join: an external, hpfw_gpu_join_plan)
    const int64_t n_groups = ((x && !x->among_new ? n_index : n_clips) + 31) / 32;
    auto group_pairs = [&](int64_t g) {
        return x ? hpfw::join_group_pairs(n_index, x->n, x->among_new, g) : std::max<int64_t>(n_clips - 32 * g - 1, 0);
    };
    int64_t pairs = 0;
    for (int64_t g = 0; g < n_groups; ++g) pairs += group_pairs(g);
    if (pairs == 0) return 0; // (an empty index joined without among_new)
    // the chunks of a pair go to `splits` workgroups
    const int64_t chunks = (2 * n_max - 2 * min_overlap) / hpfw::kSelfjoinChunk + 1;
    int64_t splits = overlap_splits(chunks, pairs, "HPFW_SELFJOIN_SPLITS");
    // row groups are processed in passes so that the table stays at or below 1 GiB (2^26 entries; HPFW_SELFJOIN_TABLE_KB:
    // that many KiB, at least one row group's, for tests of more than one pass)
    int64_t budget = (int64_t)1 << 26;
    if (const char *e = std::getenv("HPFW_SELFJOIN_TABLE_KB")) budget = std::min(std::max<int64_t>(std::atoll(e) * 64, 32 * n_cols), budget);
    splits = std::min(splits, budget / (32 * n_cols));
    const int64_t pass_groups = std::min(n_groups, budget / (32 * n_cols * splits));
    const int64_t n_passes = (n_groups + pass_groups - 1) / pass_groups;
    // every pass numbers its pairs from 0: pair_first [pass_groups + 1] per pass
    std::vector<uint32_t> pair_first((size_t)(n_passes * (pass_groups + 1)), 0);
    for (int64_t p = 0; p < n_passes; ++p) {
        uint32_t *pf = pair_first.data() + p * (pass_groups + 1);
        for (int64_t i = 0; i < pass_groups; ++i) pf[i + 1] = pf[i] + (uint32_t)(p * pass_groups + i < n_groups ? group_pairs(p * pass_groups + i) : 0);
    }
    if ((rc = ensure(h->index.d_sj_pairs, pair_first.size() * 4))) return rc;
    HIP_TRY(hipMemcpyAsync(h->index.d_sj_pairs.get(), pair_first.data(), pair_first.size() * 4, hipMemcpyHostToDevice, s));
    if (x) {
        if ((rc = ensure(h->index.d_sj_x_off, (size_t)(x->n + 1) * 8))) return rc;
        HIP_TRY(hipMemcpyAsync(h->index.d_sj_x_off.get(), x->off, (size_t)(x->n + 1) * 8, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipStreamSynchronize(s)); // (pair_first and the caller's offsets have been read)
    const size_t tab_bytes = (size_t)(32 * pass_groups * n_cols * splits) * 16;
    if ((rc = ensure(h->index.d_sj_tab, tab_bytes))) return rc;
    if ((rc = ensure(h->index.d_sj_rows, (size_t)(32 * pass_groups) * (8 + 4)))) return rc;
    int64_t *d_row_first = h->index.d_sj_rows.as<int64_t>();
    int *d_row_count = reinterpret_cast<int *>(d_row_first + 32 * pass_groups);
    for (int64_t p = 0; p < n_passes; ++p) {
        const int64_t g0 = p * pass_groups, ng = std::min(pass_groups, n_groups - g0);
        const uint32_t *d_pf = h->index.d_sj_pairs.as<uint32_t>() + p * (pass_groups + 1);
        const uint32_t n_pairs = pair_first[(size_t)(p * (pass_groups + 1) + ng)];
        if (n_pairs == 0) continue; // (the last group is the last clip alone)
        HIP_TRY(hipMemsetAsync(h->index.d_sj_tab.get(), 0xff, (size_t)(32 * ng * n_cols * splits) * 16, s));
        {
            Timed t(h, K_SCAN, s);
            if (x)
                hpfw::launch_join_scan(popc, h->index.d_db.as<uint64_t>(), h->index.d_db_off.as<int64_t>(), (int)n_index, x->d_hp,
                                       h->index.d_sj_x_off.as<int64_t>(), (int)x->n, x->among_new, (int)g0, (int)ng, d_pf, n_pairs, min_overlap,
                                       (int)splits, h->index.d_sj_tab.get(), s);
            else
                hpfw::launch_selfjoin_scan(popc, h->index.d_db.as<uint64_t>(), h->index.d_db_off.as<int64_t>(), (int)n_clips, (int)g0, (int)ng,
                                           d_pf, n_pairs, min_overlap, (int)splits, h->index.d_sj_tab.get(), s);
        }
        if ((rc = check_launch("selfjoin scan"))) return rc;
        {
            Timed t(h, K_TOPK, s);
            hpfw::launch_selfjoin_select(h->index.d_sj_tab.get(), (int)n_cols, (int)col0, (int)splits, (int)(32 * g0), (int)(32 * ng),
                                         (uint32_t)rate_num, (uint32_t)rate_den, d_row_count, d_row_first, h->index.clip_base, d_out, cap, d_count, s);
        }
        if ((rc = check_launch("selfjoin select"))) return rc;
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
    pair_first[0] = 0;
    for (int64_t i = 0; i < n_groups; ++i) {
        const int64_t next = (int64_t)pair_first[i] + hpfw::join_group_pairs(n_clips, n_x, among_new, group0 + i);
        if (next > (int64_t)UINT32_MAX) return fail(HPFW_E_UNSUPPORTED, "join plan: more than 2^32 - 1 pairs in a pass");
        pair_first[i + 1] = (uint32_t)next;
    }
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
