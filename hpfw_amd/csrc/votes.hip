// votes.hip -- the voting search (AnnStorage semantics, exact neighbours; kernels: k_votes.hip,
// k_merge.hip): the neighbour scan and the tally on the device in groups of windows, the host functions as round trips over
// them, and the merge of the shards' neighbour lists.
#include "handle.h"

namespace {
constexpr int kVoteWin = 64, kVoteNn = 5;

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
} // namespace

extern "C" {

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

// ---- the host functions: round trips over the device calls on the null stream, as hpfw_gpu_search_topk is over its own ----
int hpfw_gpu_knn_windows(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, uint64_t *keys,
                         int64_t keys_cap)
{
    if (!h || !q_hp || !q_off || !keys || n_q < 0) return fail(HPFW_E_INVALID, "bad argument");
    std::vector<int64_t> wf;
    if (!votes_windows_of(q_off, n_q, wf)) return fail(HPFW_E_INVALID, "q_off must be non-decreasing");
    const int64_t n_keys = wf.back() * kVoteNn;
    if (n_keys > keys_cap) return fail(HPFW_E_INVALID, "keys buffer too small");
    HIP_TRY(hipSetDevice(h->device));
    if (n_keys == 0) return 0;
    return search_round_trip(q_hp, q_off, n_q, n_keys, keys, [&](const uint64_t *d_q, const int64_t *rel, uint64_t *d_keys) {
        return hpfw_gpu_knn_windows_device(h, d_q, rel, n_q, d_keys, n_keys, nullptr);
    });
}

int hpfw_gpu_search_votes(hpfw_gpu *h, const uint64_t *q_hp, const int64_t *q_off, int64_t n_q, hpfw_vote *out)
{
    if (!h || !q_hp || !q_off || !out || n_q < 0) return fail(HPFW_E_INVALID, "bad argument");
    std::vector<int64_t> wf;
    if (!votes_windows_of(q_off, n_q, wf)) return fail(HPFW_E_INVALID, "q_off must be non-decreasing");
    HIP_TRY(hipSetDevice(h->device));
    if (n_q == 0) return 0;
    return search_round_trip(q_hp, q_off, n_q, n_q, out, [&](const uint64_t *d_q, const int64_t *rel, hpfw_vote *d_out) {
        return hpfw_gpu_search_votes_device(h, d_q, rel, n_q, d_out, nullptr);
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

} // extern "C"
