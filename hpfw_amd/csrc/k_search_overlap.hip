// k_search_overlap.hip -- the overlap search (include/hpfw_gpu.h): a query may overhang either end of
// a clip, and every alignment is rated by its mismatches per overlapping hashprint.
//
// The rule -- which lags are candidates and how they are ordered -- its comparison, a workgroup's best, the fold of the
// splits, the expansion to fp4 and the end of a chunk on either route are in overlap_rule.h, shared with the joins
// (k_selfjoin.hip).  This file instantiates OverlapSearchRule: dist <= 64 L, L <= 16000, 24-bit products below 2^34.
//
// (a) overlap_mfma_kernel is the scan of query_scan.h with the clip's window zero-filled on both sides: with hashprint bits as
// fp4 +-1 and fp4 0 outside the query and outside the clip, the accumulator of (query row, lag) is 64 L - 2 dist.  The lags of
// a clip start at min_overlap - (the group's longest query) and end at n - min_overlap; the window is restaged per chunk.
// (b) overlap_popc_kernel computes the same by xor/popcount: queries whose window does not fit the LDS, and the second
// opinion on the device (HPFW_OVERLAP_POPC).
//
// Both write one 16-byte entry {dist, L, lag, 0} per (query, clip, split) with ordinary stores: a clip's chunks are dealt
// round robin to `splits` workgroups, each of which owns its entry (no atomics, nothing depends on the order workgroups
// run in).  overlap_select_kernel folds the splits and picks the k best clips per query.
#include "kernels.h"
#include "query_scan.h"

namespace hpfw {

extern __shared__ __align__(16) unsigned char smem_raw[];

namespace {
using Rule = OverlapSearchRule;
static_assert(kOverlapChunk == Rule::kChunk, "a candidate's lag inside the chunk takes 10 bits");
constexpr unsigned kNoDist = Rule::kNoDist; // the "none" of OvPick below
} // namespace

struct OverlapArgs {
    const uint64_t *db;
    const int64_t *db_off;
    int n_clips;
    const uint64_t *q;    // the call's hashprints (xor/popcount kernel)
    const int64_t *q_off; // [n_q + 1] (device), this launch's first query at q_off[0]
    int n_q;
    const v4i *qa;        // expanded queries of this launch (expand_queries_kernel's image)
    int kt_pad;
    const int *gk;        // [2 g]: longest query of group g
    int min_overlap, splits;
    uint4 *tab;           // [n_q][n_clips][splits], every byte preset to 0xff
};

__global__ __launch_bounds__(kScanThreads, 4) void overlap_mfma_kernel(OverlapArgs a)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_lane = lane & 31, h = lane >> 5;
    const int clip = blockIdx.x / a.splits, split = blockIdx.x - clip * a.splits, g = blockIdx.y;
    const int64_t r0 = a.db_off[clip];
    const int n = (int)(a.db_off[clip + 1] - r0);
    const int kt = a.gk[2 * g], mo = a.min_overlap;
    if (n < mo || kt < mo) return; // no row of the group has a candidate in this clip
    const int d_lo = mo - kt, d_hi = n - mo;
    const int n_wg_chunks = (d_hi - d_lo) / kScanWgLags + 1;

    const int win = kScanWgLags + kt;
    const ScanLds l = scan_lds(smem_raw, win);
    int *kq_s = l.len;                                // lengths of the group's queries (0: no candidate)
    uint2 *red = reinterpret_cast<uint2 *>(l.A);      // [8 waves][32 queries], over the A operand once the sums are done

    if (tid < 32) {
        const int qi = g * 32 + tid;
        int k = 0;
        if (qi < a.n_q) k = (int)(a.q_off[qi + 1] - a.q_off[qi]);
        kq_s[tid] = k >= mo ? k : 0;
    }
    const v4i *qa = a.qa + (int64_t)g * a.kt_pad * 64;
    const v4i *bp = l.B + h * win + wave * kScanWaveLags + n_lane;
    Rule::Best best; // (threads below 32)

    for (int wc = split; wc < n_wg_chunks; wc += a.splits) {
        const int d0 = d_lo + wc * kScanWgLags;
        __syncthreads(); // the chunk before this one has read its window and its candidates
        scan_stage_window(l.B, win, a.db, r0, n, d0, tid);
        f32x16 acc[kScanTiles];
#pragma unroll
        for (int t = 0; t < kScanTiles; ++t) acc[t] = f32x16{0};
        // a wave whose 128 lags all lie past n - min_overlap (the clip's last chunk) is not live
        scan_walk(qa, l.A, bp, kt, d0 + wave * kScanWaveLags <= d_hi, tid, lane,
                  [&](const v4i *ap, const v4i *bj, int j) { scan_products(acc, ap, bj, j); });
        // the chunk's candidates go over the A operand, the best of each query row to its thread's `best`
        Rule::tile_epilogue(acc, kq_s, n, mo, d0, red, best, tid, wave, n_lane, h);
    }
    if (tid < 32 && g * 32 + tid < a.n_q)
        best.store(a.tab + ((int64_t)(g * 32 + tid) * a.n_clips + clip) * a.splits + split);
}

// one workgroup per (query, clip, split): a thread takes four lags of a chunk and walks their overlaps
__global__ __launch_bounds__(256) void overlap_popc_kernel(OverlapArgs a)
{
    __shared__ uint2 red[4];
    const int tid = threadIdx.x;
    const int clip = blockIdx.x / a.splits, split = blockIdx.x - clip * a.splits, qi = blockIdx.y;
    const int64_t r0 = a.db_off[clip], q0 = a.q_off[qi];
    const int n = (int)(a.db_off[clip + 1] - r0), k = (int)(a.q_off[qi + 1] - q0), mo = a.min_overlap;
    if (n < mo || k < mo) return;
    const uint64_t *q = a.q + q0, *r = a.db + r0;
    const int d_lo = mo - k, d_hi = n - mo;
    const int n_wg_chunks = (d_hi - d_lo) / kScanWgLags + 1;
    Rule::Best best; // (thread 0)
    for (int wc = split; wc < n_wg_chunks; wc += a.splits) {
        const int d0 = d_lo + wc * kScanWgLags;
        Rule::popc_chunk<false>(q, k, r, n, mo, d0, d_hi, red, best, tid); // d_lo <= d <= d_hi: every lag overlaps min_overlap
    }
    if (tid == 0) best.store(a.tab + ((int64_t)qi * a.n_clips + clip) * a.splits + split);
}

namespace {
struct OverlapHitDev {
    uint32_t dist, clip;
    int32_t lag;
    uint32_t overlap;
};

// clips of one query: dist / L, then larger L, then the smaller clip id.  "none" is (kNoDist, 1, 0x7fffffff).
struct OvPick {
    unsigned dist, L, clip;
};
__device__ __forceinline__ bool ov_pick_less(const OvPick &x, const OvPick &y)
{
    const uint64_t a = Rule::mul(x.dist, y.L), b = Rule::mul(y.dist, x.L);
    return a < b || (a == b && (x.L > y.L || (x.L == y.L && x.clip < y.clip)));
}
} // namespace

// one workgroup per query: the splits of every clip folded into the clip's first entry, then k rounds of "the smallest
// clip above the one before"
__global__ __launch_bounds__(256) void overlap_select_kernel(uint4 *__restrict__ tab, int n_clips, int splits,
                                                             const int32_t *__restrict__ exclude, int k, uint32_t clip_base,
                                                             OverlapHitDev *__restrict__ out)
{
    __shared__ OvPick red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, qi = blockIdx.x;
    uint4 *row = tab + (int64_t)qi * n_clips * splits;
    const int ex = exclude ? exclude[qi] : -1;
    if (splits > 1) {
        for (int c = tid; c < n_clips; c += 256) {
            uint4 b = row[(int64_t)c * splits];
            for (int s = 1; s < splits; ++s) Rule::fold(b, row[(int64_t)c * splits + s]);
            row[(int64_t)c * splits] = b;
        }
        __syncthreads();
    }
    const OvPick none = {kNoDist, 1u, 0x7fffffffu};
    OvPick prev = none;
    for (int r = 0; r < k; ++r) {
        OvPick mine = none;
        if (r == 0 || prev.dist != kNoDist) {
            for (int c = tid; c < n_clips; c += 256) {
                const uint4 e = row[(int64_t)c * splits];
                if (overlap_no_entry(e) || c == ex) continue;
                const OvPick p = {e.x, e.y, (unsigned)c};
                if ((r == 0 || ov_pick_less(prev, p)) && ov_pick_less(p, mine)) mine = p;
            }
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const OvPick o = {(unsigned)__shfl_xor((int)mine.dist, s), (unsigned)__shfl_xor((int)mine.L, s),
                              (unsigned)__shfl_xor((int)mine.clip, s)};
            if (ov_pick_less(o, mine)) mine = o;
        }
        __syncthreads(); // (the round before has been read)
        if (lane == 0) red[wave] = mine;
        __syncthreads();
        OvPick sel = red[0];
        for (int w = 1; w < 4; ++w)
            if (ov_pick_less(red[w], sel)) sel = red[w];
        if (tid == 0) {
            OverlapHitDev hit = {0xffffffffu, 0xffffffffu, 0, 0u};
            if (sel.dist != kNoDist) hit = {sel.dist, clip_base + sel.clip, (int32_t)row[(int64_t)sel.clip * splits].z, sel.L};
            out[(int64_t)qi * k + r] = hit;
        }
        prev = sel;
    }
}

void launch_overlap_mfma(const uint64_t *d_db, const int64_t *d_db_off, int n_clips, const int64_t *d_q_off, int n_q, const void *d_qa,
                         int kt_pad, const int *d_gk, int k_max, int min_overlap, int splits, void *d_tab, hipStream_t s)
{
    static PerDeviceOnce attr_set;
    scan_allow_lds(attr_set, {reinterpret_cast<const void *>(overlap_mfma_kernel)});
    OverlapArgs a = {};
    a.db = d_db;
    a.db_off = d_db_off;
    a.n_clips = n_clips;
    a.q_off = d_q_off;
    a.n_q = n_q;
    a.qa = reinterpret_cast<const v4i *>(d_qa);
    a.kt_pad = kt_pad;
    a.gk = d_gk;
    a.min_overlap = min_overlap;
    a.splits = splits;
    a.tab = reinterpret_cast<uint4 *>(d_tab);
    const dim3 grid((unsigned)n_clips * (unsigned)splits, (unsigned)((n_q + 31) / 32));
    hipLaunchKernelGGL(overlap_mfma_kernel, grid, dim3(kScanThreads), query_scan_lds_bytes(k_max), s, a);
}

void launch_overlap_popc(const uint64_t *d_db, const int64_t *d_db_off, int n_clips, const uint64_t *d_q, const int64_t *d_q_off, int n_q,
                         int min_overlap, int splits, void *d_tab, hipStream_t s)
{
    OverlapArgs a = {};
    a.db = d_db;
    a.db_off = d_db_off;
    a.n_clips = n_clips;
    a.q = d_q;
    a.q_off = d_q_off;
    a.n_q = n_q;
    a.min_overlap = min_overlap;
    a.splits = splits;
    a.tab = reinterpret_cast<uint4 *>(d_tab);
    const dim3 grid((unsigned)n_clips * (unsigned)splits, (unsigned)n_q);
    hipLaunchKernelGGL(overlap_popc_kernel, grid, dim3(256), 0, s, a);
}

void launch_overlap_select(void *d_tab, int n_q, int n_clips, int splits, const int32_t *d_exclude, int k, uint32_t clip_base, void *d_out,
                           hipStream_t s)
{
    hipLaunchKernelGGL(overlap_select_kernel, dim3(n_q), dim3(256), 0, s, reinterpret_cast<uint4 *>(d_tab), n_clips, splits, d_exclude, k,
                       clip_base, reinterpret_cast<OverlapHitDev *>(d_out));
}

} // namespace hpfw
