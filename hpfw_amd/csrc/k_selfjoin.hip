// k_selfjoin.hip -- the join of the index with itself (include/hpfw_gpu.h): for clips a < b the best lag
// of a against b by the overlap rule of section 17, and every pair under the caller's threshold.
//
// Clip a takes the query's part and b the clip's: lag d puts position j of a on position d + j of b, L(d) =
// min(n_a, n_b - d) - max(0, -d), dist(d) = sum popcount(a[j] ^ b[d + j]).  The rule, its comparison, a workgroup's best,
// the fold of the splits, the threshold test, the expansion to fp4 and the end of a chunk on either route are in
// overlap_rule.h, shared with the overlap search; this file instantiates JoinRule (dist <= 2^24, L < 2^18: full 64-bit
// products).  The pairs, the staging in slices, the arguments for skipped slices and masked rows and the selection of a
// pass's pairs are in join_scan.h, shared with the local self-join; this file keeps the step and the table's entry.
//
// (a) selfjoin_mfma_kernel: join_scan.h's geometry with the overlap step -- per position one product per lag tile, fp4 +-1
// operands, fp4 0 outside either recording, accumulator 64 L - 2 dist; Rule::tile_epilogue ends a chunk.
// (b) selfjoin_popc_kernel computes the same by xor/popcount (HPFW_SELFJOIN_POPC): the second opinion on the device.
//
// Both kernels write one 16-byte entry {dist, L, lag, 0} per (row, b, split) with ordinary stores, as section 17 does.
// SelfjoinSelect is the selection's policy: Rule::fold, Rule::reported under (rate_num, rate_den), hpfw_dup_pair.
//
// The join of the index with recordings that are not in it is the same scan under JoinArgs: the rows
// are the 32-row groups of the list "index slots, then externals", b runs over the externals only, a clip's hashprints lie in
// the index or in the caller's buffer, and the table's columns are the externals.  Both scan kernels are templates over
// their arguments; what differs is in sj_clip, sj_ptr, sj_hp, sj_first_b, sj_row_end (join_scan.h) and sj_entry.
#include "join_scan.h"

namespace hpfw {

extern __shared__ __align__(16) unsigned char smem_raw[];

namespace {
static_assert(kSelfjoinChunk == JoinRule::kChunk, "a candidate's lag inside the chunk takes 10 bits");

using Rule = JoinRule;
} // namespace

struct SelfjoinArgs : JoinScanArgs {
    uint4 *tab;                 // [32 n_groups][n_clips][splits], every byte preset to 0xff
};

// the join: clip ids n_index .. n_index + n_x - 1 are the externals x, n_clips = n_index + n_x, a pass's pairs are numbered as
// hpfw_gpu_join_plan numbers them, rows at or above row_end are masked (among_new = 0: n_index)
struct JoinArgs : SelfjoinArgs {
    const uint64_t *x;
    const int64_t *x_off;       // [n_x + 1]
    int n_index, n_x, row_end;  // tab [32 n_groups][n_x][splits]
    static constexpr bool kJoin = true;
};

namespace {
// the entry of (row of the pass, b, split)
template <class Args>
__device__ __forceinline__ uint4 *sj_entry(const Args &a, int row, int b, int split)
{
    if constexpr (Args::kJoin)
        return a.tab + ((int64_t)row * a.n_x + (b - a.n_index)) * a.splits + split;
    else
        return a.tab + ((int64_t)row * a.n_clips + b) * a.splits + split;
}
} // namespace

template <class Args>
__global__ __launch_bounds__(kJoinThreads, 4) void selfjoin_mfma_kernel(Args a)
{
    Rule::Best best; // (threads below 32)
    f32x16 acc[kJoinTiles];
#pragma unroll
    for (int t = 0; t < kJoinTiles; ++t) acc[t] = f32x16{0};
    const JoinChunk c = join_scan(
        a, smem_raw,
        [&](const v4i *ap, const v4i *bp, int j) { scan_products(acc, ap, bp, j); },
        [&](const JoinChunk &c) { // the candidates [8 waves][32 rows] go over the A operand now that the sums are done
            Rule::tile_epilogue(acc, c.lens, c.n, a.min_overlap, c.d0, static_cast<uint2 *>(c.red), best, c.tid, c.wave, c.n_lane, c.h);
#pragma unroll
            for (int t = 0; t < kJoinTiles; ++t) acc[t] = f32x16{0};
        });
    if (c.tid < 32 && c.lens[c.tid] > 0) best.store(sj_entry(a, 32 * c.p.gi + c.tid, c.p.b, c.p.split));
}

// the same pairs, splits and chunks (the chunks of a pair begin at min_overlap - the group's longest row for every row): a
// thread takes four lags of a chunk and walks their overlaps, one row after the other
template <class Args>
__global__ __launch_bounds__(256) void selfjoin_popc_kernel(Args a)
{
    __shared__ uint2 red[4];
    __shared__ int lens[32];
    __shared__ int64_t starts[32];
    const int tid = threadIdx.x;
    const JoinPair p = join_pair(a, lens, starts);
    int n;
    const int64_t r0 = sj_clip(a, p.b, n);
    const int mo = a.min_overlap;
    if (n < mo || p.kt == 0) return;
    const uint64_t *r = sj_ptr(a, r0);
    const int d_lo = mo - p.kt, d_hi = n - mo;
    const int n_wg_chunks = (d_hi - d_lo) / kSelfjoinChunk + 1;
    for (int m = 0; m < 32; ++m) {
        const int k = lens[m];
        if (k == 0) continue;
        const uint64_t *q = sj_ptr(a, starts[m]);
        Rule::Best best; // (thread 0)
        for (int wc = p.split; wc < n_wg_chunks; wc += a.splits) // (true: a row shorter than the group's longest)
            Rule::popc_chunk<true>(q, k, r, n, mo, d_lo + wc * kSelfjoinChunk, d_hi, red, best, tid);
        if (tid == 0) best.store(sj_entry(a, 32 * p.gi + m, p.b, p.split));
    }
}

// one workgroup: row_first[i] = *total + the counts of the pass's rows before i, then *total += the pass's pairs
__global__ __launch_bounds__(1024) void join_offsets_kernel(const int *__restrict__ row_count, int n_rows, int64_t *__restrict__ row_first,
                                                            int64_t *__restrict__ total)
{
    __shared__ int64_t part[1024];
    const int tid = threadIdx.x;
    const int per = (n_rows + 1023) / 1024, i0 = tid * per, i1 = min(n_rows, i0 + per);
    int64_t sum = 0;
    for (int i = i0; i < i1; ++i) sum += row_count[i];
    part[tid] = sum;
    __syncthreads();
    for (int s = 1; s < 1024; s <<= 1) { // (inclusive scan of the threads' sums)
        const int64_t v = tid >= s ? part[tid - s] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    const int64_t base = *total;
    int64_t at = base + part[tid] - sum;
    for (int i = i0; i < i1; ++i) {
        row_first[i] = at;
        at += row_count[i];
    }
    __syncthreads(); // (every thread has read *total)
    if (tid == 1023) *total = base + part[1023];
}

void launch_join_offsets(const int *d_row_count, int n_rows, int64_t *d_row_first, int64_t *d_total, hipStream_t s)
{
    hipLaunchKernelGGL(join_offsets_kernel, dim3(1), dim3(1024), 0, s, d_row_count, n_rows, d_row_first, d_total);
}

namespace {
struct DupPairDev {
    uint32_t a, b, dist, overlap;
    int32_t lag;
    uint32_t pad;
};
static_assert(sizeof(DupPairDev) == sizeof(hpfw_dup_pair), "the record of include/hpfw_gpu.h");

// the selection (join_scan.h) by the overlap rule: pairs with dist rate_den <= rate_num L.  Column c of the table is clip
// col0 + c (the self-join: col0 = 0, n_cols = n_clips; the join: the externals)
struct SelfjoinSelect {
    using Entry = uint4;
    using Record = DupPairDev;
    unsigned rate_num, rate_den;
    int col0;
    static __device__ __forceinline__ Entry none() { return make_uint4(kOverlapNoEntry, 0u, 0u, 0u); }
    static __device__ __forceinline__ void fold(Entry &b, const Entry e) { Rule::fold(b, e); }
    __device__ __forceinline__ bool reported(const Entry &e) const { return Rule::reported(e, rate_num, rate_den); }
    static __device__ __forceinline__ Record record(uint32_t a, uint32_t b, const Entry &e) { return {a, b, e.x, e.y, (int32_t)e.z, 0u}; }
};
} // namespace

static SelfjoinArgs selfjoin_args(const uint64_t *d_db, const int64_t *d_db_off, int n_clips, int g0, int n_groups, const uint32_t *d_pair_first,
                                  int min_overlap, int splits, void *d_tab)
{
    SelfjoinArgs a = {};
    a.db = d_db;
    a.db_off = d_db_off;
    a.n_clips = n_clips;
    a.g0 = g0;
    a.n_groups = n_groups;
    a.pair_first = d_pair_first;
    a.min_overlap = min_overlap;
    a.splits = splits;
    a.tab = reinterpret_cast<uint4 *>(d_tab);
    return a;
}

// either scan under either arguments (the matrix-core kernel's LDS is raised once per device and instantiation)
template <class Args>
static void launch_scan(bool popc, const Args &a, uint32_t n_pairs, hipStream_t s)
{
    const dim3 grid(n_pairs * (unsigned)a.splits);
    if (popc) {
        hipLaunchKernelGGL(selfjoin_popc_kernel<Args>, grid, dim3(256), 0, s, a);
        return;
    }
    static PerDeviceOnce attr_set;
    if (attr_set.need()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(selfjoin_mfma_kernel<Args>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)join_scan_lds_bytes());
        attr_set.mark();
    }
    hipLaunchKernelGGL(selfjoin_mfma_kernel<Args>, grid, dim3(kJoinThreads), join_scan_lds_bytes(), s, a);
}

void launch_selfjoin_scan(bool popc, const uint64_t *d_db, const int64_t *d_db_off, int n_clips, int g0, int n_groups,
                          const uint32_t *d_pair_first, uint32_t n_pairs, int min_overlap, int splits, void *d_tab, hipStream_t s)
{
    launch_scan(popc, selfjoin_args(d_db, d_db_off, n_clips, g0, n_groups, d_pair_first, min_overlap, splits, d_tab), n_pairs, s);
}

void launch_join_scan(bool popc, const uint64_t *d_db, const int64_t *d_db_off, int n_index, const uint64_t *d_x, const int64_t *d_x_off, int n_x,
                      int among_new, int g0, int n_groups, const uint32_t *d_pair_first, uint32_t n_pairs, int min_overlap, int splits,
                      void *d_tab, hipStream_t s)
{
    JoinArgs a = {};
    static_cast<SelfjoinArgs &>(a) = selfjoin_args(d_db, d_db_off, n_index + n_x, g0, n_groups, d_pair_first, min_overlap, splits, d_tab);
    a.x = d_x;
    a.x_off = d_x_off;
    a.n_index = n_index;
    a.n_x = n_x;
    a.row_end = among_new ? n_index + n_x : n_index;
    launch_scan(popc, a, n_pairs, s);
}

void launch_selfjoin_select(void *d_tab, int n_cols, int col0, int splits, int row0, int n_rows, uint32_t rate_num, uint32_t rate_den,
                            int *d_row_count, int64_t *d_row_first, uint32_t clip_base, void *d_out, int64_t cap, int64_t *d_count, hipStream_t s)
{
    launch_join_select(d_tab, n_cols, splits, row0, n_rows, SelfjoinSelect{rate_num, rate_den, col0}, d_row_count, d_row_first, clip_base, d_out,
                       cap, d_count, s);
}

} // namespace hpfw
