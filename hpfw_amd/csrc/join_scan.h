// join_scan.h -- what the catalogue self-join, the join with recordings outside the index (k_selfjoin.hip, DESIGN.md
// sections 22 and 23) and the local self-join (k_localjoin.hip, section 26) share on the device, stated once: the geometry of
// the matrix-core scan, a workgroup's pair, the walk of a chunk in slices, and the selection of a pass's pairs from its table.
// Device code only; everything but the selection kernels is inlined into its kernel.
//
// GEOMETRY.  A workgroup = 32 rows (clips a of one row group) x kSelfjoinChunk lags of one clip b per chunk; lag d puts
// position j of a on position d + j of b.  Workgroup p / splits of a pass is pair p of pair_first's prefix, found by binary
// search; the chunks of a pair are dealt round robin to `splits` workgroups.  The rows are walked in SLICES of kSelfjoinSlice
// positions: per slice the 32 rows' hashprints and the kJoinWin positions of b that the chunk's lags put under them are read
// from where they lie, expanded to fp4 +-1 (fp4 0 outside either recording) and staged in the LDS; the caller's accumulators
// stay in registers across slices, so the LDS does not depend on a recording's length.  After the second barrier of a slice
// the next slice is fetched into registers while this one multiplies: the caller's step runs for the slice's positions
// j < jn of every live wave -- the loop has no per-lag or per-position condition, only `live`, which switches off a whole
// wave whose 128 lags all lie past the last admissible lag d_hi (those lags are read by nobody).
//
// A step is one of two.  The overlap step (k_selfjoin.hip) adds the products: acc = 64 L - 2 dist.  The run step
// (k_localjoin.hip) adds the products and the constant 2 T - 64, then best = max(best, cur), cur = max(cur, 0): a position
// outside a or b multiplies fp4 zeros, so it adds nothing to the first and counts as x = T - 32 < 0 in the second.
//
// SKIPPED SLICES.  A chunk stages only the slices whose window of b meets b, and only positions below the longest unmasked
// row kt.  For the overlap step a slice that is not staged would have added products with fp4 zeros: nothing.  For the run
// step: (1) in a slice whose window lies wholly before b's start every position of every lag of the chunk is outside b, so
// every step is T - 32 < 0: from cur = 0, where the chunk starts, each step leaves cur < 0 and the clamp returns it to 0,
// and best does not move -- the state after the slice is the state before it.  (2) In a slice whose window lies wholly past
// b's end, and at positions at or past kt, every step is strictly negative as well, so cur only falls (or is clamped) and
// best = max(best, cur) cannot rise; no slice follows that could use cur.
//
// MASKED ROWS.  Rows with a >= b (the triangle cuts through a group), rows at or above the join's row_end, rows that do not
// exist, and rows shorter than min_overlap are given length 0: they are staged as fp4 zeros and the caller's epilogue and
// final store skip them (the overlap step: no lag of theirs is a candidate; the run step: every step of theirs is
// T - 32 < 0, their best stays 0, and a score of 0 makes no candidate).
//
// SELECTION.  Each scan leaves one entry per (row, b, split) in a table preset to 0xff in every byte.  join_count_kernel folds
// the splits into the pair's first entry and counts a row's reported pairs, join_offsets_kernel turns the counts into
// positions, join_write_kernel writes the pairs in (a, b) order below cap: no atomics, nothing depends on the order
// workgroups run in.  What an entry is, how two fold, which are reported and the record written are the Policy's.
#pragma once
#include "kernels.h"
#include "overlap_rule.h"
#include "query_scan.h" // scan_products: a position's products

namespace hpfw {

constexpr int kJoinThreads = 512;                              // 8 waves
constexpr int kJoinTiles = kScanTiles;                         // lag tiles of 32 per wave
constexpr int kJoinWaveLags = 32 * kJoinTiles;                 // 128
constexpr int kJoinWin = kSelfjoinChunk + kSelfjoinSlice;      // positions of b staged per slice (one spare)
constexpr int kJoinBLoads = (kJoinWin + kJoinThreads - 1) / kJoinThreads; // positions of b per thread and slice
static_assert(kJoinWaveLags * (kJoinThreads / 64) == kSelfjoinChunk, "kernels.h states the chunk");
static_assert(kSelfjoinSlice == 32 && kJoinThreads == 512, "the staging deals 32 positions x 32 rows to 512 threads, two each");

// dynamic LDS of a matrix-core scan: ldsB [2][kJoinWin], ldsA [kSelfjoinSlice][64], starts [32], lens [32]
inline size_t join_scan_lds_bytes() { return (size_t)2 * kJoinWin * 16 + (size_t)kSelfjoinSlice * 64 * 16 + 32 * 8 + 32 * 4; }

// what every scan is told; a scan adds its table and what its step needs
struct JoinScanArgs {
    const uint64_t *db;
    const int64_t *db_off;
    int n_clips;
    int g0, n_groups;           // the pass: row groups g0 .. g0 + n_groups - 1 (rows 32 g .. 32 g + 31)
    const uint32_t *pair_first; // [n_groups + 1]: group g0 + i has the pairs pair_first[i] .. pair_first[i + 1] - 1, one per b > 32 (g0 + i)
    int min_overlap, splits;    // (the local self-join: min_overlap is its min_len)
    static constexpr bool kJoin = false;
};

// Arguments with kJoin (k_selfjoin.hip's JoinArgs) add the recordings outside the index: x, x_off, n_index, n_x, row_end.
// Where clip `id` begins and its length: without externals an offset into the index, with them the address itself (the
// clip lies in the index or among the externals); sj_hp reads position j from either
template <class Args>
__device__ __forceinline__ int64_t sj_clip(const Args &a, int id, int &len)
{
    if constexpr (Args::kJoin) {
        const bool ext = id >= a.n_index;
        const int64_t *off = ext ? a.x_off + (id - a.n_index) : a.db_off + id;
        const int64_t o = off[0];
        len = (int)(off[1] - o);
        return reinterpret_cast<int64_t>((ext ? a.x : a.db) + o);
    } else {
        const int64_t o = a.db_off[id];
        len = (int)(a.db_off[id + 1] - o);
        return o;
    }
}
template <class Args>
__device__ __forceinline__ const uint64_t *sj_ptr(const Args &a, int64_t start)
{
    if constexpr (Args::kJoin)
        return reinterpret_cast<const uint64_t *>(start);
    else
        return a.db + start;
}
template <class Args>
__device__ __forceinline__ uint64_t sj_hp(const Args &a, int64_t start, int j)
{
    if constexpr (Args::kJoin)
        return reinterpret_cast<const uint64_t *>(start)[j];
    else
        return a.db[start + j];
}
// the b of a group's first pair; the rows of a pair are those below sj_row_end: a < b, and for the join a < row_end
template <class Args>
__device__ __forceinline__ int sj_first_b(const Args &a, int g)
{
    if constexpr (Args::kJoin)
        return max(a.n_index, 32 * g + 1);
    else
        return 32 * g + 1;
}
template <class Args>
__device__ __forceinline__ int sj_row_end(const Args &a, int b)
{
    if constexpr (Args::kJoin)
        return min(b, a.row_end);
    else
        return b;
}

// the workgroup's pair and split; the rows' lengths (0: masked) and starts go to lens [32] and starts [32]; kt, the longest
// unmasked row
struct JoinPair {
    int gi, b, split, kt;
};
template <class Args>
__device__ __forceinline__ JoinPair join_pair(const Args &a, int *lens, int64_t *starts)
{
    JoinPair p;
    const unsigned pair = blockIdx.x / (unsigned)a.splits;
    p.split = (int)(blockIdx.x - pair * (unsigned)a.splits);
    int lo = 0, hi = a.n_groups; // the last group whose first pair is at or below this one
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.pair_first[mid] <= pair)
            lo = mid;
        else
            hi = mid;
    }
    p.gi = lo;
    p.b = sj_first_b(a, a.g0 + lo) + (int)(pair - a.pair_first[lo]);
    if (threadIdx.x < 32) {
        const int row = 32 * (a.g0 + lo) + (int)threadIdx.x;
        int k = 0;
        int64_t o = 0;
        if (row < sj_row_end(a, p.b)) { // (b < n_clips: the row exists)
            o = sj_clip(a, row, k);
            if (k < a.min_overlap) k = 0;
        }
        lens[threadIdx.x] = k;
        starts[threadIdx.x] = o;
    }
    __syncthreads();
    p.kt = 0;
    for (int m = 0; m < 32; ++m) p.kt = max(p.kt, lens[m]);
    return p;
}

// The matrix-core scan of the workgroup's pair (kJoinThreads threads, join_scan_lds_bytes() of dynamic LDS at smem).  The
// accumulators are the caller's registers, zero on entry.  step(ap, bp, j) takes in position j of the staged slice: this
// lane's operands are ap[j * 64] and bp[j + 32 t] for lag tile t.  chunk_end(c) reduces the accumulators of chunk c.d0 and leaves them zero for the next
// chunk; c.red, the A operand's 32 KiB, is its own until it returns (a barrier lies before it, and one before the next
// store there).  What join_scan returns names the pair and its rows for the workgroup's final store; without a chunk
// (no row of the group has a candidate in this clip) neither callable has run.
struct JoinChunk {
    JoinPair p;
    const int *lens; // [32]: the rows' lengths, 0 for a masked row
    int n, d0;       // b's length; the chunk's first lag
    void *red;
    int tid, wave, n_lane, h; // lane = n_lane + 32 h
};
template <class Args, class Step, class End>
__device__ __forceinline__ JoinChunk join_scan(const Args &a, unsigned char *smem, Step step, End chunk_end)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_lane = lane & 31, h = lane >> 5;
    v4i *ldsB = reinterpret_cast<v4i *>(smem);               // [2][kJoinWin]: plane h = bits [32 h, 32 h + 32) of each hashprint
    v4i *ldsA = ldsB + 2 * kJoinWin;                         // [kSelfjoinSlice][64]: lane (m, h) of position j
    int64_t *starts = reinterpret_cast<int64_t *>(ldsA + kSelfjoinSlice * 64); // [32]
    int *lens = reinterpret_cast<int *>(starts + 32);        // [32]

    const JoinPair p = join_pair(a, lens, starts);
    int n;
    const int64_t r0 = sj_clip(a, p.b, n);
    const int kt = p.kt, mo = a.min_overlap;
    JoinChunk ck = {p, lens, n, 0, ldsA, tid, wave, n_lane, h};
    if (n < mo || kt == 0) return ck; // no row of the group has a candidate in this clip
    const int d_lo = mo - kt, d_hi = n - mo;
    const int n_wg_chunks = (d_hi - d_lo) / kSelfjoinChunk + 1;

    // staging: thread -> 8 consecutive positions of 8 rows per wave (64-byte runs of a row), two (position, row) items
    int ja[2], ma[2], ka[2];
    int64_t oa[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int c = wave * 2 + e;
        ja[e] = (c & 3) * 8 + (lane & 7);
        ma[e] = (c >> 2) * 8 + (lane >> 3);
        ka[e] = lens[ma[e]];
        oa[e] = starts[ma[e]];
    }
    const v4i *bp = ldsB + h * kJoinWin + wave * kJoinWaveLags + n_lane;
    const v4i *ap = ldsA + lane;

    for (int wc = p.split; wc < n_wg_chunks; wc += a.splits) {
        const int d0 = d_lo + wc * kSelfjoinChunk;
        // slices j0 (multiples of kSelfjoinSlice) whose window of b, positions d0 + j0 .. d0 + j0 + kJoinWin - 1, meets the clip
        const int before = -d0 - kJoinWin + 1; // j0 >= before
        const int j_begin = before <= 0 ? 0 : (before + kSelfjoinSlice - 1) / kSelfjoinSlice * kSelfjoinSlice;
        const int j_end = min(kt, n - d0);     // j0 < j_end
        // a wave whose 128 lags all lie past d_hi (the clip's last chunk) multiplies nothing: it only helps staging
        const bool live = d0 + wave * kJoinWaveLags <= d_hi;

        uint64_t ra[2], rb[kJoinBLoads];
        unsigned ok = 0; // bit e: ra[e] is a hashprint of its row; bit 2 + e: rb[e] is a hashprint of b
        auto load = [&](int j0) {
            ok = 0;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                ra[e] = 0;
                if (j0 + ja[e] < ka[e]) {
                    ra[e] = sj_hp(a, oa[e], j0 + ja[e]);
                    ok |= 1u << e;
                }
            }
#pragma unroll
            for (int e = 0; e < kJoinBLoads; ++e) {
                const int i = tid + kJoinThreads * e, gi = d0 + j0 + i;
                rb[e] = 0;
                if (i < kJoinWin && gi >= 0 && gi < n) {
                    rb[e] = sj_hp(a, r0, gi);
                    ok |= 4u << e;
                }
            }
        };
        load(j_begin);
        for (int j0 = j_begin; j0 < j_end; j0 += kSelfjoinSlice) {
            __syncthreads(); // the slice before this one, or the chunk's reduction, have been read
            const v4i zero = {0, 0, 0, 0};
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const bool v = (ok >> e) & 1u;
                ldsA[ja[e] * 64 + ma[e]] = v ? expand32((uint32_t)ra[e]) : zero;
                ldsA[ja[e] * 64 + 32 + ma[e]] = v ? expand32((uint32_t)(ra[e] >> 32)) : zero;
            }
#pragma unroll
            for (int e = 0; e < kJoinBLoads; ++e) {
                const int i = tid + kJoinThreads * e;
                if (i < kJoinWin) {
                    const bool v = (ok >> (2 + e)) & 1u;
                    ldsB[i] = v ? expand32((uint32_t)rb[e]) : zero;
                    ldsB[kJoinWin + i] = v ? expand32((uint32_t)(rb[e] >> 32)) : zero;
                }
            }
            __syncthreads();
            if (j0 + kSelfjoinSlice < j_end) load(j0 + kSelfjoinSlice); // the next slice into registers while this one multiplies
            // kt and j0 are the workgroup's, so the count is a scalar; said outright, since left to itself the compiler counts
            // the positions down in a vector register once the step is a callable: two vector instructions more a position
            const int jn = __builtin_amdgcn_readfirstlane(min(kSelfjoinSlice, kt - j0));
            for (int j = 0; live && j < jn; ++j) step(ap, bp, j);
        }
        __syncthreads(); // the last slice has been read: the chunk's reduction goes over the A operand
        ck.d0 = d0;
        chunk_end(ck);
    }
    return ck;
}

// ---- the selection ----
// Policy: Entry, the table's entry; none(), the entry nobody wrote; col0, the clip of the table's column 0; fold(b, e), b takes
// in the entry e of another split; reported(e); record(a, b, e), what is written for clips a and b (ids with clip_base)

// one workgroup per row a of the pass: the splits of every b > a folded into the pair's first entry, and the row's reported
// pairs counted.  Column c of the table is clip col0 + c
template <class Policy>
__global__ __launch_bounds__(256) void join_count_kernel(typename Policy::Entry *__restrict__ tab, int n_cols, int splits, int row0, Policy pol,
                                                         int *__restrict__ row_count)
{
    __shared__ int red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    typename Policy::Entry *row = tab + (int64_t)blockIdx.x * n_cols * splits;
    int cnt = 0;
    for (int c = max(row0 + (int)blockIdx.x + 1 - pol.col0, 0) + tid; c < n_cols; c += 256) {
        typename Policy::Entry b = row[(int64_t)c * splits];
        for (int s = 1; s < splits; ++s) Policy::fold(b, row[(int64_t)c * splits + s]);
        if (splits > 1) row[(int64_t)c * splits] = b;
        cnt += pol.reported(b) ? 1 : 0;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) cnt += __shfl_xor(cnt, s);
    if (lane == 0) red[wave] = cnt;
    __syncthreads();
    if (tid == 0) row_count[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// join_offsets_kernel (k_selfjoin.hip), one workgroup: d_row_first[i] = *d_total + the counts of the pass's rows before i,
// then *d_total += the pass's pairs
void launch_join_offsets(const int *d_row_count, int n_rows, int64_t *d_row_first, int64_t *d_total, hipStream_t s);

// one workgroup per row a: its reported pairs in rising b, from position row_first[a] on, while below cap
template <class Policy>
__global__ __launch_bounds__(256) void join_write_kernel(const typename Policy::Entry *__restrict__ tab, int n_cols, int splits, int row0, Policy pol,
                                                         const int64_t *__restrict__ row_first, uint32_t clip_base,
                                                         typename Policy::Record *__restrict__ out, int64_t cap)
{
    __shared__ int wave_n[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = row0 + (int)blockIdx.x;
    const typename Policy::Entry *row = tab + (int64_t)blockIdx.x * n_cols * splits;
    int64_t at = row_first[blockIdx.x];
    for (int c0 = max(a + 1 - pol.col0, 0); c0 < n_cols && at < cap; c0 += 256) {
        const int c = c0 + tid;
        typename Policy::Entry e = Policy::none();
        if (c < n_cols) e = row[(int64_t)c * splits];
        const bool rep = pol.reported(e);
        const unsigned long long mask = __ballot(rep);
        __syncthreads(); // (the block of 256 before has been read)
        if (lane == 0) wave_n[wave] = __popcll(mask);
        __syncthreads();
        int64_t mine = at + __popcll(mask & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) mine += wave_n[w];
        if (rep && mine < cap) out[mine] = Policy::record(clip_base + (uint32_t)a, clip_base + (uint32_t)(pol.col0 + c), e);
        at += wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
    }
}

// count, offsets and, with cap > 0, write for rows row0 .. row0 + n_rows - 1 of a pass
template <class Policy>
void launch_join_select(void *d_tab, int n_cols, int splits, int row0, int n_rows, const Policy &pol, int *d_row_count, int64_t *d_row_first,
                        uint32_t clip_base, void *d_out, int64_t cap, int64_t *d_count, hipStream_t s)
{
    hipLaunchKernelGGL(join_count_kernel<Policy>, dim3(n_rows), dim3(256), 0, s, reinterpret_cast<typename Policy::Entry *>(d_tab), n_cols, splits,
                       row0, pol, d_row_count);
    launch_join_offsets(d_row_count, n_rows, d_row_first, d_count, s);
    if (cap > 0)
        hipLaunchKernelGGL(join_write_kernel<Policy>, dim3(n_rows), dim3(256), 0, s, reinterpret_cast<const typename Policy::Entry *>(d_tab), n_cols,
                           splits, row0, pol, d_row_first, clip_base, reinterpret_cast<typename Policy::Record *>(d_out), cap);
}

} // namespace hpfw
