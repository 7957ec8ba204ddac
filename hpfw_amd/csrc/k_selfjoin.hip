// k_selfjoin.hip -- the join of the index with itself (include/hpfw_gpu.h): for clips a < b the best lag
// of a against b by the overlap rule of section 17, and every pair under the caller's threshold.
//
// Clip a takes the query's part and b the clip's: lag d puts position j of a on position d + j of b, L(d) =
// min(n_a, n_b - d) - max(0, -d), dist(d) = sum popcount(a[j] ^ b[d + j]).  The rule, its comparison, a workgroup's best,
// the fold of the splits, the threshold test, the expansion to fp4 and the end of a chunk on either route are in
// overlap_rule.h, shared with the overlap search; this file instantiates JoinRule (dist <= 2^24, L < 2^18: full 64-bit
// products) and keeps what is its own: the pairs, the staging and the multiply loop.
//
// (a) selfjoin_mfma_kernel has overlap_mfma_kernel's geometry (k_search_overlap.hip): a workgroup = 32 rows (clips a of one
// row group) x 1024 lags of one b per chunk, fp4 +-1 operands, fp4 0 outside either recording, accumulator 64 L - 2 dist.
// Both operands are read from the index where it lies and expanded while they are staged.  The rows are walked in SLICES of
// kSjSlice positions: per slice the 32 rows' hashprints and the kSjChunk + kSjSlice positions of b that the chunk's lags put
// under them go to the LDS, and the accumulators stay in registers across slices -- the LDS does not depend on a
// recording's length.  Slices that lie wholly before b's start or past its end are not staged.
// (b) selfjoin_popc_kernel computes the same by xor/popcount (HPFW_SELFJOIN_POPC): the second opinion on the device.
//
// Work is launched for b above a group's first row only: workgroup p / splits of a pass is pair p of pair_first's prefix.
// Rows with a >= b (the triangle cuts through a group) and rows below min_overlap are masked.  Both kernels write one
// 16-byte entry {dist, L, lag, 0} per (row, b, split) with ordinary stores, as section 17 does.  selfjoin_count_kernel folds
// the splits and counts a row's pairs under the threshold, selfjoin_offsets_kernel turns the counts into positions, and
// selfjoin_write_kernel writes the pairs in (a, b) order: no atomics, nothing depends on the order workgroups run in.
//
// The join of the index with recordings that are not in it is the same scan under JoinArgs: the rows
// are the 32-row groups of the list "index slots, then externals", b runs over the externals only, a clip's hashprints lie in
// the index or in the caller's buffer, and the table's columns are the externals.  Both scan kernels are templates over
// their arguments; what differs is in sj_clip, sj_ptr, sj_hp, sj_first_b, sj_row_end and sj_entry.
#include "kernels.h"
#include "overlap_rule.h"

namespace hpfw {

extern __shared__ __align__(16) unsigned char smem_raw[];

typedef int v8i __attribute__((ext_vector_type(8)));

namespace {
constexpr int kSjThreads = 512;                            // 8 waves
constexpr int kSjTiles = 4;                                // lag tiles of 32 per wave
constexpr int kSjWaveLags = 32 * kSjTiles;                 // 128
constexpr int kSjWin = kSelfjoinChunk + kSelfjoinSlice;    // positions of b staged per slice (one spare)
constexpr int kSjBLoads = (kSjWin + kSjThreads - 1) / kSjThreads; // positions of b per thread and slice
static_assert(kSjWaveLags * (kSjThreads / 64) == kSelfjoinChunk, "kernels.h states the chunk");
static_assert(kSelfjoinSlice == 32 && kSjThreads == 512, "stage_a deals 32 positions x 32 rows to 512 threads, two each");
static_assert(kSelfjoinChunk == JoinRule::kChunk, "a candidate's lag inside the chunk takes 10 bits");

using Rule = JoinRule;
} // namespace

struct SelfjoinArgs {
    const uint64_t *db;
    const int64_t *db_off;
    int n_clips;
    int g0, n_groups;           // the pass: row groups g0 .. g0 + n_groups - 1 (rows 32 g .. 32 g + 31)
    const uint32_t *pair_first; // [n_groups + 1]: group g0 + i has the pairs pair_first[i] .. pair_first[i + 1] - 1, one per b > 32 (g0 + i)
    int min_overlap, splits;
    uint4 *tab;                 // [32 n_groups][n_clips][splits], every byte preset to 0xff
    static constexpr bool kJoin = false;
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
// the workgroup's pair and split; the rows' lengths (0: masked) and starts; kt, the longest unmasked row
struct SjPair {
    int gi, b, split, kt;
};
// where clip `id` begins and its length: the self-join keeps an offset into the index, the join the address itself (the
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
// the entry of (row of the pass, b, split)
template <class Args>
__device__ __forceinline__ uint4 *sj_entry(const Args &a, int row, int b, int split)
{
    if constexpr (Args::kJoin)
        return a.tab + ((int64_t)row * a.n_x + (b - a.n_index)) * a.splits + split;
    else
        return a.tab + ((int64_t)row * a.n_clips + b) * a.splits + split;
}

template <class Args>
__device__ __forceinline__ SjPair sj_pair(const Args &a, int *lens, int64_t *starts)
{
    SjPair p;
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
} // namespace

template <class Args>
__global__ __launch_bounds__(kSjThreads, 4) void selfjoin_mfma_kernel(Args a)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_lane = lane & 31, h = lane >> 5;
    v4i *ldsB = reinterpret_cast<v4i *>(smem_raw);           // [2][kSjWin]: plane h = bits [32 h, 32 h + 32) of each hashprint
    v4i *ldsA = ldsB + 2 * kSjWin;                           // [kSjSlice][64]: lane (m, h) of position j
    int64_t *starts = reinterpret_cast<int64_t *>(ldsA + kSelfjoinSlice * 64); // [32]
    int *lens = reinterpret_cast<int *>(starts + 32);        // [32]
    uint2 *red = reinterpret_cast<uint2 *>(ldsA);            // [8 waves][32 rows], over the A operand once the sums are done

    const SjPair p = sj_pair(a, lens, starts);
    int n;
    const int64_t r0 = sj_clip(a, p.b, n);
    const int kt = p.kt, mo = a.min_overlap;
    if (n < mo || kt == 0) return; // no row of the group has a candidate in this clip
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
    const int one = 0x7f7f7f7f; // E8M0 scale 2^0
    const v4i *bp = ldsB + h * kSjWin + wave * kSjWaveLags + n_lane;
    const v4i *ap = ldsA + lane;
    Rule::Best best; // (threads below 32)

    for (int wc = p.split; wc < n_wg_chunks; wc += a.splits) {
        const int d0 = d_lo + wc * kSelfjoinChunk;
        // slices j0 (multiples of kSjSlice) whose window of b, positions d0 + j0 .. d0 + j0 + kSjWin - 1, meets the clip
        const int before = -d0 - kSjWin + 1; // j0 >= before
        const int j_begin = before <= 0 ? 0 : (before + kSelfjoinSlice - 1) / kSelfjoinSlice * kSelfjoinSlice;
        const int j_end = min(kt, n - d0);   // j0 < j_end
        f32x16 acc[kSjTiles];
#pragma unroll
        for (int t = 0; t < kSjTiles; ++t) acc[t] = f32x16{0};
        // a wave whose 128 lags all lie past n - min_overlap (the clip's last chunk) multiplies nothing: it only helps staging
        const bool live = d0 + wave * kSjWaveLags <= d_hi;

        uint64_t ra[2], rb[kSjBLoads];
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
            for (int e = 0; e < kSjBLoads; ++e) {
                const int i = tid + kSjThreads * e, gi = d0 + j0 + i;
                rb[e] = 0;
                if (i < kSjWin && gi >= 0 && gi < n) {
                    rb[e] = sj_hp(a, r0, gi);
                    ok |= 4u << e;
                }
            }
        };
        load(j_begin);
        for (int j0 = j_begin; j0 < j_end; j0 += kSelfjoinSlice) {
            __syncthreads(); // the slice before this one, or the chunk's candidates, have been read
            const v4i zero = {0, 0, 0, 0};
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const bool v = (ok >> e) & 1u;
                ldsA[ja[e] * 64 + ma[e]] = v ? expand32((uint32_t)ra[e]) : zero;
                ldsA[ja[e] * 64 + 32 + ma[e]] = v ? expand32((uint32_t)(ra[e] >> 32)) : zero;
            }
#pragma unroll
            for (int e = 0; e < kSjBLoads; ++e) {
                const int i = tid + kSjThreads * e;
                if (i < kSjWin) {
                    const bool v = (ok >> (2 + e)) & 1u;
                    ldsB[i] = v ? expand32((uint32_t)rb[e]) : zero;
                    ldsB[kSjWin + i] = v ? expand32((uint32_t)(rb[e] >> 32)) : zero;
                }
            }
            __syncthreads();
            if (j0 + kSelfjoinSlice < j_end) load(j0 + kSelfjoinSlice); // the next slice into registers while this one multiplies
            const int jn = min(kSelfjoinSlice, kt - j0);
            for (int j = 0; live && j < jn; ++j) {
                const v4i a4 = ap[j * 64];
                const v8i av = {a4.x, a4.y, a4.z, a4.w, 0, 0, 0, 0};
#pragma unroll
                for (int t = 0; t < kSjTiles; ++t) {
                    const v4i b4 = bp[j + 32 * t];
                    const v8i bv = {b4.x, b4.y, b4.z, b4.w, 0, 0, 0, 0};
                    acc[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc[t], 4, 4, 0, one, 0, one);
                }
            }
        }
        __syncthreads(); // the last slice has been read: the candidates go over the A operand

        Rule::tile_epilogue(acc, lens, n, mo, d0, red, best, tid, wave, n_lane, h);
    }
    if (tid < 32 && lens[tid] > 0)
        best.store(sj_entry(a, 32 * p.gi + tid, p.b, p.split));
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
    const SjPair p = sj_pair(a, lens, starts);
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

// one workgroup per row a of the pass: the splits of every b > a folded into the pair's first entry, and the row's pairs
// under the threshold counted.  Column c of the table is clip col0 + c (the self-join: col0 = 0, n_cols = n_clips; the join:
// the externals)
__global__ __launch_bounds__(256) void selfjoin_count_kernel(uint4 *__restrict__ tab, int n_cols, int col0, int splits, int row0,
                                                             unsigned rate_num, unsigned rate_den, int *__restrict__ row_count)
{
    __shared__ int red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint4 *row = tab + (int64_t)blockIdx.x * n_cols * splits;
    int cnt = 0;
    for (int c = max(row0 + (int)blockIdx.x + 1 - col0, 0) + tid; c < n_cols; c += 256) {
        uint4 b = row[(int64_t)c * splits];
        for (int s = 1; s < splits; ++s) Rule::fold(b, row[(int64_t)c * splits + s]);
        if (splits > 1) row[(int64_t)c * splits] = b;
        cnt += Rule::reported(b, rate_num, rate_den) ? 1 : 0;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) cnt += __shfl_xor(cnt, s);
    if (lane == 0) red[wave] = cnt;
    __syncthreads();
    if (tid == 0) row_count[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// one workgroup: row_first[i] = *total + the counts of the pass's rows before i, then *total += the pass's pairs
__global__ __launch_bounds__(1024) void selfjoin_offsets_kernel(const int *__restrict__ row_count, int n_rows, int64_t *__restrict__ row_first,
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

namespace {
struct DupPairDev {
    uint32_t a, b, dist, overlap;
    int32_t lag;
    uint32_t pad;
};
static_assert(sizeof(DupPairDev) == sizeof(hpfw_dup_pair), "the record of include/hpfw_gpu.h");
} // namespace

// one workgroup per row a: its pairs under the threshold in rising b, from position row_first[a] on, while below cap
__global__ __launch_bounds__(256) void selfjoin_write_kernel(const uint4 *__restrict__ tab, int n_cols, int col0, int splits, int row0,
                                                             unsigned rate_num, unsigned rate_den, const int64_t *__restrict__ row_first,
                                                             uint32_t clip_base, DupPairDev *__restrict__ out, int64_t cap)
{
    __shared__ int wave_n[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = row0 + (int)blockIdx.x;
    const uint4 *row = tab + (int64_t)blockIdx.x * n_cols * splits;
    int64_t at = row_first[blockIdx.x];
    for (int c0 = max(a + 1 - col0, 0); c0 < n_cols && at < cap; c0 += 256) {
        const int c = c0 + tid;
        uint4 e = make_uint4(kOverlapNoEntry, 0u, 0u, 0u);
        if (c < n_cols) e = row[(int64_t)c * splits];
        const bool rep = Rule::reported(e, rate_num, rate_den);
        const unsigned long long mask = __ballot(rep);
        __syncthreads(); // (the block of 256 before has been read)
        if (lane == 0) wave_n[wave] = __popcll(mask);
        __syncthreads();
        int64_t mine = at + __popcll(mask & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) mine += wave_n[w];
        if (rep && mine < cap) out[mine] = {clip_base + (uint32_t)a, clip_base + (uint32_t)(col0 + c), e.x, e.y, (int32_t)e.z, 0u};
        at += wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
    }
}

size_t selfjoin_mfma_lds_bytes() { return (size_t)2 * kSjWin * 16 + (size_t)kSelfjoinSlice * 64 * 16 + 32 * 8 + 32 * 4; }

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
                                  (int)selfjoin_mfma_lds_bytes());
        attr_set.mark();
    }
    hipLaunchKernelGGL(selfjoin_mfma_kernel<Args>, grid, dim3(kSjThreads), selfjoin_mfma_lds_bytes(), s, a);
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
    hipLaunchKernelGGL(selfjoin_count_kernel, dim3(n_rows), dim3(256), 0, s, reinterpret_cast<uint4 *>(d_tab), n_cols, col0, splits, row0,
                       rate_num, rate_den, d_row_count);
    hipLaunchKernelGGL(selfjoin_offsets_kernel, dim3(1), dim3(1024), 0, s, d_row_count, n_rows, d_row_first, d_count);
    if (cap > 0)
        hipLaunchKernelGGL(selfjoin_write_kernel, dim3(n_rows), dim3(256), 0, s, reinterpret_cast<const uint4 *>(d_tab), n_cols, col0, splits,
                           row0, rate_num, rate_den, d_row_first, clip_base, reinterpret_cast<DupPairDev *>(d_out), cap);
}

} // namespace hpfw
