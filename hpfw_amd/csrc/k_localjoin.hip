// k_localjoin.hip -- the local self-join (include/hpfw_gpu.h): for clips a < b of the index the
// best-scoring run of consecutive hashprints of a on any diagonal of b, and every pair whose run scores at least min_score.
//
// Clip a takes the query's part of the local search (section 25) and b the clip's: lag d puts position j of a on position
// d + j of b, x_j = T - popcount(a[j] ^ b[d + j]) (T = max_rate, 1..31), a run [j0, j1) scores sum x_j, and the pair's
// candidate is its best run over all lags: larger score, then smaller lag, then smaller j1, then smaller j0.  Exact integers.
//
// (a) localjoin_mfma_kernel: join_scan.h's geometry -- the pairs, the splits, the staging in slices, shared with the
// catalogue self-join -- with the run step, which is local_mfma_kernel's work per position (k_search_local.hip, the pieces in
// local_rule.h): one product instruction per tile, one instruction per tile that adds the step's constant (a row of +1
// against a column with 64 - 2 T values of -1), then best = max(best, cur), cur = max(cur, 0) on the bit patterns as signed
// integers.  cur is the accumulator itself: after a step it holds twice the best run that ends there.  acc and best stay in
// registers across slices.  A position outside a or b multiplies fp4 zeros and so counts as x = T - 32 < 0; a staged slice
// runs the constant's instruction at every one of its positions for every tile of every live wave, whether or not the lag
// has left b there.  Why skipped slices and masked rows change nothing is argued in join_scan.h.  All values are integers of
// magnitude at most 2 * 31 * L + 64 < 2^24 (kernels.h asserts it): exact in f32, in any order.
//
// PRUNING.  A run that scores at least min_score has at least min_len = ceil(min_score / T) positions (x_j <= T), so it
// lies on a lag with overlap L(d) >= min_len: min_len is the scan's min_overlap, and the chunks of a pair cover the lags
// min_len - kt .. n_b - min_len only (kt: the group's longest unmasked row).  Lags outside are either not computed or
// computed and harmless: whatever they score is below min_score, so they cannot displace a run that is reported, and a pair
// without such a run is not reported at all.
//
// TABLE ENTRIES.  At the end of a chunk each row is reduced over its lags by one 64-bit key, (kLocaljoinScoreBias - score)
// << 32 | (lag + kLocaljoinLagBias): the smaller key has the larger score, then the smaller lag (scores take 23 bits and lags
// 19 and a sign, more than the local search's packing holds).  Thread m keeps the smallest key of row m over the
// workgroup's chunks and leaves it in the workgroup's own entry (row, b, split) with an ordinary store; the table is preset
// to 0xff in every byte, "no candidate".  LocaljoinSelect is the selection's policy (join_scan.h): the fold of the splits is
// a minimum, a pair is reported with score >= min_score.
// (b) localjoin_popc_kernel computes the same entries by xor/popcount (HPFW_LOCALJOIN_POPC): the second opinion.
// (c) localjoin_ends_kernel walks the diagonal of every written pair once (local_walk): the run's first position, its length
// and its mismatching bits, and the score again, which must be the scan's.
#include "join_scan.h"
#include "local_rule.h"

namespace hpfw {

extern __shared__ __align__(16) unsigned char smem_raw[];

namespace {
static_assert(31 * kSelfjoinMaxLen < kLocaljoinScoreBias && kSelfjoinMaxLen < kLocaljoinLagBias, "a key holds every score and lag");

constexpr unsigned long long kLjNone = ~0ull;

struct LocaljoinArgs : JoinScanArgs { // (min_overlap: min_len)
    int max_rate;
    unsigned long long *tab;    // [32 n_groups][n_clips][splits], every byte preset to 0xff
};

__device__ __forceinline__ unsigned long long lj_key(int score, int lag)
{
    return ((unsigned long long)(unsigned)(kLocaljoinScoreBias - score) << 32) | (unsigned)(lag + kLocaljoinLagBias);
}
__device__ __forceinline__ int lj_score(unsigned long long key) { return kLocaljoinScoreBias - (int)(unsigned)(key >> 32); }
__device__ __forceinline__ int lj_lag(unsigned long long key) { return (int)(unsigned)key - kLocaljoinLagBias; }
__device__ __forceinline__ bool lj_reported(unsigned long long key, int min_score) { return key != kLjNone && lj_score(key) >= min_score; }
} // namespace

__global__ __launch_bounds__(kJoinThreads, 2) void localjoin_mfma_kernel(LocaljoinArgs a)
{
    const int one = 0x7f7f7f7f; // E8M0 scale 2^0
    // the step's constant: every row of +1 times every column with 64 - 2 T values of -1 over K, half h of K in lanes 32 h ..
    const v8i ones_a = {0x22222222, 0x22222222, 0x22222222, 0x22222222, 0, 0, 0, 0};
    const v4i c4 = minus_ones(64 - 2 * a.max_rate - 32 * (int)((threadIdx.x & 63) >> 5));
    const v8i step_b = {c4.x, c4.y, c4.z, c4.w, 0, 0, 0, 0};
    unsigned long long best = kLjNone; // (threads below 32: row tid over the workgroup's chunks)
    f32x16 acc[kJoinTiles];
    i32x16 bs[kJoinTiles];
#pragma unroll
    for (int t = 0; t < kJoinTiles; ++t) {
        acc[t] = f32x16{0};
        bs[t] = i32x16{0};
    }
    const JoinChunk c = join_scan(
        a, smem_raw,
        [&](const v4i *ap, const v4i *bp, int j) {
            scan_products(acc, ap, bp, j);
            // the tiles in turn: the vector work of one tile under the matrix instructions of the tiles after it
#pragma unroll
            for (int t = 0; t < kJoinTiles; ++t) {
                acc[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ones_a, step_b, acc[t], 4, 4, 0, one, 0, one);
                if (t > 0) scan_tile(acc[t - 1], bs[t - 1]);
            }
            scan_tile(acc[kJoinTiles - 1], bs[kJoinTiles - 1]);
        },
        [&](const JoinChunk &c) {
            // bs[t][reg]: twice the best score of row m = (reg & 3) + 8 (reg >> 2) + 4 h at lag d0 + wave 128 + t 32 + n_lane
            unsigned long long *red = static_cast<unsigned long long *>(c.red); // [8 waves][32 rows]
            unsigned long long *wave_red = red + c.wave * 32;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int m = (reg & 3) + 8 * (reg >> 2) + 4 * c.h;
                unsigned long long key = kLjNone;
#pragma unroll
                for (int t = 0; t < kJoinTiles; ++t) {
                    const int score = (int)__int_as_float(bs[t][reg]) >> 1;
                    const unsigned long long cand = lj_key(score, c.d0 + c.wave * kJoinWaveLags + t * 32 + c.n_lane);
                    if (score > 0 && cand < key) key = cand;
                }
#pragma unroll
                for (int s = 16; s >= 1; s >>= 1) { // the best of the 32 lag columns of this half-wave
                    const unsigned long long o = (unsigned long long)__shfl_xor((long long)key, s);
                    key = o < key ? o : key;
                }
                if (c.n_lane == 0) wave_red[m] = key;
            }
            __syncthreads();
            if (c.tid < 32) {
                for (int w = 0; w < kJoinThreads / 64; ++w) best = red[w * 32 + c.tid] < best ? red[w * 32 + c.tid] : best;
            }
#pragma unroll
            for (int t = 0; t < kJoinTiles; ++t) {
                acc[t] = f32x16{0};
                bs[t] = i32x16{0};
            }
        });
    if (c.tid < 32 && c.lens[c.tid] > 0 && best != kLjNone)
        a.tab[((int64_t)(32 * c.p.gi + c.tid) * a.n_clips + c.p.b) * a.splits + c.p.split] = best;
}

// the same pairs, splits and chunks (the chunks of a pair begin at min_len - the group's longest row for every row): a thread
// takes four lags of a chunk and walks their diagonals, one row after the other
__global__ __launch_bounds__(256) void localjoin_popc_kernel(LocaljoinArgs a)
{
    __shared__ unsigned long long red[4];
    __shared__ int lens[32];
    __shared__ int64_t starts[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const JoinPair p = join_pair(a, lens, starts);
    int n;
    const int64_t r0 = sj_clip(a, p.b, n);
    const int ml = a.min_overlap, T = a.max_rate;
    if (n < ml || p.kt == 0) return;
    const uint64_t *r = a.db + r0;
    const int d_lo = ml - p.kt, d_hi = n - ml;
    const int n_wg_chunks = (d_hi - d_lo) / kSelfjoinChunk + 1;
    for (int m = 0; m < 32; ++m) {
        const int k = lens[m];
        if (k == 0) continue;
        const uint64_t *q = a.db + starts[m];
        unsigned long long key = kLjNone;
        for (int wc = p.split; wc < n_wg_chunks; wc += a.splits) {
            const int d0 = d_lo + wc * kSelfjoinChunk;
            for (int e = 0; e < kSelfjoinChunk / 256; ++e) {
                const int d = d0 + tid + 256 * e;
                if (d > d_hi) break;
                const int j0 = max(0, -d), j1 = min(k, n - d);
                if (j1 - j0 < ml) continue; // (a row shorter than the group's longest)
                int pre = 0, mn = 0, bs = 0;
                for (int j = j0; j < j1; ++j) {
                    pre += T - __popcll(q[j] ^ r[d + j]);
                    bs = max(bs, pre - mn);
                    mn = min(mn, pre);
                }
                if (bs > 0) {
                    const unsigned long long cand = lj_key(bs, d);
                    key = cand < key ? cand : key;
                }
            }
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const unsigned long long o = (unsigned long long)__shfl_xor((long long)key, s);
            key = o < key ? o : key;
        }
        __syncthreads(); // (the row before has been read)
        if (lane == 0) red[wave] = key;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; ++w) key = red[w] < key ? red[w] : key;
            if (key != kLjNone) a.tab[((int64_t)(32 * p.gi + m) * a.n_clips + p.b) * a.splits + p.split] = key;
        }
    }
}

namespace {
struct PassagePairDev {
    uint32_t a, b;
    int32_t score, lag;
    uint32_t a_start, length, dist, pad;
};
static_assert(sizeof(PassagePairDev) == sizeof(hpfw_passage_pair), "the record of include/hpfw_gpu.h");

// the selection (join_scan.h) by score: the table's columns are the index's clips; the run's ends are localjoin_ends_kernel's
struct LocaljoinSelect {
    using Entry = unsigned long long;
    using Record = PassagePairDev;
    int min_score;
    static constexpr int col0 = 0;
    static __device__ __forceinline__ Entry none() { return kLjNone; }
    static __device__ __forceinline__ void fold(Entry &b, const Entry e) { b = e < b ? e : b; }
    __device__ __forceinline__ bool reported(const Entry &e) const { return lj_reported(e, min_score); }
    static __device__ __forceinline__ Record record(uint32_t a, uint32_t b, const Entry &e) { return {a, b, lj_score(e), lj_lag(e), 0u, 0u, 0u, 0u}; }
};
} // namespace

// one thread per written pair: the walk of its diagonal
__global__ __launch_bounds__(64) void localjoin_ends_kernel(const uint64_t *__restrict__ db, const int64_t *__restrict__ db_off, int T,
                                                            uint32_t clip_base, PassagePairDev *__restrict__ out, int64_t cap,
                                                            const int64_t *__restrict__ count, unsigned *__restrict__ disagree)
{
    const int64_t n_pairs = min(*count, cap);
    for (int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x; i < n_pairs; i += (int64_t)gridDim.x * 64) {
        PassagePairDev pr = out[i];
        const int64_t q0 = db_off[pr.a - clip_base], r0 = db_off[pr.b - clip_base];
        const int k = (int)(db_off[pr.a - clip_base + 1] - q0), n = (int)(db_off[pr.b - clip_base + 1] - r0);
        const LocalRun run = local_walk(db + q0, db + r0, pr.lag, k, n, T);
        if (run.score != pr.score) atomicAdd(disagree, 1u);
        pr.score = run.score;
        pr.a_start = (uint32_t)run.j0;
        pr.length = (uint32_t)(run.j1 - run.j0);
        pr.dist = (uint32_t)(T * (run.j1 - run.j0) - run.score);
        out[i] = pr;
    }
}

void launch_localjoin_scan(bool popc, const uint64_t *d_db, const int64_t *d_db_off, int n_clips, int g0, int n_groups,
                           const uint32_t *d_pair_first, uint32_t n_pairs, int min_len, int max_rate, int splits, void *d_tab, hipStream_t s)
{
    LocaljoinArgs a = {};
    a.db = d_db;
    a.db_off = d_db_off;
    a.n_clips = n_clips;
    a.g0 = g0;
    a.n_groups = n_groups;
    a.pair_first = d_pair_first;
    a.min_overlap = min_len;
    a.splits = splits;
    a.max_rate = max_rate;
    a.tab = reinterpret_cast<unsigned long long *>(d_tab);
    const dim3 grid(n_pairs * (unsigned)splits);
    if (popc) {
        hipLaunchKernelGGL(localjoin_popc_kernel, grid, dim3(256), 0, s, a);
        return;
    }
    static PerDeviceOnce attr_set;
    if (attr_set.need()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(localjoin_mfma_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)join_scan_lds_bytes());
        attr_set.mark();
    }
    hipLaunchKernelGGL(localjoin_mfma_kernel, grid, dim3(kJoinThreads), join_scan_lds_bytes(), s, a);
}

void launch_localjoin_select(void *d_tab, int n_clips, int splits, int row0, int n_rows, int min_score, int *d_row_count, int64_t *d_row_first,
                             uint32_t clip_base, void *d_out, int64_t cap, int64_t *d_count, hipStream_t s)
{
    launch_join_select(d_tab, n_clips, splits, row0, n_rows, LocaljoinSelect{min_score}, d_row_count, d_row_first, clip_base, d_out, cap, d_count,
                       s);
}

void launch_localjoin_ends(const uint64_t *d_db, const int64_t *d_db_off, int max_rate, uint32_t clip_base, void *d_out, int64_t cap,
                           const int64_t *d_count, unsigned *d_disagree, hipStream_t s)
{
    const unsigned blocks = (unsigned)std::min<int64_t>((cap + 63) / 64, 16384);
    hipLaunchKernelGGL(localjoin_ends_kernel, dim3(blocks), dim3(64), 0, s, d_db, d_db_off, max_rate, clip_base,
                       reinterpret_cast<PassagePairDev *>(d_out), cap, d_count, d_disagree);
}

} // namespace hpfw
