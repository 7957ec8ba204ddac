// k_localjoin.hip -- the local self-join (include/hpfw_gpu.h): for clips a < b of the index the
// best-scoring run of consecutive hashprints of a on any diagonal of b, and every pair whose run scores at least min_score.
//
// Clip a takes the query's part of the local search (section 25) and b the clip's: lag d puts position j of a on position
// d + j of b, x_j = T - popcount(a[j] ^ b[d + j]) (T = max_rate, 1..31), a run [j0, j1) scores sum x_j, and the pair's
// candidate is its best run over all lags: larger score, then smaller lag, then smaller j1, then smaller j0.  Exact integers.
//
// (a) localjoin_mfma_kernel has selfjoin_mfma_kernel's geometry (k_selfjoin.hip): a workgroup = 32 rows (clips a of one row
// group) x kSelfjoinChunk lags of one b per chunk, its pair found in pair_first by binary search, the chunks of a pair dealt
// to `splits` workgroups, rows walked in slices of kSelfjoinSlice positions, both operands read from the index where it lies
// and expanded to fp4 +-1 while they are staged, fp4 0 outside either recording.  Per position it does local_mfma_kernel's
// work (k_search_local.hip): one product instruction per tile, one instruction per tile that adds the step's constant (a row
// of +1 against a column with 64 - 2 T values of -1), then best = max(best, cur), cur = max(cur, 0) on the bit patterns as
// signed integers.  cur is the accumulator itself: after a step it holds twice the best run that ends there.  acc and best
// stay in registers across slices, so the LDS does not depend on a recording's length.  A position outside a or b
// multiplies fp4 zeros and so counts as x = T - 32 < 0.  All values are integers of magnitude at most 2 * 31 * L + 64 <
// 2^24 (kernels.h asserts it): exact in f32, in any order.
//
// SKIPPED SLICES.  As the self-join, a chunk stages only the slices whose window of b meets b.  (1) In a slice whose window
// lies wholly before b's start every position of every lag of the chunk is outside b, so every step is T - 32 < 0: from
// cur = 0, where the chunk starts, each step leaves cur < 0 and the clamp returns it to 0, and best does not move -- the
// state after the slice is the state before it.  (2) In a slice whose window lies wholly past b's end every step is
// strictly negative as well, so cur only falls (or is clamped) and best = max(best, cur) cannot rise; no slice follows that
// could use cur.  The same holds for positions at or past the longest row.  (3) A slice that IS staged runs the constant's
// instruction at every one of its positions for every tile of every live wave, whether or not the lag has left b there: the
// loop below has no per-lag or per-position condition, only `live`, which switches off a whole wave whose 128 lags all lie
// past the last admissible lag (those lags are never read: see PRUNING).
//
// MASKED ROWS.  Rows with a >= b (the triangle cuts through a group), rows that do not exist, empty rows and rows shorter
// than min_len are given length 0: they are staged as fp4 zeros, every step of theirs is T - 32 < 0, their best stays 0,
// a score of 0 makes no candidate, and the final store is skipped for them.
//
// PRUNING.  A run that scores at least min_score has at least min_len = ceil(min_score / T) positions (x_j <= T), so it
// lies on a lag with overlap L(d) >= min_len: the chunks of a pair cover the lags min_len - kt .. n_b - min_len only (kt:
// the group's longest unmasked row).  Lags outside are either not computed or computed and harmless: whatever they score
// is below min_score, so they cannot displace a run that is reported, and a pair without such a run is not reported at all.
//
// TABLE ENTRIES.  At the end of a chunk each row is reduced over its lags by one 64-bit key, (kLocaljoinScoreBias - score)
// << 32 | (lag + kLocaljoinLagBias): the smaller key has the larger score, then the smaller lag (scores take 23 bits and lags
// 19 and a sign, more than the local search's packing holds).  Thread m keeps the smallest key of row m over the
// workgroup's chunks and leaves it in the workgroup's own entry (row, b, split) with an ordinary store; the table is preset
// to 0xff in every byte, "no candidate".  localjoin_count_kernel folds the splits (a minimum) and counts a row's pairs with
// score >= min_score, localjoin_offsets_kernel turns the counts into positions, localjoin_write_kernel writes the pairs in
// (a, b) order below cap: no atomics, nothing depends on the order workgroups run in.
// (b) localjoin_popc_kernel computes the same entries by xor/popcount (HPFW_LOCALJOIN_POPC): the second opinion.
// (c) localjoin_ends_kernel walks the diagonal of every written pair once: the run's first position, its length and its
// mismatching bits, and the score again, which must be the scan's.
#include "kernels.h"
#include "overlap_rule.h"

namespace hpfw {

extern __shared__ __align__(16) unsigned char smem_raw[];

typedef int v8i __attribute__((ext_vector_type(8)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

namespace {
constexpr int kLjThreads = 512;                            // 8 waves
constexpr int kLjTiles = 4;                                // lag tiles of 32 per wave
constexpr int kLjWaveLags = 32 * kLjTiles;                 // 128
constexpr int kLjWin = kSelfjoinChunk + kSelfjoinSlice;    // positions of b staged per slice (one spare)
constexpr int kLjBLoads = (kLjWin + kLjThreads - 1) / kLjThreads; // positions of b per thread and slice
static_assert(kLjWaveLags * (kLjThreads / 64) == kSelfjoinChunk, "kernels.h states the chunk");
static_assert(kSelfjoinSlice == 32 && kLjThreads == 512, "the staging deals 32 positions x 32 rows to 512 threads, two each");
static_assert(31 * kSelfjoinMaxLen < kLocaljoinScoreBias && kSelfjoinMaxLen < kLocaljoinLagBias, "a key holds every score and lag");

constexpr unsigned long long kLjNone = ~0ull;

struct LocaljoinArgs {
    const uint64_t *db;
    const int64_t *db_off;
    int n_clips;
    int g0, n_groups;           // the pass: row groups g0 .. g0 + n_groups - 1 (rows 32 g .. 32 g + 31)
    const uint32_t *pair_first; // [n_groups + 1]: group g0 + i has the pairs pair_first[i] .. pair_first[i + 1] - 1, one per b > 32 (g0 + i)
    int min_len, splits, max_rate;
    unsigned long long *tab;    // [32 n_groups][n_clips][splits], every byte preset to 0xff
};

__device__ __forceinline__ unsigned long long lj_key(int score, int lag)
{
    return ((unsigned long long)(unsigned)(kLocaljoinScoreBias - score) << 32) | (unsigned)(lag + kLocaljoinLagBias);
}
__device__ __forceinline__ int lj_score(unsigned long long key) { return kLocaljoinScoreBias - (int)(unsigned)(key >> 32); }
__device__ __forceinline__ int lj_lag(unsigned long long key) { return (int)(unsigned)key - kLocaljoinLagBias; }
__device__ __forceinline__ bool lj_reported(unsigned long long key, int min_score) { return key != kLjNone && lj_score(key) >= min_score; }

// the workgroup's pair and split; the rows' lengths (0: masked) and starts; kt, the longest unmasked row
struct LjPair {
    int gi, b, split, kt;
};
__device__ __forceinline__ LjPair lj_pair(const LocaljoinArgs &a, int *lens, int64_t *starts)
{
    LjPair p;
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
    p.b = 32 * (a.g0 + lo) + 1 + (int)(pair - a.pair_first[lo]);
    if (threadIdx.x < 32) {
        const int row = 32 * (a.g0 + lo) + (int)threadIdx.x;
        int k = 0;
        int64_t o = 0;
        if (row < p.b) { // (b < n_clips: the row exists)
            o = a.db_off[row];
            k = (int)(a.db_off[row + 1] - o);
            if (k < a.min_len) k = 0;
        }
        lens[threadIdx.x] = k;
        starts[threadIdx.x] = o;
    }
    __syncthreads();
    p.kt = 0;
    for (int m = 0; m < 32; ++m) p.kt = max(p.kt, lens[m]);
    return p;
}

// one accumulator tile after a step (k_search_local.hip's scan_tile restated): cur is twice the best run that ends here; a
// run that scores below 0 is not continued.  Both maxima are taken on the bit patterns as signed integers (bs holds
// best's): the other operand is never negative, and against a value >= 0 the two orders agree.
__device__ __forceinline__ void lj_scan_tile(f32x16 &cur, i32x16 &bs)
{
    i32x16 c = __builtin_bit_cast(i32x16, cur);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        bs[reg] = max(bs[reg], c[reg]);
        c[reg] = max(c[reg], 0);
    }
    cur = __builtin_bit_cast(f32x16, c);
}

// 32 fp4 values of a lane's half of K: the first `cnt` are -1.0 (0xA), the others 0
__device__ __forceinline__ v4i lj_minus_ones(int cnt)
{
    v4i r;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int nib = min(max(cnt - 8 * w, 0), 8);
        r[w] = nib == 8 ? (int)0xAAAAAAAAu : (int)(0xAAAAAAAAu & ((1u << (4 * nib)) - 1u));
    }
    return r;
}
} // namespace

__global__ __launch_bounds__(kLjThreads, 2) void localjoin_mfma_kernel(LocaljoinArgs a)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_lane = lane & 31, h = lane >> 5;
    v4i *ldsB = reinterpret_cast<v4i *>(smem_raw);           // [2][kLjWin]: plane h = bits [32 h, 32 h + 32) of each hashprint
    v4i *ldsA = ldsB + 2 * kLjWin;                           // [kSelfjoinSlice][64]: lane (m, h) of position j
    int64_t *starts = reinterpret_cast<int64_t *>(ldsA + kSelfjoinSlice * 64); // [32]
    int *lens = reinterpret_cast<int *>(starts + 32);        // [32]
    unsigned long long *red = reinterpret_cast<unsigned long long *>(ldsA); // [8 waves][32 rows], over the A operand once a chunk is done

    const LjPair p = lj_pair(a, lens, starts);
    const int64_t r0 = a.db_off[p.b];
    const int n = (int)(a.db_off[p.b + 1] - r0);
    const int kt = p.kt, ml = a.min_len;
    if (n < ml || kt == 0) return; // no row of the group has a run to report in this clip
    const int d_lo = ml - kt, d_hi = n - ml;
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
    const v4i *bp = ldsB + h * kLjWin + wave * kLjWaveLags + n_lane;
    const v4i *ap = ldsA + lane;
    // the step's constant: every row of +1 times every column with 64 - 2 T values of -1 over K, half h of K in lanes 32 h ..
    const v8i ones_a = {0x22222222, 0x22222222, 0x22222222, 0x22222222, 0, 0, 0, 0};
    const v4i c4 = lj_minus_ones(64 - 2 * a.max_rate - 32 * h);
    const v8i step_b = {c4.x, c4.y, c4.z, c4.w, 0, 0, 0, 0};
    unsigned long long best = kLjNone; // (threads below 32: row tid over the workgroup's chunks)

    for (int wc = p.split; wc < n_wg_chunks; wc += a.splits) {
        const int d0 = d_lo + wc * kSelfjoinChunk;
        // slices j0 (multiples of kSelfjoinSlice) whose window of b, positions d0 + j0 .. d0 + j0 + kLjWin - 1, meets the clip
        const int before = -d0 - kLjWin + 1; // j0 >= before
        const int j_begin = before <= 0 ? 0 : (before + kSelfjoinSlice - 1) / kSelfjoinSlice * kSelfjoinSlice;
        const int j_end = min(kt, n - d0);   // j0 < j_end
        f32x16 acc[kLjTiles];
        i32x16 bs[kLjTiles];
#pragma unroll
        for (int t = 0; t < kLjTiles; ++t) {
            acc[t] = f32x16{0};
            bs[t] = i32x16{0};
        }
        // a wave whose 128 lags all lie past n - min_len (the clip's last chunk) multiplies nothing: it only helps staging
        const bool live = d0 + wave * kLjWaveLags <= d_hi;

        uint64_t ra[2], rb[kLjBLoads];
        unsigned ok = 0; // bit e: ra[e] is a hashprint of its row; bit 2 + e: rb[e] is a hashprint of b
        auto load = [&](int j0) {
            ok = 0;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                ra[e] = 0;
                if (j0 + ja[e] < ka[e]) {
                    ra[e] = a.db[oa[e] + j0 + ja[e]];
                    ok |= 1u << e;
                }
            }
#pragma unroll
            for (int e = 0; e < kLjBLoads; ++e) {
                const int i = tid + kLjThreads * e, gi = d0 + j0 + i;
                rb[e] = 0;
                if (i < kLjWin && gi >= 0 && gi < n) {
                    rb[e] = a.db[r0 + gi];
                    ok |= 4u << e;
                }
            }
        };
        load(j_begin);
        for (int j0 = j_begin; j0 < j_end; j0 += kSelfjoinSlice) {
            __syncthreads(); // the slice before this one, or the chunk's keys, have been read
            const v4i zero = {0, 0, 0, 0};
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const bool v = (ok >> e) & 1u;
                ldsA[ja[e] * 64 + ma[e]] = v ? expand32((uint32_t)ra[e]) : zero;
                ldsA[ja[e] * 64 + 32 + ma[e]] = v ? expand32((uint32_t)(ra[e] >> 32)) : zero;
            }
#pragma unroll
            for (int e = 0; e < kLjBLoads; ++e) {
                const int i = tid + kLjThreads * e;
                if (i < kLjWin) {
                    const bool v = (ok >> (2 + e)) & 1u;
                    ldsB[i] = v ? expand32((uint32_t)rb[e]) : zero;
                    ldsB[kLjWin + i] = v ? expand32((uint32_t)(rb[e] >> 32)) : zero;
                }
            }
            __syncthreads();
            if (j0 + kSelfjoinSlice < j_end) load(j0 + kSelfjoinSlice); // the next slice into registers while this one multiplies
            const int jn = min(kSelfjoinSlice, kt - j0);
            for (int j = 0; live && j < jn; ++j) {
                const v4i a4 = ap[j * 64];
                const v8i av = {a4.x, a4.y, a4.z, a4.w, 0, 0, 0, 0};
                // the tiles in turn: the vector work of one tile under the matrix instructions of the tiles after it
#pragma unroll
                for (int t = 0; t < kLjTiles; ++t) {
                    const v4i b4 = bp[j + 32 * t];
                    const v8i bv = {b4.x, b4.y, b4.z, b4.w, 0, 0, 0, 0};
                    acc[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc[t], 4, 4, 0, one, 0, one);
                }
#pragma unroll
                for (int t = 0; t < kLjTiles; ++t) {
                    acc[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ones_a, step_b, acc[t], 4, 4, 0, one, 0, one);
                    if (t > 0) lj_scan_tile(acc[t - 1], bs[t - 1]);
                }
                lj_scan_tile(acc[kLjTiles - 1], bs[kLjTiles - 1]);
            }
        }
        __syncthreads(); // the last slice has been read: the keys go over the A operand

        // bs[t][reg]: twice the best score of row m = (reg & 3) + 8 (reg >> 2) + 4 h at lag d0 + wave 128 + t 32 + n_lane
        unsigned long long *wave_red = red + wave * 32;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int m = (reg & 3) + 8 * (reg >> 2) + 4 * h;
            unsigned long long key = kLjNone;
#pragma unroll
            for (int t = 0; t < kLjTiles; ++t) {
                const int score = (int)__int_as_float(bs[t][reg]) >> 1;
                const unsigned long long cand = lj_key(score, d0 + wave * kLjWaveLags + t * 32 + n_lane);
                if (score > 0 && cand < key) key = cand;
            }
#pragma unroll
            for (int s = 16; s >= 1; s >>= 1) { // the best of the 32 lag columns of this half-wave
                const unsigned long long o = (unsigned long long)__shfl_xor((long long)key, s);
                key = o < key ? o : key;
            }
            if (n_lane == 0) wave_red[m] = key;
        }
        __syncthreads();
        if (tid < 32) {
            for (int w = 0; w < kLjThreads / 64; ++w) best = red[w * 32 + tid] < best ? red[w * 32 + tid] : best;
        }
    }
    if (tid < 32 && lens[tid] > 0 && best != kLjNone)
        a.tab[((int64_t)(32 * p.gi + tid) * a.n_clips + p.b) * a.splits + p.split] = best;
}

// the same pairs, splits and chunks (the chunks of a pair begin at min_len - the group's longest row for every row): a thread
// takes four lags of a chunk and walks their diagonals, one row after the other
__global__ __launch_bounds__(256) void localjoin_popc_kernel(LocaljoinArgs a)
{
    __shared__ unsigned long long red[4];
    __shared__ int lens[32];
    __shared__ int64_t starts[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const LjPair p = lj_pair(a, lens, starts);
    const int64_t r0 = a.db_off[p.b];
    const int n = (int)(a.db_off[p.b + 1] - r0);
    const int ml = a.min_len, T = a.max_rate;
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

// one workgroup per row a of the pass: the splits of every b > a folded into the pair's first entry, and the row's pairs
// with score >= min_score counted
__global__ __launch_bounds__(256) void localjoin_count_kernel(unsigned long long *__restrict__ tab, int n_clips, int splits, int row0, int min_score,
                                                              int *__restrict__ row_count)
{
    __shared__ int red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long *row = tab + (int64_t)blockIdx.x * n_clips * splits;
    int cnt = 0;
    for (int c = row0 + (int)blockIdx.x + 1 + tid; c < n_clips; c += 256) {
        unsigned long long b = row[(int64_t)c * splits];
        for (int s = 1; s < splits; ++s) {
            const unsigned long long e = row[(int64_t)c * splits + s];
            b = e < b ? e : b;
        }
        if (splits > 1) row[(int64_t)c * splits] = b;
        cnt += lj_reported(b, min_score) ? 1 : 0;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) cnt += __shfl_xor(cnt, s);
    if (lane == 0) red[wave] = cnt;
    __syncthreads();
    if (tid == 0) row_count[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// one workgroup: row_first[i] = *total + the counts of the pass's rows before i, then *total += the pass's pairs
__global__ __launch_bounds__(1024) void localjoin_offsets_kernel(const int *__restrict__ row_count, int n_rows, int64_t *__restrict__ row_first,
                                                                 int64_t *__restrict__ total)
{
    __shared__ int64_t part[1024];
    const int tid = threadIdx.x;
    const int per = (n_rows + 1023) / 1024, i0 = min(n_rows, tid * per), i1 = min(n_rows, i0 + per);
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
struct PassagePairDev {
    uint32_t a, b;
    int32_t score, lag;
    uint32_t a_start, length, dist, pad;
};
static_assert(sizeof(PassagePairDev) == sizeof(hpfw_passage_pair), "the record of include/hpfw_gpu.h");
} // namespace

// one workgroup per row a: its pairs with score >= min_score in rising b, from position row_first[a] on, while below cap;
// the run's ends are localjoin_ends_kernel's
__global__ __launch_bounds__(256) void localjoin_write_kernel(const unsigned long long *__restrict__ tab, int n_clips, int splits, int row0,
                                                              int min_score, const int64_t *__restrict__ row_first, uint32_t clip_base,
                                                              PassagePairDev *__restrict__ out, int64_t cap)
{
    __shared__ int wave_n[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = row0 + (int)blockIdx.x;
    const unsigned long long *row = tab + (int64_t)blockIdx.x * n_clips * splits;
    int64_t at = row_first[blockIdx.x];
    for (int c0 = a + 1; c0 < n_clips && at < cap; c0 += 256) {
        const int c = c0 + tid;
        unsigned long long e = kLjNone;
        if (c < n_clips) e = row[(int64_t)c * splits];
        const bool rep = lj_reported(e, min_score);
        const unsigned long long mask = __ballot(rep);
        __syncthreads(); // (the block of 256 before has been read)
        if (lane == 0) wave_n[wave] = __popcll(mask);
        __syncthreads();
        int64_t mine = at + __popcll(mask & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) mine += wave_n[w];
        if (rep && mine < cap) out[mine] = {clip_base + (uint32_t)a, clip_base + (uint32_t)c, lj_score(e), lj_lag(e), 0u, 0u, 0u, 0u};
        at += wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
    }
}

// one thread per written pair: the forward pass over its diagonal -- prefix minimum updated on strict <, best on strict >
__global__ __launch_bounds__(64) void localjoin_ends_kernel(const uint64_t *__restrict__ db, const int64_t *__restrict__ db_off, int T,
                                                            uint32_t clip_base, PassagePairDev *__restrict__ out, int64_t cap,
                                                            const int64_t *__restrict__ count, unsigned *__restrict__ disagree)
{
    const int64_t n_pairs = min(*count, cap);
    for (int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x; i < n_pairs; i += (int64_t)gridDim.x * 64) {
        PassagePairDev pr = out[i];
        const int64_t q0 = db_off[pr.a - clip_base], r0 = db_off[pr.b - clip_base];
        const int k = (int)(db_off[pr.a - clip_base + 1] - q0), n = (int)(db_off[pr.b - clip_base + 1] - r0);
        const uint64_t *q = db + q0, *r = db + r0;
        const int d = pr.lag;
        const int ja = max(0, -d), jb = min(k, n - d);
        int p = 0, mn = 0, mpos = ja, bs = 0, j0 = ja, j1 = ja;
        for (int j = ja; j < jb; ++j) {
            p += T - __popcll(q[j] ^ r[d + j]);
            if (p - mn > bs) {
                bs = p - mn;
                j0 = mpos;
                j1 = j + 1;
            }
            if (p < mn) {
                mn = p;
                mpos = j + 1;
            }
        }
        if (bs != pr.score) atomicAdd(disagree, 1u);
        pr.score = bs;
        pr.a_start = (uint32_t)j0;
        pr.length = (uint32_t)(j1 - j0);
        pr.dist = (uint32_t)(T * (j1 - j0) - bs);
        out[i] = pr;
    }
}

size_t localjoin_mfma_lds_bytes() { return (size_t)2 * kLjWin * 16 + (size_t)kSelfjoinSlice * 64 * 16 + 32 * 8 + 32 * 4; }

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
    a.min_len = min_len;
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
                                  (int)localjoin_mfma_lds_bytes());
        attr_set.mark();
    }
    hipLaunchKernelGGL(localjoin_mfma_kernel, grid, dim3(kLjThreads), localjoin_mfma_lds_bytes(), s, a);
}

void launch_localjoin_select(void *d_tab, int n_clips, int splits, int row0, int n_rows, int min_score, int *d_row_count, int64_t *d_row_first,
                             uint32_t clip_base, void *d_out, int64_t cap, int64_t *d_count, hipStream_t s)
{
    hipLaunchKernelGGL(localjoin_count_kernel, dim3(n_rows), dim3(256), 0, s, reinterpret_cast<unsigned long long *>(d_tab), n_clips, splits,
                       row0, min_score, d_row_count);
    hipLaunchKernelGGL(localjoin_offsets_kernel, dim3(1), dim3(1024), 0, s, d_row_count, n_rows, d_row_first, d_count);
    if (cap > 0)
        hipLaunchKernelGGL(localjoin_write_kernel, dim3(n_rows), dim3(256), 0, s, reinterpret_cast<const unsigned long long *>(d_tab), n_clips,
                           splits, row0, min_score, d_row_first, clip_base, reinterpret_cast<PassagePairDev *>(d_out), cap);
}

void launch_localjoin_ends(const uint64_t *d_db, const int64_t *d_db_off, int max_rate, uint32_t clip_base, void *d_out, int64_t cap,
                           const int64_t *d_count, unsigned *d_disagree, hipStream_t s)
{
    const unsigned blocks = (unsigned)std::min<int64_t>((cap + 63) / 64, 16384);
    hipLaunchKernelGGL(localjoin_ends_kernel, dim3(blocks), dim3(64), 0, s, d_db, d_db_off, max_rate, clip_base,
                       reinterpret_cast<PassagePairDev *>(d_out), cap, d_count, d_disagree);
}

} // namespace hpfw
