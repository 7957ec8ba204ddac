// k_search_local.hip -- the local search (include/hpfw_gpu.h): the best-scoring run of consecutive
// query hashprints on any diagonal of any clip.  With x_j = T - popcount(q[j] ^ r[d + j]) (T = max_rate, 1..31) a run
// [j0, j1) at lag d scores sum x_j; a clip's candidate is its best run over all lags: larger score, then smaller lag, then
// smaller j1, then smaller j0.  Exact integers throughout.
//
// (a) local_mfma_kernel is the scan of query_scan.h with the clip's window zero-filled on both sides.  The accumulators
// are read after every position j.  With acc_j the accumulator after step j, acc_j - (64 - 2 T)(j + 1) is twice the prefix
// sum of x, where a position outside the query or the clip (fp4 zeros: the product adds nothing) counts as x = T - 32 < 0.
// The best run's score is the largest prefix sum minus the smallest one before it; the scan keeps that difference, not the
// two sums: cur_j = max(cur_{j-1}, 0) + 2 x_j is twice the best run that ends at j, and best = max(best, cur_j) from 0 (only
// positive runs are hits).  The step's constant -(64 - 2 T) comes from the matrix pipe as well -- a second instruction per
// tile multiplies a row of +1 by a column with 64 - 2 T values of -1 -- so the vector pipe is left with two operations per
// accumulator register and step: best = max(best, cur), cur = max(cur, 0) (scan_tile; local_rule.h has it, the constant's
// column and the walk of a diagonal, shared with the local self-join).  Padding lies at a diagonal's two ends only and
// every step of it is strictly negative, so no best run reaches into it: the scores are those of a masked scan.  All values
// are integers below 2^21: exact in f32, in any order.
// A register's lag is fixed, so the scan tracks no position.  A workgroup reduces each row over its lags (larger score, then
// smaller lag) and offers one 64-bit key (kLocalScoreBias - score) << 32 | (lag + kLocalLagBias) to best[query][clip] with
// atomicMin: smaller keys are better, so launch_topk picks the clips unchanged.
// (b) local_popc_kernel computes the same keys by xor/popcount: queries whose window does not fit the LDS, and the second
// opinion on the device (HPFW_LOCAL_POPC).
// (c) local_ends_kernel walks the winning diagonal of each of the n_q k winners once: the run's first position, its length
// and its mismatching bits, and the score again, which must be the scan's.
#include "kernels.h"
#include "local_rule.h"
#include "query_scan.h"

namespace hpfw {

extern __shared__ __align__(16) unsigned char smem_raw[];

namespace {
static_assert(31 * 16000 < kLocalScoreBias, "a score is below the bias");

struct LocalArgs {
    const uint64_t *db;
    const int64_t *db_off;
    int n_clips;
    const uint64_t *q;    // the call's hashprints (xor/popcount kernel)
    const int64_t *q_off; // [n_q + 1] (device), this launch's first query at q_off[0]
    int n_q;
    const v4i *qa;        // expanded queries of this launch (expand_queries_kernel's image)
    int kt_pad;
    const int *gk;        // [2 g]: longest query of group g
    int max_rate;
    int chunks;           // workgroups (of 1024 lags) per clip; the first begins at lag 1 - (the group's longest query; on the
                          // popcount route: the query's length)
    unsigned long long *best; // [n_q][n_clips], every byte preset to 0xff
};

// a chunk's key: (bias - score) << 10 | lag inside the chunk; smaller is better
__device__ __forceinline__ unsigned chunk_key(int score, int lo) { return ((unsigned)(kLocalScoreBias - score) << 10) | (unsigned)lo; }

__device__ __forceinline__ void offer(unsigned long long *best, unsigned key, int d0)
{
    const unsigned long long full = ((unsigned long long)(key >> 10) << 32) | (unsigned)(d0 + (int)(key & 0x3ffu) + kLocalLagBias);
    atomicMin(best, full);
}

} // namespace

__global__ __launch_bounds__(kScanThreads, 2) void local_mfma_kernel(LocalArgs a)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_lane = lane & 31, h = lane >> 5;
    const int clip = blockIdx.x / a.chunks, wc = blockIdx.x - clip * a.chunks, g = blockIdx.y;
    const int64_t r0 = a.db_off[clip];
    const int n = (int)(a.db_off[clip + 1] - r0);
    const int kt = a.gk[2 * g];
    if (n <= 0 || kt <= 0) return;
    const int d0 = 1 - kt + wc * kScanWgLags; // the group's lags run 1 - kt .. n - 1
    if (d0 > n - 1) return;

    const int win = kScanWgLags + kt;
    const ScanLds l = scan_lds(smem_raw, win);
    scan_stage_window(l.B, win, a.db, r0, n, d0, tid);

    f32x16 acc[kScanTiles];
    i32x16 bs[kScanTiles];
#pragma unroll
    for (int t = 0; t < kScanTiles; ++t) {
        acc[t] = f32x16{0};
        bs[t] = i32x16{0};
    }
    const int one = 0x7f7f7f7f; // E8M0 scale 2^0
    // the step's constant: every row of +1 times every column with 64 - 2 T values of -1 over K, half h of K in lanes 32 h ..
    const v8i ones_a = {0x22222222, 0x22222222, 0x22222222, 0x22222222, 0, 0, 0, 0};
    const v4i c4 = minus_ones(64 - 2 * a.max_rate - 32 * h);
    const v8i step_b = {c4.x, c4.y, c4.z, c4.w, 0, 0, 0, 0};
    // a wave whose 128 lags all lie past n - 1 (the clip's last chunk) is not live
    scan_walk(a.qa + (int64_t)g * a.kt_pad * 64, l.A, l.B + h * win + wave * kScanWaveLags + n_lane, kt, d0 + wave * kScanWaveLags <= n - 1, tid,
              lane, [&](const v4i *ap, const v4i *bj, int j) {
                  scan_products(acc, ap, bj, j);
                  // the tiles in turn: the vector work of one tile under the matrix instructions of the tiles after it
#pragma unroll
                  for (int t = 0; t < kScanTiles; ++t) {
                      acc[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ones_a, step_b, acc[t], 4, 4, 0, one, 0, one);
                      if (t > 0) scan_tile(acc[t - 1], bs[t - 1]);
                  }
                  scan_tile(acc[kScanTiles - 1], bs[kScanTiles - 1]);
              });

    // bs[t][reg]: twice the best score of query row m = (reg & 3) + 8 (reg >> 2) + 4 h at lag d0 + wave 128 + t 32 + n_lane
    const unsigned key = scan_row_min(l.red, tid, wave, n_lane, h, [&](int reg, int t) {
        const int score = (int)__int_as_float(bs[t][reg]) >> 1;
        return score > 0 ? chunk_key(score, wave * kScanWaveLags + t * 32 + n_lane) : kScanNoKey;
    });
    const int qi = g * 32 + tid;
    if (tid < 32 && qi < a.n_q && key != kScanNoKey) offer(a.best + (int64_t)qi * a.n_clips + clip, key, d0);
}

// one workgroup per (query, clip, chunk): a thread takes four lags of the chunk and walks their diagonals
__global__ __launch_bounds__(256) void local_popc_kernel(LocalArgs a)
{
    __shared__ unsigned red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int clip = blockIdx.x / a.chunks, wc = blockIdx.x - clip * a.chunks, qi = blockIdx.y;
    const int64_t r0 = a.db_off[clip], q0 = a.q_off[qi];
    const int n = (int)(a.db_off[clip + 1] - r0), k = (int)(a.q_off[qi + 1] - q0), T = a.max_rate;
    if (n <= 0 || k <= 0) return;
    const int d0 = 1 - k + wc * kScanWgLags;
    if (d0 > n - 1) return;
    const uint64_t *q = a.q + q0, *r = a.db + r0;
    unsigned key = kScanNoKey;
    for (int e = 0; e < kScanWgLags / 256; ++e) {
        const int lo = tid + 256 * e, d = d0 + lo;
        if (d > n - 1) break;
        const int ja = max(0, -d), jb = min(k, n - d);
        int p = 0, mn = 0, bs = 0;
        for (int j = ja; j < jb; ++j) {
            p += T - __popcll(q[j] ^ r[d + j]);
            bs = max(bs, p - mn);
            mn = min(mn, p);
        }
        if (bs > 0) key = min(key, chunk_key(bs, lo));
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)key, s);
        key = o < key ? o : key;
    }
    if (lane == 0) red[wave] = key;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) key = red[w] < key ? red[w] : key;
        if (key != kScanNoKey) offer(a.best + (int64_t)qi * a.n_clips + clip, key, d0);
    }
}

namespace {
struct TopHitDev { // launch_topk's record of a winner: dist = bias - score, offset = lag + bias
    uint32_t dist, clip;
    int32_t offset;
    uint32_t pad;
};
struct LocalHitDev {
    int32_t score;
    uint32_t clip;
    int32_t lag;
    uint32_t q_start, length, dist;
};
} // namespace

// one thread per winner: the walk of its diagonal (local_walk)
__global__ __launch_bounds__(64) void local_ends_kernel(const TopHitDev *__restrict__ top, const uint64_t *__restrict__ db,
                                                        const int64_t *__restrict__ db_off, const uint64_t *__restrict__ q_hp,
                                                        const int64_t *__restrict__ q_off, int64_t n_hits, int k_hits, int T,
                                                        uint32_t clip_base, LocalHitDev *__restrict__ out, unsigned *__restrict__ disagree)
{
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n_hits) return;
    LocalHitDev hit = {0, 0xffffffffu, 0, 0u, 0u, 0u};
    if (top && top[i].clip != 0xffffffffu) {
        const int64_t qi = i / k_hits;
        const uint32_t c = top[i].clip - clip_base;
        const int d = top[i].offset - kLocalLagBias, score = kLocalScoreBias - (int)top[i].dist;
        const int64_t r0 = db_off[c], q0 = q_off[qi];
        const int n = (int)(db_off[c + 1] - r0), k = (int)(q_off[qi + 1] - q0);
        const LocalRun run = local_walk(q_hp + q0, db + r0, d, k, n, T);
        if (run.score != score) atomicAdd(disagree, 1u);
        hit = {run.score, top[i].clip, d, (uint32_t)run.j0, (uint32_t)(run.j1 - run.j0), (uint32_t)(T * (run.j1 - run.j0) - run.score)};
    }
    out[i] = hit;
}

void launch_local_mfma(const uint64_t *d_db, const int64_t *d_db_off, int n_clips, const int64_t *d_q_off, int n_q, const void *d_qa,
                       int kt_pad, const int *d_gk, int k_max, int max_rate, int chunks, uint64_t *d_best, hipStream_t s)
{
    static PerDeviceOnce attr_set;
    scan_allow_lds(attr_set, {reinterpret_cast<const void *>(local_mfma_kernel)});
    LocalArgs a = {};
    a.db = d_db;
    a.db_off = d_db_off;
    a.n_clips = n_clips;
    a.q_off = d_q_off;
    a.n_q = n_q;
    a.qa = reinterpret_cast<const v4i *>(d_qa);
    a.kt_pad = kt_pad;
    a.gk = d_gk;
    a.max_rate = max_rate;
    a.chunks = chunks;
    a.best = reinterpret_cast<unsigned long long *>(d_best);
    const dim3 grid((unsigned)n_clips * (unsigned)chunks, (unsigned)((n_q + 31) / 32));
    hipLaunchKernelGGL(local_mfma_kernel, grid, dim3(kScanThreads), query_scan_lds_bytes(k_max), s, a);
}

void launch_local_popc(const uint64_t *d_db, const int64_t *d_db_off, int n_clips, const uint64_t *d_q, const int64_t *d_q_off, int n_q,
                       int max_rate, int chunks, uint64_t *d_best, hipStream_t s)
{
    LocalArgs a = {};
    a.db = d_db;
    a.db_off = d_db_off;
    a.n_clips = n_clips;
    a.q = d_q;
    a.q_off = d_q_off;
    a.n_q = n_q;
    a.max_rate = max_rate;
    a.chunks = chunks;
    a.best = reinterpret_cast<unsigned long long *>(d_best);
    const dim3 grid((unsigned)n_clips * (unsigned)chunks, (unsigned)n_q);
    hipLaunchKernelGGL(local_popc_kernel, grid, dim3(256), 0, s, a);
}

void launch_local_ends(const void *d_top, const uint64_t *d_db, const int64_t *d_db_off, const uint64_t *d_q, const int64_t *d_q_off,
                       int64_t n_q, int k, int max_rate, uint32_t clip_base, void *d_out, unsigned *d_disagree, hipStream_t s)
{
    const int64_t n_hits = n_q * k;
    hipLaunchKernelGGL(local_ends_kernel, dim3((unsigned)((n_hits + 63) / 64)), dim3(64), 0, s, static_cast<const TopHitDev *>(d_top), d_db,
                       d_db_off, d_q, d_q_off, n_hits, k, max_rate, clip_base, static_cast<LocalHitDev *>(d_out), d_disagree);
}

} // namespace hpfw
