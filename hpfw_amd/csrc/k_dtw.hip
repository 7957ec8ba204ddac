// k_dtw.hip -- warped search: subsequence DTW of a query over a clip's hashprints, exact integers.
//
// c(i, j) = popcount(q[i] ^ r[j]);  D(0, j) = c(0, j), S(0, j) = j;  for i >= 1 the cell takes the smallest of
//   A: D(i-1, j-1) + c(i, j)      B: D(i-1, j-2) + c(i, j)      C: D(i-2, j-1) + c(i-1, j) + c(i, j)
// (ties: A, B, C), S follows the chosen predecessor.  Every predecessor lies in an earlier row, so a row is computed at once.
//
// One wave per (query, clip) pair.  Lane l holds the kDtwStrip columns j0 + l kDtwStrip .. of the block in registers: D and S
// of the rows i - 1 and i - 2 and the costs of row i - 1.  Even rows live in one set of registers and odd rows in the other;
// a row is computed from its last column to its first, so that row i overwrites row i - 2 in place (cell j reads row i - 2
// at j - 1 only) and nothing is moved between rows.  After a row a lane hands its last two columns to the lane on its right
// (a DPP wave shift).
// A clip wider than kDtwBlock columns runs in blocks from left to right; the last two columns of a block, for every row,
// wait in a boundary buffer [row]{D(j-1), D(j-2), S(j-1), S(j-2)} that lane (row mod 64) reads and writes 64 rows at a time.
#include "kernels.h"

namespace hpfw {

namespace {

constexpr int W = kDtwStrip;
constexpr uint32_t kInf = 0x3fffffffu; // an unreachable cell; every real D is at most 64 * 16000 < 2^20

struct DtwHitDev {
    uint32_t dist, clip;
    int32_t start, end;
};
struct TopHitDev { // hpfw_hit as launch_topk writes it
    uint32_t dist, clip;
    int32_t offset;
    uint32_t pad;
};

__device__ __forceinline__ uint32_t lane_value(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }

// lane l receives v of lane l - 1 (wave_shr:1); lane 0 receives `old`
__device__ __forceinline__ uint32_t wave_shift_right(uint32_t old, uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x138, 0xf, 0xf, false);
}

__device__ __forceinline__ uint64_t wave_min_key(uint64_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint64_t o = __shfl_xor(v, m);
        v = o < v ? o : v;
    }
    return v;
}

// Row i of one lane's strip: `d1, s1` hold row i - 1, `d2, s2` row i - 2 and receive row i; c1 the costs of row i - 1, then
// of row i.  Left of the strip: (ea, sa) row i - 1 at j0 - 1, (eb, sb) row i - 1 at j0 - 2, (ec, sc) row i - 2 at j0 - 1.
// Returns the 2-bit choices of the strip's cells (A 0, B 1, C 2), cell t in bits 2t.
template <bool PATH, bool FIRST>
__device__ __forceinline__ uint32_t dtw_row(int j0, uint32_t qlo, uint32_t qhi, const uint32_t (&rlo)[W], const uint32_t (&rhi)[W],
                                            const uint32_t (&d1)[W], const uint32_t (&s1)[W], uint32_t (&d2)[W], uint32_t (&s2)[W],
                                            uint32_t (&c1)[W], uint32_t ea, uint32_t sa, uint32_t eb, uint32_t sb, uint32_t ec, uint32_t sc)
{
    uint32_t choices = 0;
#pragma unroll
    for (int t = W - 1; t >= 0; --t) {
        const uint32_t c = (uint32_t)__popc(rlo[t] ^ qlo) + (uint32_t)__popc(rhi[t] ^ qhi);
        if (FIRST) { // row 0 starts anywhere for free
            d2[t] = c;
            s2[t] = (uint32_t)(j0 + t);
        } else {
            // every candidate adds c(i, j): they are compared without it
            uint32_t best = t >= 1 ? d1[t - 1] : ea, s = t >= 1 ? s1[t - 1] : sa;
            const uint32_t pb = t >= 2 ? d1[t - 2] : (t == 1 ? ea : eb), spb = t >= 2 ? s1[t - 2] : (t == 1 ? sa : sb);
            const uint32_t pc = (t >= 1 ? d2[t - 1] : ec) + c1[t], spc = t >= 1 ? s2[t - 1] : sc;
            uint32_t k = 0;
            if (pb < best) {
                best = pb;
                s = spb;
                k = 1;
            }
            if (pc < best) {
                best = pc;
                s = spc;
                k = 2;
            }
            best += c;
            d2[t] = best < kInf ? best : kInf; // (no valid predecessor: best >= kInf)
            s2[t] = s;
            if (PATH) choices |= k << (2 * t);
        }
        c1[t] = c;
    }
    return choices;
}

template <bool PATH>
__global__ __launch_bounds__(64) void dtw_pairs_kernel(DtwArgs a)
{
    const int lane = threadIdx.x;
    uint4 *bnd = a.bnd + (int64_t)blockIdx.x * a.k_max;
    for (int64_t p = blockIdx.x; p < a.n_pairs; p += gridDim.x) {
        int qi, ci;
        if (a.pairs) { // the caller's list
            qi = a.pairs[2 * p];
            ci = a.pairs[2 * p + 1];
        } else if (a.cand) { // the hits of the plain search, per_q of them per query
            qi = (int)(p / a.per_q);
            const uint32_t c = static_cast<const TopHitDev *>(a.cand)[p].clip;
            ci = c == 0xffffffffu ? -1 : (int)(c - a.clip_base);
        } else { // every clip of the index
            qi = (int)(p / a.per_q);
            ci = (int)(p - (int64_t)qi * a.per_q);
        }
        qi = __builtin_amdgcn_readfirstlane(qi);
        ci = __builtin_amdgcn_readfirstlane(ci);
        DtwHitDev hit = {0xffffffffu, 0xffffffffu, 0, 0};
        int K = 0, n = 0;
        const uint64_t *q = a.q, *r = a.db;
        if (ci >= 0) {
            const int64_t q0 = a.q_off[a.q_first + qi], r0 = a.db_off[ci];
            K = __builtin_amdgcn_readfirstlane((int)(a.q_off[a.q_first + qi + 1] - q0));
            n = __builtin_amdgcn_readfirstlane((int)(a.db_off[ci + 1] - r0));
            q += q0;
            r += r0;
        }
        if (K >= 1 && n >= K / 2 + 1) { // (a shorter clip has no reachable cell in the last row)
            const int nb = (n + kDtwBlock - 1) / kDtwBlock;
            uint64_t best_key = ~0ull;
            int best_start = 0;
            for (int b = 0; b < nb; ++b) {
                const int j0 = b * kDtwBlock + lane * W;
                uint32_t rlo[W], rhi[W];
#pragma unroll
                for (int t = 0; t < W; ++t) {
                    const uint64_t v = r[min(j0 + t, n - 1)]; // (columns past the clip are computed and never read: nothing depends on its right)
                    rlo[t] = (uint32_t)v;
                    rhi[t] = (uint32_t)(v >> 32);
                }
                uint32_t de[W], se[W], dod[W], sod[W], c1[W]; // even rows, odd rows, the costs of the row before
#pragma unroll
                for (int t = 0; t < W; ++t) {
                    de[t] = dod[t] = kInf;
                    se[t] = sod[t] = 0;
                    c1[t] = 0;
                }
                uint32_t ea = kInf, sa = 0, eb = kInf, sb = 0, ec = kInf, sc = 0;
                const bool carry_in = b > 0, carry_out = b + 1 < nb;
                for (int i0 = 0; i0 < K; i0 += 64) {
                    const int rows = min(64, K - i0);
                    const uint64_t qv = q[min(i0 + lane, K - 1)];
                    const uint32_t qvlo = (uint32_t)qv, qvhi = (uint32_t)(qv >> 32);
                    uint4 bin = make_uint4(kInf, kInf, 0, 0), bout = make_uint4(kInf, kInf, 0, 0);
                    if (carry_in && lane < rows) bin = bnd[i0 + lane];
                    for (int ii = 0; ii < rows; ++ii) {
                        const int i = i0 + ii;
                        const uint32_t qlo = lane_value(qvlo, ii), qhi = lane_value(qvhi, ii);
                        uint32_t choices, na, nsa, nb_, nsb; // the row's last two columns
                        if (i & 1) {
                            choices = dtw_row<PATH, false>(j0, qlo, qhi, rlo, rhi, de, se, dod, sod, c1, ea, sa, eb, sb, ec, sc);
                            na = dod[W - 1], nsa = sod[W - 1], nb_ = dod[W - 2], nsb = sod[W - 2];
                        } else {
                            if (i == 0)
                                choices = dtw_row<PATH, true>(j0, qlo, qhi, rlo, rhi, dod, sod, de, se, c1, ea, sa, eb, sb, ec, sc);
                            else
                                choices = dtw_row<PATH, false>(j0, qlo, qhi, rlo, rhi, dod, sod, de, se, c1, ea, sa, eb, sb, ec, sc);
                            na = de[W - 1], nsa = se[W - 1], nb_ = de[W - 2], nsb = se[W - 2];
                        }
                        if (PATH) a.choices[((int64_t)i * nb + b) * 64 + lane] = (uint16_t)choices;
                        if (carry_out) { // lane 63's columns go to the row's slot of the boundary buffer
                            const uint32_t x = lane_value(na, 63), y = lane_value(nb_, 63), z = lane_value(nsa, 63), w = lane_value(nsb, 63);
                            if (lane == ii) bout = make_uint4(x, y, z, w);
                        }
                        // what was left of row i - 1 is left of row i - 2 now; the left lane's columns of row i come in
                        ec = ea;
                        sc = sa;
                        // a DPP wave shift by one lane; lane 0 has no source and keeps `old`: the boundary buffer's row, or nothing
                        uint32_t x = kInf, y = kInf, z = 0, w = 0;
                        if (carry_in) x = lane_value(bin.x, ii), y = lane_value(bin.y, ii), z = lane_value(bin.z, ii), w = lane_value(bin.w, ii);
                        ea = wave_shift_right(x, na);
                        eb = wave_shift_right(y, nb_);
                        sa = wave_shift_right(z, nsa);
                        sb = wave_shift_right(w, nsb);
                    }
                    if (carry_out && lane < rows) bnd[i0 + lane] = bout;
                }
                // the last row of this block
                uint64_t key = ~0ull;
                uint32_t start = 0;
#pragma unroll
                for (int t = W - 1; t >= 0; --t) {
                    const uint32_t d = (K - 1) & 1 ? dod[t] : de[t], s = (K - 1) & 1 ? sod[t] : se[t];
                    if (j0 + t < n && d < kInf) { // (descending t: the smallest column of equal distances stays)
                        const uint64_t cand = ((uint64_t)d << 32) | (uint32_t)(j0 + t);
                        if (cand < key) key = cand, start = s;
                    }
                }
                const uint64_t wmin = wave_min_key(key);
                if (wmin < best_key) { // (uniform)
                    const int src = __ffsll((unsigned long long)__ballot(key == wmin)) - 1;
                    best_key = wmin;
                    best_start = (int)__shfl(start, src);
                }
            }
            if (best_key != ~0ull) {
                hit.dist = (uint32_t)(best_key >> 32);
                hit.clip = (uint32_t)ci;
                hit.start = best_start;
                hit.end = (int32_t)(uint32_t)best_key;
            }
        }
        if (lane == 0) {
            static_cast<DtwHitDev *>(a.out)[p] = hit;
            if (a.table) a.table[p] = hit.clip == 0xffffffffu ? ~0ull : ((uint64_t)hit.dist << 32) | (uint32_t)hit.start;
        }
    }
}

// the path of one pair from the recorded choices, walked back from (K - 1, end) by one thread; no candidate: -1 everywhere
__global__ __launch_bounds__(64) void dtw_backtrack_kernel(const uint16_t *__restrict__ choices, int K, int nb, const DtwHitDev *__restrict__ hit,
                                                           int32_t *__restrict__ path)
{
    if (hit->clip == 0xffffffffu) {
        for (int i = threadIdx.x; i < K; i += 64) path[i] = -1;
        return;
    }
    if (threadIdx.x) return;
    int i = K - 1, j = hit->end;
    while (i > 0) {
        j = max(j, 0); // (a reachable cell's predecessors lie in the clip)
        const uint32_t word = choices[((int64_t)i * nb + j / kDtwBlock) * 64 + j % kDtwBlock / W];
        const uint32_t k = (word >> (2 * (j % W))) & 3u;
        path[i] = j;
        if (k == 2 && i >= 2) { // C: rows i - 1 and i lie on column j
            path[i - 1] = j;
            i -= 2;
            j -= 1;
        } else {
            i -= 1;
            j -= k == 1 ? 2 : 1;
        }
    }
    path[0] = max(j, 0);
}

// after launch_topk on the table of a group of queries: the hits' ends from the pairs (per_q = the clips of the index)
__global__ __launch_bounds__(256) void dtw_finish_kernel(const TopHitDev *__restrict__ top, const DtwHitDev *__restrict__ pairs, int64_t n, int k,
                                                         int64_t per_q, uint32_t clip_base, DtwHitDev *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const TopHitDev h = top[i];
    DtwHitDev o = {0xffffffffu, 0xffffffffu, 0, 0};
    if (h.clip != 0xffffffffu) {
        o.dist = h.dist;
        o.clip = h.clip;
        o.start = h.offset;
        o.end = pairs[(i / k) * per_q + (h.clip - clip_base)].end;
    }
    out[i] = o;
}

// re-ranking: one wave per query orders its per_q <= 64 pairs by (dist, clip) and writes the k best
__global__ __launch_bounds__(64) void dtw_rank_kernel(const DtwHitDev *__restrict__ pairs, int per_q, int k, uint32_t clip_base,
                                                      DtwHitDev *__restrict__ out)
{
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    DtwHitDev h = {0xffffffffu, 0xffffffffu, 0, 0};
    if (lane < per_q) h = pairs[q * per_q + lane];
    const uint64_t key = ((uint64_t)h.dist << 32) | h.clip; // (the clips of a query's pairs are distinct; padding last)
    int rank = 0;
    for (int m = 0; m < 64; ++m) {
        const uint64_t o = __shfl(key, m);
        rank += (o < key || (o == key && m < lane)) ? 1 : 0;
    }
    if (h.clip != 0xffffffffu) h.clip += clip_base;
    if (rank < k) out[q * k + rank] = h;
}

} // namespace

void launch_dtw_pairs(const DtwArgs &a, int slots, bool path, hipStream_t s)
{
    if (path)
        hipLaunchKernelGGL(dtw_pairs_kernel<true>, dim3(slots), dim3(64), 0, s, a);
    else
        hipLaunchKernelGGL(dtw_pairs_kernel<false>, dim3(slots), dim3(64), 0, s, a);
}

void launch_dtw_backtrack(const uint16_t *d_choices, int k_q, int n_blocks, const void *d_hit, int32_t *d_path, hipStream_t s)
{
    hipLaunchKernelGGL(dtw_backtrack_kernel, dim3(1), dim3(64), 0, s, d_choices, k_q, n_blocks, static_cast<const DtwHitDev *>(d_hit), d_path);
}

void launch_dtw_finish(const void *d_top, const void *d_pairs, int64_t n_q, int k, int64_t per_q, uint32_t clip_base, void *d_out, hipStream_t s)
{
    const int64_t n = n_q * k;
    hipLaunchKernelGGL(dtw_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, static_cast<const TopHitDev *>(d_top),
                       static_cast<const DtwHitDev *>(d_pairs), n, k, per_q, clip_base, static_cast<DtwHitDev *>(d_out));
}

void launch_dtw_rank(const void *d_pairs, int64_t n_q, int per_q, int k, uint32_t clip_base, void *d_out, hipStream_t s)
{
    hipLaunchKernelGGL(dtw_rank_kernel, dim3((unsigned)n_q), dim3(64), 0, s, static_cast<const DtwHitDev *>(d_pairs), per_q, k, clip_base,
                       static_cast<DtwHitDev *>(d_out));
}

} // namespace hpfw
