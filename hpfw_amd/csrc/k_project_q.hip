// k_project_q.hip -- a4 (reference level and clip), a5..a8 in fixed point: dB terms -> 64-bit hashprints in ONE kernel
// (DESIGN.md S9q / S10q).
//
// The reference multiplies filters and frames in f32 (an Eigen/MKL sgemm [64 x 2420] . [2420 x n_frames],
// include/hpfw/core/parallel_collector.h:57,127) and keeps only the SIGN of P[r,i] - P[r,i+80]
// (hashprint_handle.h:119-122).  Here both factors are rounded once to fixed point,
//   u[b][c]  = rint(S[b][c] * 98304)                         (S in [-80, 0] dB; 98304 = 3 * 2^15)
//   fq[r][k] = rint(F[r][k] * 2^(21 - ilogb(max_k |F[r][k]|)))   (a positive power of two per row: no sign changes)
// and the difference is taken BEFORE the product: with Du[b][c] = u[b][c] - u[b][c + 80] (|Du| <= 80 * 98304 < 2^23),
//   D[r][i] = Pq[r][i] - Pq[r][i + 80] = sum_{b,t} fq[r][20 b + t] * Du[b][i + t]
// exactly -- integers have no rounding and no summation order -- and bit (63 - r) of hp[i] = (D[r][i] >= 0).  No
// projection ever exists in memory: the kernel reads the dB terms and writes hashprints.
// Both factors are split into three balanced base-256 digits (d in [-128, 127]: x = d0 + 256 d1 + 65536 d2) and the
// 2420-term sums of the nine digit products run on v_mfma_i32_32x32x32_i8 (32 cycles per instruction and SIMD: 16 times
// the multiply-adds per clock of the f32 form); digit products of equal weight share an int32 accumulator
// (|sum| <= 3 * 2420 * 128 * 128 < 2^27), D = sum_c acc_c 2^(8c) in int64.
//
// K is taken as k' = 128 t + bin (bins padded to 128 with zero digits) so that the sixteen bytes a lane hands the
// matrix instruction are sixteen consecutive bins of one column.  A workgroup = 4 waves = 64 filters x 128 hashprints,
// and a wave = 16 FILTERS x all 128 hashprints on v_mfma_i32_16x16x64_i8: the digits of the workgroup's
// [121 bins][128 + 19 columns] slab of Du live in LDS as 16-byte units [bin chunk][column][digit], shared and read-only
// after the prologue, while every wave takes the digits of ITS filters straight from L2 into registers (3 KB per step of
// 64 k', two steps ahead) -- nothing is exchanged between the waves in the main loop, so it has no barrier: the two
// waves of a SIMD (two workgroups share a CU: 62 KB of LDS, 256 registers) interleave their matrix instructions freely,
// and one workgroup's staging (loads, quantisation: vector ALU) and epilogue run under the other's products.
//
// The extraction's unshifted launches form only the six digit products of weight >= 2^16 (hashprint_q6_kernel) and settle
// the few values whose sign those leave open in the same workgroup, from the digits still in its slab, before the
// hashprints are stored: one launch, one pass over the spectrogram, hp written once.
//
// Every kernel here is hashprint_q_tile<FROM_T, SHIFTED, NP>, and a tile is its parts in this order: q_stage_slab (the digits
// of Du into LDS), then per filter image q_matrix_loop<NP> (the digit products), q_epilogue<NP> (D, its sign bits, the open
// values listed), for six products q_settle_open (the listed values from the slab), and q_pack.
//
// The slab is staged by chains: the 147 columns of Du need u of 227 columns, and a thread that holds u of column r, r + 80
// and r + 160 forms Du[r] and Du[r + 80] from them, so every dB term is loaded and quantised once per workgroup (1816
// column-units of 16 bins where a unit per slab column with its partner took 2352); the digit planes are gathered by
// byte permutes, and a thread's five tasks keep the loads of two tasks in flight beyond the one it quantises.  Where a
// clip's last tile is short, the short tiles of all clips are dispatched behind the full ones (q_tile_of_workgroup).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "kernels.h"

namespace hpfw {

extern __shared__ __align__(16) unsigned char smem_raw[];

typedef int v2i __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int kQThreads = 256;                 // 4 waves; each owns 16 filters x 128 hashprints
constexpr int kQTileN = 128;                   // hashprints per workgroup
constexpr int kQCols = kQTileN + kCtx - 1;     // 147 columns of Du in the slab
constexpr int kQPitch = 160;                   // columns per chunk as stored: with this pitch the operand reads (ds_read_b128,
                                               // lanes = 16 columns x 4 chunks) meet no bank conflict (147 .. 157: two-way)
constexpr int kQChunks = 8;                    // bin chunks of 16 (121 bins padded to 128)
constexpr int kQUnit = 48;                     // bytes per (chunk, column): three digits x 16 bins
constexpr int kQSlabBytes = kQChunks * kQPitch * kQUnit;      // 61 440
constexpr int kQStepBytes = 3 * 64 * 16;                      // a wave's filter digits of one step (t, half of the chunks): [digit][lane][16] = 3 072
constexpr int kQSteps = 2 * kCtx;                             // 40 steps of 64 k'
constexpr int kQLdsBytes = kQSlabBytes + kQTileN * 4 * 2;     // + the waves' 16-bit parts of every hashprint: 62 464, two workgroups per CU
constexpr float kQScale = 98304.0f;
// six-product split: open values listed per tile of 128 hashprints, kQCap 16-bit entries (r << 7 | n - n0) each
// in LDS, kQRedo in place of a count above it
constexpr int kQCap = 128;
constexpr unsigned kQRedo = 0xffffffffu;
constexpr int kQListAt = kQLdsBytes + 16;                     // behind the workgroup's count of open values:
constexpr int kQLdsBytes6 = kQListAt + kQCap * 2;             // its list of them: 62 736, still two workgroups per CU

// the three balanced base-256 digits of u as the three low bytes of one word (|u| < 2^23)
__device__ __forceinline__ unsigned q_digit_bytes(int u) { return ((unsigned)u + 0x808080u) ^ 0x808080u; }

#if defined(HPFW_Q_STAMPS)
// diagnosis build (tools/q_stamps.py extract): where the extraction's six-product kernel, which has no dbg argument, leaves its stamps
__device__ long long *g_q_stamps_dev = nullptr;
#endif

__device__ __forceinline__ int q_fixed(float s)
{
    return (int)__builtin_rintf(__builtin_fminf(__builtin_fmaxf(s, -80.0f), 0.0f) * kQScale);
}

// The staging's tasks ("one quantisation per dB term"): Du[col] = u[col] - u[col + 80], so the slab's 147 columns
// need u of the 227 columns n0 .. n0 + 226, and these fall into 80 chains r, r + 80, r + 160 (r < 80; the third only for
// r < 67).  A task = (half chunk qh: bins 8 qh .. 8 qh + 7, residue r): it loads and quantises its chain once and forms
// Du[r] and, for r < 67, Du[r + 80] from it -- every (bin, column) is loaded and passed through q_fixed by exactly one
// thread of the workgroup.  16 half chunks x 80 residues = 1280 tasks, five per thread, 24 loads each.
constexpr int kQHeavy = kQCols - kLag;                        // 67 residues whose chain holds two slab columns
constexpr int kQTasks = 2 * kQChunks * kLag / kQThreads;      // 5 tasks per thread
constexpr int kQAhead = 2;                                    // tasks whose loads are in flight beyond the one being quantised
static_assert(kQTasks * kQThreads == 2 * kQChunks * kLag && kQHeavy > 0 && kQHeavy <= kLag, "1280 tasks, five per thread");

// Digit planes of four elements: w[e] = q_digit_bytes of element e (digit j in byte j).  Returns in p[j] the dword of plane
// j, element e's digit in byte e.  v_perm_b32 takes bytes 0..3 of its selector's range from the SECOND operand, 4..7 from the first.
__device__ __forceinline__ void q_planes(const unsigned (&w)[4], unsigned (&p)[3])
{
    const unsigned t01 = __builtin_amdgcn_perm(w[1], w[0], 0x05010400u); // [w0.b0, w1.b0, w0.b1, w1.b1]
    const unsigned t23 = __builtin_amdgcn_perm(w[3], w[2], 0x05010400u);
    const unsigned u01 = __builtin_amdgcn_perm(w[1], w[0], 0x0c0c0602u); // [w0.b2, w1.b2, 0, 0]
    const unsigned u23 = __builtin_amdgcn_perm(w[3], w[2], 0x0c0c0602u);
    p[0] = __builtin_amdgcn_perm(t23, t01, 0x05040100u);
    p[1] = __builtin_amdgcn_perm(t23, t01, 0x07060302u);
    p[2] = __builtin_amdgcn_perm(u23, u01, 0x05040100u);
}

// One wave forms D[r][n0 + nl] exactly from digits alone (r, nl the same in every lane).  The 2420 taps are 160 pairs of
// 16-byte units, pair (s, g) = step s = 2 t + p of the matrix loop and its group g of 16 bins 64 p + 16 g + e:
//   filter unit of digit i: the image's wave r >> 4, step s, lane (r & 15) + 16 g       (pack_filters_q's layout)
//   slab unit of digit j:   chunk 4 p + g, column nl + t (<= 146), plane j               (the staging's layout)
// both with zero bytes for bins >= 121.  A lane takes pairs lane, lane + 64 and, below lane 32, lane + 128; all its loads
// are issued before the first product.  v_dot4c_i32_i8 products of weight 2^(8 (i + j)) share an int32 sum as in the
// matrix loop (a lane's |sum| <= 3 * 3 * 16 * 128 * 128 < 2^22), D = sum_c acc_c 2^(8c) in int64, summed over the wave.
__device__ __forceinline__ long long q_value_from_digits(const v4i *__restrict__ fq_image, const unsigned char *slab, int r, int nl, int lane)
{
    constexpr int kPairs = 4 * kQSteps; // 160
    v4i fa[3][3], sb[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int pair = min(lane + 64 * k, kPairs - 1); // (k = 2 from lane 32 on: a valid address, the units zeroed below)
        const int s = pair >> 2, g = pair & 3;
        const v4i *fu = fq_image + ((size_t)(r >> 4) * kQSteps + s) * (kQStepBytes / 16) + (r & 15) + 16 * g;
        const v4i *su = reinterpret_cast<const v4i *>(slab + (size_t)((4 * (s & 1) + g) * kQPitch + nl + (s >> 1)) * kQUnit);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            fa[k][d] = fu[d * 64];
            sb[k][d] = su[d];
        }
    }
    if (lane + 128 >= kPairs) sb[2][0] = sb[2][1] = sb[2][2] = v4i{0, 0, 0, 0};
    int acc[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int w = 0; w < 4; ++w) acc[i + j] = __builtin_amdgcn_sdot4(fa[k][i][w], sb[k][j][w], acc[i + j], false);
    long long v = acc[4];
#pragma unroll
    for (int cls = 3; cls >= 0; --cls) v = v * 256 + acc[cls];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// ---- the parts of a tile, in the order hashprint_q_tile runs them.  tid, lane, wave, kg and cl are the tile's, handed
// down: kg = lane >> 4, this lane's group of 16 k' inside a step, cl = lane & 15, its column (B) / filter (A) in a tile ----

// The wave's filter digits of steps 0 and 1 of the image at img (this lane's unit of step 0) into the first two of the
// matrix loop's three register sets
__device__ __forceinline__ void q_load_first_steps(const v4i *img, v4i (&a)[3][3])
{
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        a[0][d] = img[d * 64];
        a[1][d] = img[(kQStepBytes / 16) + d * 64];
    }
}

// Staging by chains: the digits of Du of the tile at column n0 of the clip at S [121][c] into the slab.  FROM_T: S holds dB
// terms t and the spectrogram is max(t - ref, -80) (convert.h:12-15), the reference level riding on the loads.  NP = 6:
// returns whether this thread stored a non-zero digit (the six-product kernel's shortcut for silence); else 0.
//
// A task's half unit = 8 bins of one column of Du, three digit planes of 8 bytes.  EVERY load is issued, from a valid 32-bit
// clip-relative index (S[0], S[kLag] exist), and what lies outside the valid part is zeroed afterwards: written as
// `ok ? S[..] : 0` the loads sat in branches of their own, and the compiler, short of registers for so many merged values,
// waited for all but one of the loads in flight after every fourth -- memory round trips in a row, and the staging took
// as long as the matrix loop (tools/q_stamps.py: 69 k of a workgroup's 147 k cycles).  The loads of task i + kQAhead are
// issued before task i is quantised: a wave waits for memory once, at its first task, and the accumulators' registers,
// dead until the barrier, hold the values in flight
template <bool FROM_T, int NP>
__device__ __forceinline__ unsigned q_stage_slab(unsigned char *slab, const float *S, const float ref, const int n0, const int c, const int tid)
{
    unsigned any_digit = 0;
    float x[kQTasks][3][8];
    auto issue = [&](int i) {
        const int task = tid + i * kQThreads, qh = task / kLag, r = task - qh * kLag;
        const int gc = n0 + r;
        const bool in0 = gc + kLag < c, in1 = r < kQHeavy && gc + 2 * kLag < c;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int bin = 8 * qh + e;
            const unsigned at = (unsigned)(bin * c + gc); // (< 121 * c where it is used)
            const unsigned i0 = in0 && bin < kBins ? at : 0u, i2 = in1 && bin < kBins ? at + 2 * kLag : 0u;
            x[i][0][e] = S[i0];
            x[i][1][e] = S[i0 + kLag];
            x[i][2][e] = S[i2];
        }
    };
    auto quantise = [&](int i) {
        const int task = tid + i * kQThreads, qh = task / kLag, r = task - qh * kLag;
        const int gc = n0 + r;
        const bool in0 = gc + kLag < c, in1 = r < kQHeavy && gc + 2 * kLag < c;
        unsigned wa[8], wb[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const bool okb = 8 * qh + e < kBins;
            float x0 = x[i][0][e], x1 = x[i][1][e], x2 = x[i][2][e];
            if (FROM_T) {
                x0 -= ref;
                x1 -= ref;
                x2 -= ref;
            }
            const int u0 = q_fixed(x0), u1 = q_fixed(x1), u2 = q_fixed(x2);
            wa[e] = q_digit_bytes(in0 && okb ? u0 - u1 : 0);
            wb[e] = q_digit_bytes(in1 && okb ? u1 - u2 : 0);
        }
        // the half unit's place: chunk qh >> 1, bytes 8 (qh & 1) .. + 7 of each plane
        unsigned char *dst = slab + (size_t)((qh >> 1) * kQPitch + r) * kQUnit + 8 * (qh & 1);
        auto store = [&](const unsigned (&w)[8], unsigned char *to) {
            unsigned lo[3], hi[3];
            q_planes({w[0], w[1], w[2], w[3]}, lo);
            q_planes({w[4], w[5], w[6], w[7]}, hi);
#pragma unroll
            for (int j = 0; j < 3; ++j) *reinterpret_cast<v2i *>(to + 16 * j) = v2i{(int)lo[j], (int)hi[j]};
            if (NP == 6) any_digit |= lo[0] | lo[1] | lo[2] | hi[0] | hi[1] | hi[2];
        };
        // column r + 80 of a chain without a second slab column (r >= 67) is one of the pitch's 13 spare columns 147 .. 159,
        // which nothing reads: its zero digits are stored there without a branch (inside one, the compiler moved the
        // third column's loads into it too, with a wait for everything in flight)
        static_assert(kLag + kLag <= kQPitch, "spare columns for the chains' unconditional second store");
        store(wa, dst);
        store(wb, dst + (size_t)kLag * kQUnit);
    };
#pragma unroll
    for (int i = 0; i < kQAhead && i < kQTasks; ++i) issue(i);
#pragma unroll
    for (int i = 0; i < kQTasks; ++i) {
        if (i + kQAhead < kQTasks) issue(i + kQAhead);
        __builtin_amdgcn_sched_barrier(0); // (the loads stay above the quantisation they are to hide under)
        quantise(i);
    }
    return any_digit;
}

// The matrix loop: this wave's 16 filters of the image at img (steps 0 and 1 in a[0], a[1]) times the slab's columns, the
// digit products of equal weight summed in acc[tile of 16 hashprints][weight].  NP = 9: all nine digit products; NP = 6: the
// six of weight >= 2^16, accumulators 2 .. 4.  n_tiles: the tiles that hold hashprints; the products of the others are skipped
template <int NP>
__device__ __forceinline__ void q_matrix_loop(const v4i *img, v4i (&a)[3][3], const unsigned char *slab, const int kg, const int cl, const int n_tiles, v4i (&acc)[8][5])
{
    // B operand of (step, tile f): chunk 4 (s & 1) + kg, column 16 f + cl + (s >> 1)
    const unsigned char *bl = slab + (size_t)(kg * kQPitch + cl) * kQUnit;
#pragma unroll
    for (int f = 0; f < 8; ++f)
#pragma unroll
        for (int cls = 0; cls < 5; ++cls) acc[f][cls] = v4i{0, 0, 0, 0};
    auto step = [&](int s, const v4i (&aw)[3]) {
        const unsigned char *bs = bl + (size_t)((4 * (s & 1)) * kQPitch + (s >> 1)) * kQUnit;
        // the operand reads of tile f + 1 are issued BEFORE the nine products of tile f: read right where they are used, a
        // wave alone on its SIMD left the matrix pipe idle for an LDS round trip per tile (tools/q_stamps.py: 46 k cycles of
        // matrix instructions in a 69 k cycle loop)
        v4i nb0, nb1, nb2;
        {
            const v4i *bu = reinterpret_cast<const v4i *>(bs);
            nb0 = bu[0], nb1 = bu[1], nb2 = bu[2];
        }
#pragma unroll
        for (int f = 0; f < 8; ++f) {
            if (f < n_tiles) {
                const v4i b0 = nb0, b1 = nb1, b2 = nb2;
                if (f + 1 < 8) { // (tile f + 1 of the slab exists whether or not it holds hashprints)
                    const v4i *bu = reinterpret_cast<const v4i *>(bs + (size_t)(16 * (f + 1)) * kQUnit);
                    nb0 = bu[0], nb1 = bu[1], nb2 = bu[2];
                }
                __builtin_amdgcn_sched_barrier(0); // (the scheduler would sink the reads back to where they are used)
                // filter digit i times spectrogram digit j goes to accumulator i + j
                if (NP == 9) {
                    acc[f][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aw[0], b0, acc[f][0], 0, 0, 0);
                    acc[f][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aw[0], b1, acc[f][1], 0, 0, 0);
                }
                acc[f][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aw[0], b2, acc[f][2], 0, 0, 0);
                acc[f][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aw[1], b2, acc[f][3], 0, 0, 0);
                acc[f][4] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aw[2], b2, acc[f][4], 0, 0, 0);
                if (NP == 9) acc[f][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aw[1], b0, acc[f][1], 0, 0, 0);
                acc[f][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aw[1], b1, acc[f][2], 0, 0, 0);
                acc[f][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aw[2], b1, acc[f][3], 0, 0, 0);
                acc[f][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aw[2], b0, acc[f][2], 0, 0, 0);
            }
        }
    };
    // three register sets in turn: the loads of step s + 2 are issued before the products of step s
    auto load_a = [&](int s, v4i (&aw)[3]) {
        if (s < kQSteps) {
#pragma unroll
            for (int d = 0; d < 3; ++d) aw[d] = img[(size_t)s * (kQStepBytes / 16) + d * 64];
        }
    };
    if (n_tiles > 0) {
#pragma unroll 1
        for (int s = 0; s < kQSteps - 1; s += 3) { // 40 steps = 13 x 3 + 1
            load_a(s + 2, a[2]);
            step(s, a[0]);
            load_a(s + 3, a[0]);
            step(s + 1, a[1]);
            load_a(s + 4, a[1]);
            step(s + 2, a[2]);
        }
        step(kQSteps - 1, a[0]);
    }
}

// The epilogue (S10q): D = sum_c acc_c 2^(8c), its sign bits to parts [hashprint][wave].  D layout of the 16x16 tile:
// column (hashprint) = lane & 15, row (filter) = 4 (lane >> 4) + reg.  DBG: dbg may be given, D [clip][64][nhp] (tests; the unshifted nine-product kernel).
// A flag of its own: with a pointer that is known to be NULL only once everything is inlined, the shifted kernels took two
// registers more and the six-product kernels four (profiles/q_kernel_single_path.md).
//
// NP = 6: with fq = a0 + 2^8 a1 + 2^16 a2 and Du = b0 + 2^8 b1 + 2^16 b2, D = 2^16 Dp + Dl where
//   Dp = sum (a0 b2 + a1 b1 + a2 b0) + 2^8 sum (a1 b2 + a2 b1) + 2^16 sum a2 b2      (accumulators 2, 3, 4)
//   Dl = sum a0 b0 + 2^8 sum (a0 b1 + a1 b0)                                          (accumulators 0, 1)
// and every |b| <= 128, so |Dl| <= 128 S0_r + 2^8 128 (S0_r + S1_r) = Lmax_r with S0_r, S1_r the sums of |a0| and |a1| over
// row r's 2420 taps.  Where 2^16 |Dp| > Lmax_r the sign of D is the sign of Dp (and D != 0); a row with Lmax_r = 0 has
// D = 2^16 Dp exactly.  Else the value is OPEN: the bit from Dp >= 0 stands for the moment, and the value is counted in
// *n_open and, up to kQCap of them, listed as (r << 7 | n - n0) for q_settle_open.  thr[r] = floor(Lmax_r / 2^16), or -1
// for Lmax_r = 0: open iff |Dp| <= thr[r] (pack_filters_q)
template <int NP, bool DBG>
__device__ __forceinline__ void q_epilogue(const v4i (&acc)[8][5], const int clip, const int n0, const int nhp, const int n_tiles,
                                           unsigned short *parts, const int *thr, unsigned *n_open, unsigned short *list,
                                           long long *dbg, const int wave, const int kg, const int cl)
{
    v4i th = v4i{-1, -1, -1, -1};
    if (NP == 6) th = *reinterpret_cast<const v4i *>(thr + 16 * wave + 4 * kg);
#pragma unroll
    for (int f = 0; f < 8; ++f) {
        const int n = n0 + 16 * f + cl;
        (void)n;
        unsigned bits = 0; // this wave's 16 filters of hashprint n, filter 16 wave + row at bit 15 - row
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = 4 * kg + reg;
            long long v = acc[f][4][reg];
#pragma unroll
            for (int cls = 3; cls >= (NP == 9 ? 0 : 2); --cls) v = v * 256 + acc[f][cls][reg]; // (NP = 6: Dp)
            bits |= (unsigned)(v >= 0) << (15 - row);
            if (NP == 6 && f < n_tiles && n < nhp && (v < 0 ? -v : v) <= (long long)th[reg]) {
                const unsigned pos = atomicAdd(n_open, 1u);
                if (pos < (unsigned)kQCap) list[pos] = (unsigned short)(((16 * wave + row) << 7) | (16 * f + cl));
            }
#if !defined(HPFW_Q_STAMPS)
            if (DBG && dbg && f < n_tiles && n < nhp) dbg[((int64_t)clip * kFilters + 16 * wave + row) * nhp + n] = v;
#endif
        }
        // the four lanes of a column hold four filters each
        bits |= (unsigned)__shfl_xor((int)bits, 16);
        bits |= (unsigned)__shfl_xor((int)bits, 32);
        if (kg == 0) parts[(16 * f + cl) * 4 + wave] = (unsigned short)bits;
    }
}

// Settling the cnt listed open values, behind the barrier that ends the epilogue: every wave takes each fourth entry,
// forms D from the digits of the filter image and of the slab (q_value_from_digits) and flips the bit in `parts` where
// D >= 0 disagrees with it
__device__ __forceinline__ void q_settle_open(const v4i *fq_image, const unsigned char *slab, unsigned short *parts,
                                              const unsigned short *list, const unsigned cnt, const int wave, const int lane)
{
    for (unsigned e = (unsigned)__builtin_amdgcn_readfirstlane(wave); e < cnt; e += kQThreads / 64) {
        const int entry = __builtin_amdgcn_readfirstlane((int)list[e]);
        const int r = entry >> 7, nl = entry & 127;
        const long long d = q_value_from_digits(fq_image, slab, r, nl, lane);
        if (lane == 0) { // parts[nl * 4 + (r >> 4)], filter r at bit 15 - (r & 15) of it: two waves can meet in one word
            unsigned *w = reinterpret_cast<unsigned *>(parts) + nl * 2 + (r >> 5);
            const unsigned bit = 1u << (16 * ((r >> 4) & 1) + 15 - (r & 15));
            if (((*static_cast<volatile unsigned *>(w) & bit) != 0) != (d >= 0)) atomicXor(w, bit);
        }
    }
}

// The pack: the four waves' parts of the tile's hashprints n0 .. to hp[first + n0 ..] (first: where the clip's row of
// this image begins), one 64-bit word each
__device__ __forceinline__ void q_pack(const unsigned short *parts, uint64_t *hp, const int64_t first, const int n0, const int nhp, const int tid)
{
    if (tid < kQTileN && n0 + tid < nhp) {
        const unsigned short *p = parts + tid * 4;
        hp[first + n0 + tid] = ((uint64_t)p[0] << 48) | ((uint64_t)p[1] << 32) | ((uint64_t)p[2] << 16) | (uint64_t)p[3];
    }
}

// One tile t = clip * n_tiles_x + tile of 128 hashprints: stage the slab, then per filter image the matrix loop, the
// epilogue and the pack.  FROM_T: sdb holds the dB terms t written by the chirp-z kernel and tmax the clips' reference
// levels (q_stage_slab).  fq_images: filter digit images one after the other, the slab staged once and each image in turn
// running over it, hp [clip][image][nhp]: SHIFTED = false, the extraction's one image; SHIFTED = true, n_images shifted
// ones (shift_filter_images_kernel).  dbg (tests only, NULL in extraction; SHIFTED = false): D as
// int64 [clip][64][nhp].
//
// NP = 9: the nine digit products, D exactly.  NP = 6 (hashprint_q6_kernel: the unshifted image, no dbg): the six products
// of weight >= 2^16, and the workgroup settles the values whose sign those leave open itself, before it packs
// (q_epilogue, q_settle_open).  A workgroup with more than kQCap open values (near-stationary input) runs the nine-product
// matrix loop and epilogue over its slab instead, the six-product accumulators dead by then.  hp is written once and
// final.  counts[t] = the tile's number of open values, or kQRedo above kQCap.  A slab of zero digits (silence, the -80 dB
// floor) has D = 0 everywhere: all bits one, count 0, and no product is formed.
template <bool FROM_T, bool SHIFTED, int NP>
__device__ __forceinline__ void hashprint_q_tile(const unsigned t, const v4i *__restrict__ fq_images, const float *__restrict__ sdb,
                                                 const float *__restrict__ tmax, int c, int nhp, int n_tiles_x, uint64_t *__restrict__ hp,
                                                 long long *__restrict__ dbg, int n_images, const int *__restrict__ thr,
                                                 unsigned *__restrict__ counts)
{
    unsigned char *slab = smem_raw;                                   // [chunk][column (pitch 160)][digit][16]
    unsigned short *parts = reinterpret_cast<unsigned short *>(smem_raw + kQSlabBytes); // [hashprint][wave]
    unsigned *n_open = reinterpret_cast<unsigned *>(smem_raw + kQLdsBytes);             // (NP = 6)
    unsigned short *list = reinterpret_cast<unsigned short *>(smem_raw + kQListAt);     // (NP = 6) kQCap entries
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kg = lane >> 4, cl = lane & 15;  // this lane's group of 16 k' inside a step; its column (B) / filter (A) in a tile
    const int clip = t / n_tiles_x;
    const int n0 = (t - clip * n_tiles_x) * kQTileN;
    if (NP == 6 && tid == 0) *n_open = 0; // (before the prologue barrier)
#if defined(HPFW_Q_STAMPS)
    // diagnosis build (tools/q_stamps.py): s_memtime of wave 0 at the phase boundaries, written to dbg [workgroup][8]
    long long st[6];
    st[0] = __builtin_amdgcn_s_memtime();
#define Q_STAMP(k) st[k] = __builtin_amdgcn_s_memtime()
#else
#define Q_STAMP(k) ((void)0)
#endif
    const float *S = sdb + (int64_t)clip * kBins * c;
    const float ref = FROM_T ? tmax[clip] : 0.0f;
    // the wave's filter digits of the first two steps are on their way while the slab is quantised
    const v4i *img = fq_images + (size_t)wave * kQSteps * (kQStepBytes / 16) + lane;
    v4i a[3][3];
    q_load_first_steps(img, a);
    const unsigned any_digit = q_stage_slab<FROM_T, NP>(slab, S, ref, n0, c, tid);
    Q_STAMP(1);
    // the only barrier before the epilogue: the slab is read-only from here on
    if (NP == 6) {
        if (!__syncthreads_or((int)(any_digit != 0))) { // Du = 0 in the whole slab: D = 0, every bit one, nothing open
            if (tid < kQTileN && n0 + tid < nhp) hp[(int64_t)clip * nhp + n0 + tid] = ~0ull;
            if (tid == 0) counts[t] = 0;
            return;
        }
    } else {
        __syncthreads();
    }
    Q_STAMP(2);
    // tiles of 16 hashprints that hold any (the last workgroup of a clip)
    const int n_tiles = min(8, (nhp - n0 + 15) / 16);
    // one trip per image over the same slab, the first two steps' digits of image im in a[0] and a[1].  The extraction's
    // instance is compiled without a loop (the condition folds to false before any optimisation): with a loop, even of
    // one trip known at compile time, the compiler allocated its registers differently (16 more waits for memory in
    // <true, false>, 44 in <false, false>), and a run-time image count with dbg live across the loop spilled
    int im = 0;
#pragma unroll 1
    do {
        if (SHIFTED && im > 0) {
            __syncthreads(); // (parts is written again by this image's epilogue)
            img += (size_t)4 * kQSteps * kQStepBytes / 16;
            q_load_first_steps(img, a);
        }
        v4i acc[8][5];
        q_matrix_loop<NP>(img, a, slab, kg, cl, n_tiles, acc);
        Q_STAMP(3);
        q_epilogue<NP, NP == 9 && !SHIFTED>(acc, clip, n0, nhp, n_tiles, parts, thr, n_open, list, dbg, wave, kg, cl);
        Q_STAMP(4);
        __syncthreads();
        if (NP == 6) {
            const unsigned cnt = *n_open; // (the same for the whole workgroup; nothing adds to it behind the barrier)
            if (cnt > (unsigned)kQCap) { // the redo: nine products over the slab as it stands
                if (tid == 0) counts[t] = kQRedo;
                q_load_first_steps(img, a);
                q_matrix_loop<9>(img, a, slab, kg, cl, n_tiles, acc);
                q_epilogue<9, false>(acc, clip, n0, nhp, n_tiles, parts, nullptr, nullptr, nullptr, nullptr, wave, kg, cl);
                __syncthreads();
                q_pack(parts, hp, (int64_t)clip * nhp, n0, nhp, tid);
                return;
            }
            if (cnt > 0) {
                q_settle_open(fq_images, slab, parts, list, cnt, wave, lane);
                __syncthreads();
            }
        }
        q_pack(parts, hp, ((int64_t)clip * (SHIFTED ? n_images : 1) + im) * nhp, n0, nhp, tid);
        if (NP == 6 && tid == 0) counts[t] = *n_open <= (unsigned)kQCap ? *n_open : kQRedo;
    } while (SHIFTED && ++im < n_images);
#if defined(HPFW_Q_STAMPS)
    Q_STAMP(5);
    long long *stamps = dbg ? dbg : g_q_stamps_dev;
    if (stamps && tid == 0) {
        for (int k = 0; k < 6; ++k) stamps[(int64_t)t * 8 + k] = st[k];
        stamps[(int64_t)t * 8 + 6] = __builtin_amdgcn_s_getreg((15 << 11) | 4); // HW_ID: wave, SIMD, CU, SH, SE
        stamps[(int64_t)t * 8 + 7] = blockIdx.x;
    }
#endif
}

// Workgroups go to the eight XCDs in turn (id mod 8), each with an L2 of its own: an XCD takes a contiguous run of
// (clip, tile) pairs with the tile fastest, so that the 99 columns two neighbouring tiles share, and the columns a
// tile reads twice (as c and as c + 80), come from HBM once: 2.34 -> 1.19 MB per clip by the counters (1.17 algorithmic; profiles/r04_pmc.json)
//
// Short tiles last: where a clip's last tile holds fewer than eight tiles of 16 hashprints (n_hp = 2320: one of eight) its
// workgroup stages a whole slab for a fraction of the matrix work, and a workgroup that starts in the launch's last
// generation runs its whole life on a nearly empty chip.  The full tiles then come first, in the order above, and the
// clips' short tiles after them, each XCD again with a contiguous run: the launch ends on short workgroups.  The
// logical tile t = clip * n_tiles_x + tile (counts, hp, dbg) does not change.
constexpr unsigned kQNoTile = 0xffffffffu;
__host__ __device__ inline bool q_short_last(int nhp, int n_tiles_x) { return nhp - (n_tiles_x - 1) * kQTileN <= kQTileN - 16; }
__host__ __device__ inline unsigned q_round8(unsigned n) { return 8 * ((n + 7) / 8); }

static unsigned q_grid(int nhp, int n_tiles_x, int n_clips)
{
    if (!q_short_last(nhp, n_tiles_x)) return q_round8((unsigned)n_tiles_x * (unsigned)n_clips);
    return q_round8((unsigned)(n_tiles_x - 1) * (unsigned)n_clips) + q_round8((unsigned)n_clips);
}

__device__ __forceinline__ unsigned q_tile_of_workgroup(int nhp, int n_tiles_x, int n_clips)
{
    unsigned b = blockIdx.x;
    if (!q_short_last(nhp, n_tiles_x)) {
        const unsigned t = (b & 7) * (gridDim.x / 8) + (b >> 3);
        return t < (unsigned)(n_tiles_x * n_clips) ? t : kQNoTile;
    }
    const unsigned full_x = (unsigned)(n_tiles_x - 1), n_full = full_x * (unsigned)n_clips, grid_full = q_round8(n_full);
    if (b < grid_full) {
        const unsigned j = (b & 7) * (grid_full / 8) + (b >> 3);
        if (j >= n_full) return kQNoTile;
        const unsigned clip = j / full_x;
        return clip * (unsigned)n_tiles_x + (j - clip * full_x);
    }
    b -= grid_full; // (a multiple of 8: the XCD is b & 7 as before)
    const unsigned j = (b & 7) * ((gridDim.x - grid_full) / 8) + (b >> 3);
    return j < (unsigned)n_clips ? j * (unsigned)n_tiles_x + full_x : kQNoTile;
}

template <bool FROM_T, bool SHIFTED>
__global__ __launch_bounds__(kQThreads, 2) void hashprint_q_kernel(const v4i *__restrict__ fq_images, const float *__restrict__ sdb,
                                                                   const float *__restrict__ tmax, int c, int nhp, int n_tiles_x, int n_clips,
                                                                   uint64_t *__restrict__ hp, long long *__restrict__ dbg, int n_images)
{
    const unsigned t = q_tile_of_workgroup(nhp, n_tiles_x, n_clips);
    if (t == kQNoTile) return;
    hashprint_q_tile<FROM_T, SHIFTED, 9>(t, fq_images, sdb, tmax, c, nhp, n_tiles_x, hp, dbg, n_images, nullptr, nullptr);
}

// the six-product instantiation of the extraction's kernel (hashprint_q_tile, NP = 6): bits from Dp, the open values
// settled from the slab before the hashprints are stored
template <bool FROM_T>
__global__ __launch_bounds__(kQThreads, 2) void hashprint_q6_kernel(const v4i *__restrict__ fq_image, const float *__restrict__ sdb,
                                                                    const float *__restrict__ tmax, int c, int nhp, int n_tiles_x, int n_clips,
                                                                    uint64_t *__restrict__ hp, const int *__restrict__ thr,
                                                                    unsigned *__restrict__ counts)
{
    const unsigned t = q_tile_of_workgroup(nhp, n_tiles_x, n_clips);
    if (t == kQNoTile) return;
    hashprint_q_tile<FROM_T, false, 6>(t, fq_image, sdb, tmax, c, nhp, n_tiles_x, hp, nullptr, 1, thr, counts);
}

// Image i (blockIdx.y) of the filters moved by shifts.s[i] bins: the byte of bin b holds the digit of fq[r][20 (b - s) + t]
// taken from the unshifted image (so the row scale is the unshifted filter's), zero where b - s is not a bin.  One
// thread per 16-byte unit [wave][step][digit][lane] of the image.
__global__ __launch_bounds__(256) void shift_filter_images_kernel(const unsigned char *__restrict__ base, ShiftList shifts,
                                                                  v4i *__restrict__ out)
{
    constexpr int kUnits = 4 * kQSteps * kQStepBytes / 16;
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= kUnits) return;
    const int s = shifts.s[blockIdx.y];
    const int l = u & 63, i = (u >> 6) % 3, ws = u / 192;
    const int step = ws % kQSteps, w = ws / kQSteps, t = step >> 1, p = step & 1;
    unsigned wd[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int b = 64 * p + 16 * (l >> 4) + e, src = b - s;
        if (b < kBins && src >= 0 && src < kBins) {
            const unsigned char v = base[((size_t)w * kQSteps + 2 * t + (src >> 6)) * kQStepBytes + ((size_t)i * 64 + (l & 15) + 16 * ((src >> 4) & 3)) * 16 +
                                         (src & 15)];
            wd[e >> 2] |= (unsigned)v << (8 * (e & 3));
        }
    }
    out[(size_t)blockIdx.y * kUnits + u] = v4i{(int)wd[0], (int)wd[1], (int)wd[2], (int)wd[3]};
}

// host: the filters' digits as the A operand of v_mfma_i32_16x16x64_i8, [wave][step s = 2 t + p][digit][lane][16 bytes]:
// byte e of lane l = digit of fq[row = 16 wave + (l & 15)][k = 20 bin + t], bin = 64 p + 16 (l >> 4) + e (zero for bin >= 121)
// thr, when given: the 64 thresholds of the six-product split: floor(Lmax_r / 2^16) with Lmax_r = 128 (S0_r + 256 (S0_r +
// S1_r)), S0_r and S1_r the sums of |digit 0| and |digit 1| of row r's taps, or -1 where Lmax_r = 0 (q_epilogue).
void pack_filters_q(const float *f, std::vector<int8_t> &image, std::vector<int32_t> *thr)
{
    std::vector<int32_t> fq((size_t)kFilters * kFrame);
    for (int r = 0; r < kFilters; ++r) {
        float m = 0.0f;
        for (int k = 0; k < kFrame; ++k) m = std::fmax(m, std::fabs(f[(size_t)k * kFilters + r]));
        const int e = m > 0.0f ? 21 - std::ilogb(m) : 0;
        for (int k = 0; k < kFrame; ++k) fq[(size_t)r * kFrame + k] = (int32_t)std::rint(std::ldexp(f[(size_t)k * kFilters + r], e));
    }
    if (thr) {
        thr->clear();
        for (int r = 0; r < kFilters; ++r) {
            int64_t s0 = 0, s1 = 0;
            for (int k = 0; k < kFrame; ++k) {
                const int u = fq[(size_t)r * kFrame + k];
                const int d0 = ((u + 128) & 255) - 128, u1 = (u - d0) >> 8, d1 = ((u1 + 128) & 255) - 128;
                s0 += std::abs(d0);
                s1 += std::abs(d1);
            }
            const int64_t lmax = 128 * (s0 + 256 * (s0 + s1)); // <= 128 * 128 * 2420 * 513 < 2^35
            thr->push_back(lmax > 0 ? (int32_t)(lmax >> 16) : -1);
        }
    }
    image.assign((size_t)4 * kQSteps * kQStepBytes, 0);
    for (int w = 0; w < 4; ++w)
        for (int t = 0; t < kCtx; ++t)
            for (int p = 0; p < 2; ++p)
                for (int l = 0; l < 64; ++l)
                    for (int e = 0; e < 16; ++e) {
                        const int bin = 64 * p + 16 * (l >> 4) + e;
                        if (bin >= kBins) continue;
                        const int u = fq[(size_t)(16 * w + (l & 15)) * kFrame + bin * kCtx + t];
                        const int d0 = ((u + 128) & 255) - 128, u1 = (u - d0) >> 8, d1 = ((u1 + 128) & 255) - 128, d2 = (u1 - d1) >> 8;
                        const int d[3] = {d0, d1, d2};
                        for (int i = 0; i < 3; ++i)
                            image[((size_t)w * kQSteps + (2 * t + p)) * kQStepBytes + ((size_t)i * 64 + l) * 16 + e] = (int8_t)d[i];
                    }
}

#if defined(HPFW_Q_STAMPS)
static long long *g_q_stamps = nullptr;
extern "C" void hpfw_gpu_debug_set_q_stamps(void *d)
{
    g_q_stamps = static_cast<long long *>(d);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_q_stamps_dev), &g_q_stamps, sizeof(g_q_stamps));
}
#endif

size_t project_q_image_bytes() { return (size_t)4 * kQSteps * kQStepBytes; }
size_t project_q_split_bytes(int64_t tiles) { return (size_t)tiles * 4; }
int64_t project_q_tiles(int64_t n_clips, int64_t c)
{
    const int64_t nhp = c - (kCtx - 1) - kLag;
    return nhp > 0 ? n_clips * ((nhp + kQTileN - 1) / kQTileN) : 0;
}

// dB terms (d_tmax != NULL) or dB spectrograms -> hashprints [n_clips][max(n_shifts, 1)][c - 99] of the filter images at
// d_images: the unshifted one (n_shifts = 0), or n_shifts from launch_shift_filter_images.  One shift runs the image loop
// too: 2.14 ms against 2.15 for the extraction's instance on 1000 x 30 s clips (profiles/transpose.json).  d_dbg: NULL,
// or D [n_clips][64][c - 99] of the unshifted image (tests)
// split (n_shifts = 0, no d_dbg; else NULL): the six-product kernel instead of the nine-product kernel.  d_thr: the device
// copy of pack_filters_q's thresholds; d_work: project_q_split_bytes(project_q_tiles(n_clips, c)) bytes, counts [tiles]
void launch_hashprints_q(const void *d_images, int n_shifts, const float *d_db, const float *d_tmax, int n_clips, int c, uint64_t *d_hp,
                         long long *d_dbg, hipStream_t s, const QSplit *split)
{
    static PerDeviceOnce attr_set;
    if (attr_set.need()) {
        for (const void *k : {reinterpret_cast<const void *>(hashprint_q_kernel<true, false>), reinterpret_cast<const void *>(hashprint_q_kernel<false, false>),
                              reinterpret_cast<const void *>(hashprint_q_kernel<true, true>), reinterpret_cast<const void *>(hashprint_q_kernel<false, true>)})
            (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kQLdsBytes);
        for (const void *k : {reinterpret_cast<const void *>(hashprint_q6_kernel<true>), reinterpret_cast<const void *>(hashprint_q6_kernel<false>)})
            (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kQLdsBytes6);
        attr_set.mark();
    }
    const int nhp = c - (kCtx - 1) - kLag;
    if (nhp <= 0 || n_clips <= 0 || n_shifts < 0) return;
#if defined(HPFW_Q_STAMPS)
    // (tools/q_stamps.py extract: the stamps of the extraction's own launches; its six-product kernel finds them by g_q_stamps_dev)
    if (!d_dbg && !(split && n_shifts == 0)) d_dbg = g_q_stamps;
#endif
    const int tiles = (nhp + kQTileN - 1) / kQTileN;
    const dim3 grid(q_grid(nhp, tiles, n_clips)); // one-dimensional, in XCD-aware order (q_tile_of_workgroup)
    if (split && n_shifts == 0 && !d_dbg) {
        auto k6 = d_tmax ? hashprint_q6_kernel<true> : hashprint_q6_kernel<false>;
        hipLaunchKernelGGL(k6, grid, dim3(kQThreads), kQLdsBytes6, s, static_cast<const v4i *>(d_images), d_db, d_tmax, c, nhp, tiles, n_clips, d_hp,
                           split->d_thr, static_cast<unsigned *>(split->d_work));
        return;
    }
    auto k = n_shifts > 0 ? (d_tmax ? hashprint_q_kernel<true, true> : hashprint_q_kernel<false, true>)
                          : (d_tmax ? hashprint_q_kernel<true, false> : hashprint_q_kernel<false, false>);
    hipLaunchKernelGGL(k, grid, dim3(kQThreads), kQLdsBytes, s, static_cast<const v4i *>(d_images), d_db, d_tmax, c, nhp, tiles, n_clips,
                       d_hp, d_dbg, n_shifts);
}

void launch_shift_filter_images(const void *d_fq_image, const ShiftList &shifts, void *d_images, hipStream_t s)
{
    constexpr int kUnits = 4 * kQSteps * kQStepBytes / 16;
    hipLaunchKernelGGL(shift_filter_images_kernel, dim3((kUnits + 255) / 256, shifts.n), dim3(256), 0, s,
                       static_cast<const unsigned char *>(d_fq_image), shifts, static_cast<v4i *>(d_images));
}

} // namespace hpfw
