// query_scan.h -- what the matrix-core scans of the plain, overlap and local searches (k_search_mfma.hip, k_search_overlap.hip,
// k_search_local.hip) share on the device, stated once: the geometry, the LDS layout, the
// staging of a clip's window, the walk of the queries' image and the reduction of a tile to one key per query row.  The
// product step is the joins' as well (k_selfjoin.hip, k_localjoin.hip).  The device code is inlined into its kernel; the two host
// helpers are the LDS byte count and the launchers' LDS attribute.
//
// GEOMETRY.  A workgroup = 8 waves = 32 queries (one group g of expand_queries_kernel's image) x kScanWgLags lags of one clip;
// lag d puts position j of a query on position d + j of the clip.  Wave w has the lags d0 + 128 w .. + 127 in kScanTiles
// tiles of 32: acc[t][reg] belongs to query row m = (reg & 3) + 8 (reg >> 2) + 4 h and lag d0 + 128 w + 32 t + n_lane
// (lane = n_lane + 32 h).  Operand B of position j for lag column n is the clip's hashprint d0 + n + j: a window of
// kScanWgLags + kt slots sliding through the LDS (kt: the group's longest query), fp4 zeros outside the clip; operand A of
// position j, the 32 queries' hashprint j (fp4 zeros past a query's end), is read once per position and used by the four
// tiles.  The image is walked in chunks of kScanChunk positions, double-buffered: the next chunk is fetched into registers
// while this one multiplies.  The kernel's step runs for the positions j < jn of every live wave; the loop has no per-lag or
// per-position condition.
#pragma once
#include "kernels.h"
#include "overlap_rule.h"
#include "search_plan.h" // kScanLdsLimit

namespace hpfw {

typedef int v8i __attribute__((ext_vector_type(8)));

constexpr int kScanThreads = 512;                                // 8 waves
constexpr int kScanTiles = 4;                                    // lag tiles of 32 per wave
constexpr int kScanWaveLags = 32 * kScanTiles;                   // 128
constexpr int kScanWgLags = kScanWaveLags * (kScanThreads / 64); // 1024 lags per workgroup (and chunk of a split)
constexpr int kScanChunk = 16;                                   // positions j per staged chunk of the A operand (16 KB)
static_assert(kScanWgLags == kOverlapChunk && kScanWgLags == kLocalChunk, "kernels.h states the chunks");
static_assert(kScanChunk * 64 == 2 * kScanThreads, "a chunk of A is two entries per thread");

// dynamic LDS for a group whose longest query has kt hashprints: ldsB [2][win], win = kScanWgLags + kt slots (one spare),
// plane h = bits [32 h, 32 h + 32) of each hashprint (lanes of a half-wave read 16 B apart: no bank conflicts); ldsA
// [2][kScanChunk][64]; len [32], the rows' lengths as the kernel counts them; red [8 waves][32 rows]
struct ScanLds {
    v4i *B, *A;
    int *len;
    unsigned *red;
};
__device__ __forceinline__ ScanLds scan_lds(unsigned char *smem, int win)
{
    ScanLds l;
    l.B = reinterpret_cast<v4i *>(smem);
    l.A = l.B + 2 * win;
    l.len = reinterpret_cast<int *>(l.A + 2 * kScanChunk * 64);
    l.red = reinterpret_cast<unsigned *>(l.len + 32);
    return l;
}
inline size_t query_scan_lds_bytes(int kt)
{
    return (size_t)2 * (kScanWgLags + kt) * 16 + (size_t)2 * kScanChunk * 64 * 16 + 32 * 4 + (kScanThreads / 64) * 32 * 4;
}

// once per device: the kernels may take dynamic LDS up to the scans' limit (search_plan.h's 160 KiB)
inline void scan_allow_lds(PerDeviceOnce &once, std::initializer_list<const void *> kernels)
{
    if (!once.need()) return;
    for (const void *f : kernels) (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kScanLdsLimit);
    once.mark();
}

// the clip's positions d0 .. d0 + win - 1 (the clip: n hashprints from db[r0] on), expanded; fp4 zeros before its start and
// past its end -- not the expansion of 0, which is all +1
__device__ __forceinline__ void scan_stage_window(v4i *ldsB, int win, const uint64_t *__restrict__ db, int64_t r0, int n, int d0, int tid)
{
    for (int i = tid; i < win; i += kScanThreads) {
        const int gi = d0 + i;
        v4i lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
        if (gi >= 0 && gi < n) {
            const uint64_t w = db[r0 + gi];
            lo = expand32((uint32_t)w);
            hi = expand32((uint32_t)(w >> 32));
        }
        ldsB[i] = lo;
        ldsB[win + i] = hi;
    }
}

// The walk of one group's image qa [kt_pad][64] over the staged window (the caller has stored it; the first barrier here
// covers it).  step(ap, bj, j) takes in position j of the chunk: this lane's operands are ap[j * 64] and bj[j + 32 t] for lag
// tile t; the accumulators are the caller's registers.  bp: ldsB + h win + 128 wave + n_lane.  A wave that is not live
// multiplies nothing and only helps staging.  A barrier follows the last step.
template <class Step>
__device__ __forceinline__ void scan_walk(const v4i *__restrict__ qa, v4i *ldsA, const v4i *bp, int kt, bool live, int tid, int lane,
                                          Step step)
{
    const int n_chunks = (kt + kScanChunk - 1) / kScanChunk;
    v4i st0 = qa[tid], st1 = qa[tid + kScanThreads]; // 16 positions x 64 lanes = 1024 entries: two per thread
    ldsA[tid] = st0;
    ldsA[tid + kScanThreads] = st1;
    __syncthreads();
    for (int c = 0; c < n_chunks; ++c) {
        const bool more = c + 1 < n_chunks;
        if (more) { // next chunk of A into registers while this one multiplies
            st0 = qa[(c + 1) * (kScanChunk * 64) + tid];
            st1 = qa[(c + 1) * (kScanChunk * 64) + tid + kScanThreads];
        }
        const v4i *ap = ldsA + (c & 1) * (kScanChunk * 64) + lane;
        const v4i *bj = bp + c * kScanChunk;
        // kt is the workgroup's, so the count is a scalar; said outright (join_scan.h: left to itself the compiler counts
        // the positions in a vector register once the step is a callable)
        const int jn = __builtin_amdgcn_readfirstlane(min(kScanChunk, kt - c * kScanChunk));
        for (int j = 0; live && j < jn; ++j) step(ap, bj, j);
        if (more) {
            v4i *dst = ldsA + ((c + 1) & 1) * (kScanChunk * 64);
            dst[tid] = st0;
            dst[tid + kScanThreads] = st1;
        }
        __syncthreads();
    }
}

// one position's products: A operand ap[j * 64] against the TILES B operands bj[j + 32 t], both fp4 with unit scales
template <int TILES>
__device__ __forceinline__ void scan_products(f32x16 (&acc)[TILES], const v4i *ap, const v4i *bj, int j)
{
    const int one = 0x7f7f7f7f; // E8M0 scale 2^0
    const v4i a4 = ap[j * 64];
    const v8i av = {a4.x, a4.y, a4.z, a4.w, 0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
        const v4i b4 = bj[j + 32 * t];
        const v8i bv = {b4.x, b4.y, b4.z, b4.w, 0, 0, 0, 0};
        acc[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc[t], 4, 4, 0, one, 0, one);
    }
}

// The smallest key of every query row over the workgroup's lags: key(reg, t) is the candidate of accumulator register reg of
// tile t, kScanNoKey for none.  The minimum over the tiles, then over the 32 lag columns of the half-wave, then over the
// waves through red; thread m < 32 receives row m's (the other threads nothing of use).  Holds a barrier.
constexpr unsigned kScanNoKey = 0xffffffffu;
template <class Key>
__device__ __forceinline__ unsigned scan_row_min(unsigned *red, int tid, int wave, int n_lane, int h, Key key)
{
    unsigned *wave_red = red + wave * 32;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        unsigned best = kScanNoKey;
#pragma unroll
        for (int t = 0; t < kScanTiles; ++t) {
            const unsigned cand = key(reg, t);
            best = cand < best ? cand : best;
        }
#pragma unroll
        for (int s = 16; s >= 1; s >>= 1) {
            const unsigned o = (unsigned)__shfl_xor((int)best, s);
            best = o < best ? o : best;
        }
        if (n_lane == 0) wave_red[(reg & 3) + 8 * (reg >> 2) + 4 * h] = best;
    }
    __syncthreads();
    unsigned best = kScanNoKey;
    if (tid < 32) {
        best = red[tid];
        for (int w = 1; w < kScanThreads / 64; ++w) best = red[w * 32 + tid] < best ? red[w * 32 + tid] : best;
    }
    return best;
}

} // namespace hpfw
