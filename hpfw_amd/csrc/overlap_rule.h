// overlap_rule.h -- the overlap rule on the device, stated once for the overlap search
// (k_search_overlap.hip), the catalogue self-join and the ingest join (k_selfjoin.hip, sections 22 and 23) and the scored
// overlap search's reader of their table (k_stats.hip).  Device code only; everything here is inlined into its kernel.
//
// Lag d puts position j of the query (the joins: of clip a) on position d + j of the clip (of clip b).  Over the
// L(d) = min(k, n - d) - max(0, -d) positions both have, dist(d) = sum popcount(q[j] ^ r[d + j]).
//   - a lag with L >= min_overlap is a candidate;
//   - candidates are ordered by dist / L as an exact rational, cross-multiplied in 64 bits;
//   - then by larger L;
//   - then by smaller lag.
// No floating point takes part in the order.
//
// A pair's lags are scanned in chunks of kChunk = 1024, dealt round robin to `splits` workgroups.  Inside a chunk a candidate
// is two words: dist, and w = (kLMax - L) << 10 | lag inside the chunk -- at equal rates the smaller w has the larger L, then
// the smaller lag; "none" is (kNoDist, kNoW), a rate above every rate with L = 1.  A workgroup keeps the best of its chunks
// in a Best and leaves it as one 16-byte table entry {dist, L, lag, 0} per (row, clip, split); the table is preset to 0xff
// in every byte, so an entry nobody wrote reads dist = kOverlapNoEntry.  fold() joins the entries of a pair's splits.
//
// OverlapRule<LMAX, NODIST, MUL24>: L <= LMAX, dist < NODIST, and MUL24 says that both fit 24 bits, so that a product is
// one 24-bit multiply pair instead of a full 32 x 32 one.  kernels.h names the two instantiations:
//   OverlapSearchRule = <16383, 2^21, true>             queries of at most 16000 hashprints   k_search_overlap.hip
//   JoinRule          = <kSelfjoinMaxLen, 2^25, false>  recordings of at most 2^18 - 1        k_selfjoin.hip
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace hpfw {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// 8 bits -> 8 E2M1 nibbles, bit i in nibble i: 0 -> +1.0 (0x2), 1 -> -1.0 (0xA)
__device__ __forceinline__ uint32_t expand8(uint32_t x)
{
    uint32_t t = (x | (x << 12)) & 0x000F000Fu;
    t = (t | (t << 6)) & 0x03030303u;
    t = (t | (t << 3)) & 0x11111111u;
    return 0x22222222u | (t << 3);
}

__device__ __forceinline__ v4i expand32(uint32_t w)
{
    v4i r;
    r.x = (int)expand8(w & 0xff);
    r.y = (int)expand8((w >> 8) & 0xff);
    r.z = (int)expand8((w >> 16) & 0xff);
    r.w = (int)expand8(w >> 24);
    return r;
}

// dist of a table entry that no workgroup wrote (every byte still 0xff): the (row, clip, split) has no candidate
constexpr unsigned kOverlapNoEntry = 0xffffffffu;
__device__ __forceinline__ bool overlap_no_entry(const uint4 &e) { return e.x == kOverlapNoEntry; }

template <unsigned LMAX, unsigned NODIST, bool MUL24>
struct OverlapRule {
    static_assert(!MUL24 || (NODIST < (1u << 24) && LMAX < (1u << 24)), "a 24-bit product needs operands below 2^24");
    static_assert(64ull * LMAX < (1ull << 24), "the fp32 accumulators hold 64 L - 2 dist exactly only below 2^24");
    static_assert(LMAX < (1u << 22), "w keeps kLMax - L above a 10-bit lag in 32 bits");

    static constexpr int kChunk = 1 << 10; // lags per chunk: a candidate's lag inside the chunk takes 10 bits of w
    static constexpr unsigned kLMax = LMAX, kNoDist = NODIST;
    static constexpr unsigned kNoW = ((LMAX - 1) << 10) | 0x3ffu;

    static __device__ __forceinline__ uint64_t mul(unsigned a, unsigned b)
    {
        if constexpr (MUL24)
            return (uint64_t)(a & 0xffffffu) * (uint64_t)(b & 0xffffffu);
        else
            return (uint64_t)a * (uint64_t)b;
    }

    // candidate (d1, w1) before (d2, w2): dist1 / L1 against dist2 / L2, then w
    static __device__ __forceinline__ bool less(unsigned d1, unsigned w1, unsigned d2, unsigned w2)
    {
        const uint64_t a = mul(d1, kLMax - (w2 >> 10)), b = mul(d2, kLMax - (w1 >> 10));
        return a < b || (a == b && w1 < w2);
    }

    // a workgroup's best of one row over the chunks it has done (in rising order of lag), in one thread per row
    struct Best {
        unsigned dist = kNoDist, L = 1;
        int lag = 0;
        // a candidate of a later chunk: a larger lag, so it wins on a smaller rate or, at the same rate, a larger L
        __device__ void offer(unsigned d, unsigned l, int g)
        {
            const uint64_t a = mul(d, L), b = mul(dist, l);
            if (a < b || (a == b && l > L)) {
                dist = d;
                L = l;
                lag = g;
            }
        }
        // the best (dist, w) of chunk d0, if it has one
        __device__ void offer_chunk(unsigned d, unsigned w, int d0)
        {
            if (d != kNoDist) offer(d, kLMax - (w >> 10), d0 + (int)(w & 0x3ffu));
        }
        __device__ void store(uint4 *e) const
        {
            if (dist != kNoDist) *e = make_uint4(dist, L, (unsigned)lag, 0u);
        }
    };

    // b, the fold of a pair's entries so far, takes in the entry e of another split (splits meet lags in no order)
    static __device__ __forceinline__ void fold(uint4 &b, const uint4 e)
    {
        if (overlap_no_entry(e)) return;
        const uint64_t x = mul(e.x, b.y), y = mul(b.x, e.y);
        if (overlap_no_entry(b) || x < y || (x == y && (e.y > b.y || (e.y == b.y && (int)e.z < (int)b.z)))) b = e;
    }

    // dist / L at or below rate_num / rate_den (the joins' threshold: dist rate_den <= 2^34, rate_num L < 2^34)
    static __device__ __forceinline__ bool reported(const uint4 &e, unsigned rate_num, unsigned rate_den)
    {
        return !overlap_no_entry(e) && mul(e.x, rate_den) <= mul(rate_num, e.y);
    }

    // The end of a chunk on the matrix cores, 8 waves of TILES lag tiles of 32: acc[t][reg] = 64 L - 2 dist of row
    // m = (reg & 3) + 8 (reg >> 2) + 4 h at lag d0 + wave 32 TILES + t 32 + n_lane (lane = n_lane + 32 h).  lens [32]: the
    // rows' lengths, 0 for a row without candidates; n: the clip's length.  The best of a half-wave's 32 lag columns, then
    // of the 8 waves through red [8][32], goes to the Best of thread m.  The caller has a barrier before (red may lie over an
    // operand) and one before red is written again.
    template <int TILES>
    static __device__ __forceinline__ void tile_epilogue(const f32x16 (&acc)[TILES], const int *lens, int n, int min_overlap, int d0,
                                                         uint2 *red, Best &best, int tid, int wave, int n_lane, int h)
    {
        static_assert(8 * 32 * TILES == kChunk, "8 waves cover a chunk");
        uint2 *wave_red = red + wave * 32; // formed once: from red[wave * 32 + m] the compiler keeps red + m, one more VGPR
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int m = (reg & 3) + 8 * (reg >> 2) + 4 * h;
            const int k = lens[m];
            unsigned bd = kNoDist, bw = kNoW;
#pragma unroll
            for (int t = 0; t < TILES; ++t) {
                const int lo = wave * (32 * TILES) + t * 32 + n_lane;
                const int d = d0 + lo;
                const int L = min(k, n - d) + min(0, d);
                const unsigned dist = (unsigned)((64 * L - (int)acc[t][reg]) >> 1);
                const unsigned w = ((kLMax - (unsigned)L) << 10) | (unsigned)lo;
                if (k > 0 && L >= min_overlap && less(dist, w, bd, bw)) {
                    bd = dist;
                    bw = w;
                }
            }
#pragma unroll
            for (int s = 16; s >= 1; s >>= 1) { // the best of the 32 lag columns of this half-wave
                const unsigned od = (unsigned)__shfl_xor((int)bd, s), ow = (unsigned)__shfl_xor((int)bw, s);
                if (less(od, ow, bd, bw)) {
                    bd = od;
                    bw = ow;
                }
            }
            if (n_lane == 0) wave_red[m] = make_uint2(bd, bw);
        }
        __syncthreads();
        if (tid < 32) {
            uint2 b = red[tid];
            for (int w = 1; w < 8; ++w) {
                const uint2 o = red[w * 32 + tid];
                if (less(o.x, o.y, b.x, b.y)) b = o;
            }
            best.offer_chunk(b.x, b.y, d0);
        }
    }

    // Chunk d0 of one (row q of k hashprints, clip r of n) by xor/popcount, 256 threads: a thread takes the lags
    // d0 + tid + 256 e up to d_hi and walks their overlaps; the best of the chunk goes to thread 0's Best through the wave
    // shuffle and red [4].  SHORT_ROWS: the chunks were laid out for a longer row, so a lag may overlap less than min_overlap.
    template <bool SHORT_ROWS>
    static __device__ __forceinline__ void popc_chunk(const uint64_t *q, int k, const uint64_t *r, int n, int min_overlap, int d0, int d_hi,
                                                      uint2 *red, Best &best, int tid)
    {
        const int lane = tid & 63, wave = tid >> 6;
        unsigned bd = kNoDist, bw = kNoW;
        // the joins' four lags unrolled (four loads in flight, 58 VGPRs), the search's rolled (32 VGPRs): what each kernel's
        // times in DESIGN.md were measured with; left alone, the compiler unrolls both
        constexpr int kUnroll = SHORT_ROWS ? kChunk / 256 : 1;
#pragma unroll kUnroll
        for (int e = 0; e < kChunk / 256; ++e) {
            const int lo = tid + 256 * e, d = d0 + lo;
            if (d > d_hi) break;
            const int j0 = max(0, -d), j1 = min(k, n - d);
            if (SHORT_ROWS && j1 - j0 < min_overlap) continue;
            unsigned dist = 0;
            for (int j = j0; j < j1; ++j) dist += (unsigned)__popcll(q[j] ^ r[d + j]);
            const unsigned w = ((kLMax - (unsigned)(j1 - j0)) << 10) | (unsigned)lo;
            if (less(dist, w, bd, bw)) {
                bd = dist;
                bw = w;
            }
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const unsigned od = (unsigned)__shfl_xor((int)bd, s), ow = (unsigned)__shfl_xor((int)bw, s);
            if (less(od, ow, bd, bw)) {
                bd = od;
                bw = ow;
            }
        }
        __syncthreads(); // (the chunk before has been read)
        if (lane == 0) red[wave] = make_uint2(bd, bw);
        __syncthreads();
        if (tid == 0) {
            uint2 b = red[0];
            for (int w = 1; w < 4; ++w)
                if (less(red[w].x, red[w].y, b.x, b.y)) b = red[w];
            best.offer_chunk(b.x, b.y, d0);
        }
    }
};

} // namespace hpfw
