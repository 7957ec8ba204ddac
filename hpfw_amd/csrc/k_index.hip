// k_index.hip -- removing clips from the index in place (the plan and its order: index_plan.h).
//
// A chunk of the plan is a segmented gather.  A workgroup takes a tile of kIndexTile DESTINATION hashprints, aligned on 16
// bytes of the destination, finds the pieces of moves that cover it (the pieces of a chunk tile its destinations without a
// gap, ascending) and copies: a thread writes two adjacent hashprints with one 16-byte store.  The shift src - dst may be
// odd, so a source is only 8-byte aligned: a thread loads 16 bytes where both words come from one piece at an even source,
// two 8-byte words otherwise (the same for every thread inside one piece).
// A direct chunk is one index_gather from the index into the index.  A staged chunk is index_gather into the staging buffer,
// then index_copy from there: hashprint e of the chunk waits at staging[e - (lo & ~1)], so the copy is 16-byte aligned at
// both ends.  No workgroup waits for another, there is no atomic, and every position and count is 64-bit.
#include "kernels.h"

namespace hpfw {

namespace {

constexpr int kThreads = 256;
constexpr int kPairs = kIndexTile / 2 / kThreads; // 16-byte stores per thread
static_assert(kPairs * kThreads * 2 == kIndexTile, "a tile is a whole number of 16-byte stores per thread");

// the last piece of [a, b] whose destination begins at or below e (piece a does)
__device__ __forceinline__ int64_t piece_of(const hpfw_index_move *mv, int64_t a, int64_t b, int64_t e)
{
    while (a < b) {
        const int64_t mid = a + (b - a + 1) / 2;
        if (mv[mid].dst <= e) a = mid;
        else b = mid - 1;
    }
    return a;
}

// out[e - out_shift] = in[src + (e - dst)] of the piece (dst, src, len) that holds e, for e in [lo, hi); the pieces
// mv[0 .. n_mv) cover [lo, hi) exactly; out_shift is even
__global__ __launch_bounds__(kThreads) void index_gather(uint64_t *__restrict__ out, int64_t out_shift, const uint64_t *__restrict__ in,
                                                         const hpfw_index_move *__restrict__ mv, int64_t n_mv, int64_t lo, int64_t hi)
{
    const int64_t t0 = (lo & ~(int64_t)1) + (int64_t)blockIdx.x * kIndexTile; // even
    if (t0 >= hi) return;
    const int64_t t_first = t0 > lo ? t0 : lo, t_last = (t0 + kIndexTile < hi ? t0 + kIndexTile : hi) - 1;
    // the pieces of this tile (the same for every thread)
    const int64_t m_a = piece_of(mv, 0, n_mv - 1, t_first), m_b = piece_of(mv, m_a, n_mv - 1, t_last);
#pragma unroll 2
    for (int i = 0; i < kPairs; ++i) {
        const int64_t e = t0 + 2 * ((int64_t)i * kThreads + threadIdx.x);
        const bool has0 = e >= lo && e < hi, has1 = e + 1 >= lo && e + 1 < hi;
        if (!has0 && !has1) continue;
        const int64_t m0 = piece_of(mv, m_a, m_b, has0 ? e : e + 1);
        const hpfw_index_move p0 = mv[m0];
        uint64_t v0 = 0, v1 = 0;
        if (has0 && has1) {
            const int64_t k = e - p0.dst;
            if (k + 1 < p0.len) { // both words in one piece
                const int64_t s0 = p0.src + k;
                if (!(s0 & 1)) {
                    const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(in + s0);
                    v0 = v.x;
                    v1 = v.y;
                } else {
                    v0 = in[s0];
                    v1 = in[s0 + 1];
                }
            } else { // the second word opens the next piece
                v0 = in[p0.src + k];
                const hpfw_index_move p1 = mv[m0 + 1 < n_mv ? m0 + 1 : m0];
                v1 = in[p1.src + (e + 1 - p1.dst)];
            }
            *reinterpret_cast<ulonglong2 *>(out + (e - out_shift)) = make_ulonglong2(v0, v1);
        } else { // the first or last hashprint of the chunk alone
            const int64_t e1 = has0 ? e : e + 1;
            out[e1 - out_shift] = in[p0.src + (e1 - p0.dst)];
        }
    }
}

// out[e] = in[e - in_shift] for e in [lo, hi); in_shift even
__global__ __launch_bounds__(kThreads) void index_copy(uint64_t *__restrict__ out, const uint64_t *__restrict__ in, int64_t in_shift, int64_t lo,
                                                       int64_t hi)
{
    const int64_t t0 = (lo & ~(int64_t)1) + (int64_t)blockIdx.x * kIndexTile;
#pragma unroll 2
    for (int i = 0; i < kPairs; ++i) {
        const int64_t e = t0 + 2 * ((int64_t)i * kThreads + threadIdx.x);
        const bool has0 = e >= lo && e < hi, has1 = e + 1 >= lo && e + 1 < hi;
        if (has0 && has1)
            *reinterpret_cast<ulonglong2 *>(out + e) = *reinterpret_cast<const ulonglong2 *>(in + (e - in_shift));
        else if (has0)
            out[e] = in[e - in_shift];
        else if (has1)
            out[e + 1] = in[e + 1 - in_shift];
    }
}

unsigned index_tiles(int64_t lo, int64_t hi) { return (unsigned)((hi - (lo & ~(int64_t)1) + kIndexTile - 1) / kIndexTile); }

} // namespace

void launch_index_gather(uint64_t *d_out, int64_t out_shift, const uint64_t *d_in, const hpfw_index_move *d_moves, int64_t n_moves, int64_t lo,
                         int64_t hi, hipStream_t s)
{
    if (hi <= lo || n_moves < 1) return;
    hipLaunchKernelGGL(index_gather, dim3(index_tiles(lo, hi)), dim3(kThreads), 0, s, d_out, out_shift, d_in, d_moves, n_moves, lo, hi);
}

void launch_index_copy(uint64_t *d_out, const uint64_t *d_in, int64_t in_shift, int64_t lo, int64_t hi, hipStream_t s)
{
    if (hi <= lo) return;
    hipLaunchKernelGGL(index_copy, dim3(index_tiles(lo, hi)), dim3(kThreads), 0, s, d_out, d_in, in_shift, lo, hi);
}

} // namespace hpfw
