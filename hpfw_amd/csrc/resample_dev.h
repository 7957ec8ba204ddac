// resample_dev.h -- what the two kernels of the sample-rate conversion share (DESIGN.md sections 10 and 14): resample_kernel
// (k_resample.hip, a clip at a time) and ring_resample_append_kernel (k_streams_resample.hip, the chunks of live feeds).  The
// geometry of a pass, the staging of a span of int16 samples in LDS, and one output's T products: both kernels produce an
// output with the same instructions on the same operands, which is what makes a feed's ring equal the file's conversion.
#pragma once
#include "kernels.h"

namespace hpfw {
namespace {

constexpr int kRsThreads = 256;
constexpr int kRsPerLane = 8;
constexpr int kRsTile = kRsThreads * kRsPerLane; // outputs per pass
constexpr int kRsPasses = 8;                      // passes per workgroup (the table is staged once for them)
constexpr size_t kRsLdsMax = 64 * 1024;           // table + samples in LDS up to this

typedef short s16x2 __attribute__((ext_vector_type(2)));

// samples [lo, lo + span) of clip x into s, zeros outside [0, n)
__device__ inline void stage_span(const int16_t *__restrict__ x, int64_t n, int64_t lo, int span, int16_t *s)
{
    const int64_t g0 = lo < 0 ? 0 : lo, g1 = lo + span < n ? lo + span : n; // the part inside the clip
    int64_t v0 = g1, nv = 0;                                               // 16-byte-aligned chunks [v0, v0 + 8 nv)
    if (g0 < g1 && !((uintptr_t)(x + g0) & 1)) {
        v0 = g0 + (int64_t)((16 - ((uintptr_t)(x + g0) & 15)) & 15) / 2;
        nv = v0 < g1 ? (g1 - v0) / 8 : 0;
    }
    const int64_t v1 = v0 + 8 * nv;
    for (int j = threadIdx.x; j < span; j += kRsThreads) {
        const int64_t gi = lo + j;
        if (gi < g0 || gi >= g1) s[j] = 0;
        else if (gi < v0 || gi >= v1) s[j] = x[gi];
    }
    const int4 *xv = reinterpret_cast<const int4 *>(x + v0);
    for (int64_t v = threadIdx.x; v < nv; v += kRsThreads) {
        const int4 q = xv[v];
        int16_t *d = s + (v0 - lo) + 8 * v;
        const int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            d[2 * i] = (int16_t)(w[i] & 0xffff);
            d[2 * i + 1] = (int16_t)((uint32_t)w[i] >> 16);
        }
    }
}

__device__ __forceinline__ int dot2(uint32_t a, uint32_t b, int acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b), acc, false);
}

// One output: the staged samples as words sw, the first tap's sample k (an odd k: each pair straddles two words), the phase's
// row of `chunks` 16-byte chunks of taps.  clamp((sum + 2^13) >> 14)
__device__ __forceinline__ int16_t rs_output(const uint32_t *sw, uint32_t k, const int4 *row, int chunks)
{
    const uint32_t *xs = sw + (k >> 1);
    const uint32_t sh = (k & 1) * 16;
    int acc = 0;
    uint32_t prev = xs[0];
    for (int c = 0; c < chunks; ++c) {
        const int4 tv = row[c];
        const uint32_t w1 = xs[4 * c + 1], w2 = xs[4 * c + 2], w3 = xs[4 * c + 3], w4 = xs[4 * c + 4];
        acc = dot2(__builtin_amdgcn_alignbit(w1, prev, sh), (uint32_t)tv.x, acc);
        acc = dot2(__builtin_amdgcn_alignbit(w2, w1, sh), (uint32_t)tv.y, acc);
        acc = dot2(__builtin_amdgcn_alignbit(w3, w2, sh), (uint32_t)tv.z, acc);
        acc = dot2(__builtin_amdgcn_alignbit(w4, w3, sh), (uint32_t)tv.w, acc);
        prev = w4;
    }
    int v = (acc + (1 << (kRsShift - 1))) >> kRsShift;
    v = v < -32768 ? -32768 : (v > 32767 ? 32767 : v);
    return (int16_t)v;
}

// the sample buffer of a pass in int16 slots: floor(m_last M / L) - floor(m0 M / L) + 2 rw + 2 <= ((tile - 1) M + L - 1) / L + 2 rw + 2
inline uint32_t rs_span_cap(int32_t L, int32_t M, uint32_t rw)
{
    const uint64_t span_max = ((uint64_t)(kRsTile - 1) * M + L - 1) / L + 2ull * rw + 2;
    return (uint32_t)((span_max + 7) / 8 * 8);
}

} // namespace
} // namespace hpfw
