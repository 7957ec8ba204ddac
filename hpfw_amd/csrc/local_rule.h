// local_rule.h -- the run rule of the local search (k_search_local.hip) and the local self-join
// (k_localjoin.hip, section 26) on the device, stated once.  With x_j = T - popcount(q[j] ^ r[d + j]) (T = max_rate, 1..31) a
// run [j0, j1) at lag d scores sum x_j; the best run: larger score, then smaller j1, then smaller j0.  Device code only;
// everything here is inlined into its kernel.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "overlap_rule.h"

namespace hpfw {

typedef int i32x16 __attribute__((ext_vector_type(16)));

// one accumulator tile after a step: cur is twice the best run that ends here; a run that scores below 0 is not continued.
// Both maxima are taken on the bit patterns as signed integers (bs holds best's): the other operand is never negative, and
// against a value >= 0 the two orders agree -- a negative float, -0 included, is a negative integer.  A float maximum would
// cost a second instruction per operand, the canonicalisation of a value the compiler cannot see the origin of.
__device__ __forceinline__ void scan_tile(f32x16 &cur, i32x16 &bs)
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
__device__ __forceinline__ v4i minus_ones(int cnt)
{
    v4i r;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int nib = min(max(cnt - 8 * w, 0), 8);
        r[w] = nib == 8 ? (int)0xAAAAAAAAu : (int)(0xAAAAAAAAu & ((1u << (4 * nib)) - 1u));
    }
    return r;
}

// the best run [j0, j1) of q (k hashprints) on the diagonal d of r (n hashprints): the forward pass over the diagonal --
// prefix minimum updated on strict <, best on strict >
struct LocalRun {
    int score, j0, j1;
};
__device__ __forceinline__ LocalRun local_walk(const uint64_t *q, const uint64_t *r, int d, int k, int n, int T)
{
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
    return {bs, j0, j1};
}

} // namespace hpfw
