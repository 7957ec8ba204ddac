// db_spec.h -- the dB term of DESIGN.md S8, t(p) = (float)(10 log10_d(max(p, 1e-10))), shared by the
// kernels that produce spectrogram values (convert.h:7-16 of the reference).
//
// db_term_spec is the specification: a fixed sequence of IEEE operations in double.  db_term_fast returns the same
// float for every input by a cheaper evaluation that knows when it cannot be sure and then takes the specified sequence.
// tests/emu/db_term_check.cpp compiles this text for the host (simt.h) and compares the two on every float.
#pragma once
#include "simt.h"
#include "db_tab.h"

namespace hpfw {

// log10 in double by a fixed sequence of IEEE operations
HPFW_DEVICE double log10_spec(double x)
{
    unsigned long long u = __builtin_bit_cast(unsigned long long, x);
    int e = (int)((u >> 52) & 0x7ff) - 1023;
    u = (u & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL;
    double m = __builtin_bit_cast(double, u);
    if (m > 1.4142135623730951) {
        m *= 0.5;
        e += 1;
    }
    const double f = m - 1.0;
    const double s = f / (2.0 + f);
    const double z = s * s;
    double r = 1.0 / 23.0;
    r = __builtin_fma(r, z, 1.0 / 21.0);
    r = __builtin_fma(r, z, 1.0 / 19.0);
    r = __builtin_fma(r, z, 1.0 / 17.0);
    r = __builtin_fma(r, z, 1.0 / 15.0);
    r = __builtin_fma(r, z, 1.0 / 13.0);
    r = __builtin_fma(r, z, 1.0 / 11.0);
    r = __builtin_fma(r, z, 1.0 / 9.0);
    r = __builtin_fma(r, z, 1.0 / 7.0);
    r = __builtin_fma(r, z, 1.0 / 5.0);
    r = __builtin_fma(r, z, 1.0 / 3.0);
    r = __builtin_fma(r, z, 1.0);
    const double lm = 2.0 * s * r;
    return __builtin_fma((double)e, 0.30102999566398119521, lm * 0.43429448190325182765);
}

HPFW_DEVICE float db_term_spec(float pw)
{
    const float xx = pw < 1e-10f ? 1e-10f : pw;
    return (float)(10.0 * log10_spec((double)xx));
}

// ---- the same value without the division and the long series -------------------------------------------------------
// (double)p = 2^e m, m in [1, 2); the top HPFW_DB_CELL_BITS bits of m's fraction choose a cell with centre c; with
// r = m / c - 1 (|r| < 2^-(HPFW_DB_CELL_BITS + 1)), y = e 10 log10(2) + 10 log10(c) + 10 log10(1 + r), the last term by
// its series to degree HPFW_DB_DEGREE.  |y - 10 log10_spec| stays below HPFW_DB_DELTA / 32 (every input tried,
// profiles/r06_db_term.md), so where (float)(y - HPFW_DB_DELTA) and (float)(y + HPFW_DB_DELTA) are the same float the specified
// value, which lies between them and is rounded the same way, is that float too.  Elsewhere -- about eleven inputs in a
// million -- and for every p outside [1e-10, inf) the specified sequence runs.
struct alignas(16) DbCell {
    double inv_c, t; // 1 / c, 10 log10(c)
};
#if defined(HPFW_SIMT_EMU)
static const DbCell kDbTab[1 << HPFW_DB_CELL_BITS] = HPFW_DB_TABLE;
#else
// the master copy, in global memory: db_kernel, the Mel dB kernel, the large-band path and cq_kernel's classes of fewer
// than 256 threads read it directly; the other classes of cq_kernel copy it into the LDS behind their data (k_cq.hip)
static __device__ const DbCell kDbTab[1 << HPFW_DB_CELL_BITS] = HPFW_DB_TABLE;
#endif
#if !defined(HPFW_DB_DELTA)
#define HPFW_DB_DELTA 0x1p-37 // 7.3e-12, 32 times the largest |y - 10 log10_spec| of any input (2^-42)
#endif

// y of the comment above for 1e-10f <= pw < inf; a finite number without meaning for any other pw (the cell index is masked).
// tab: kDbTab or a copy of it (cq_kernel keeps one in LDS)
HPFW_DEVICE double db_fast_y(float pw, const DbCell *tab = kDbTab)
{
    constexpr double kPoly[HPFW_DB_DEGREE] = HPFW_DB_POLY;
    const unsigned long long u = __builtin_bit_cast(unsigned long long, (double)pw);
    const unsigned hi = (unsigned)(u >> 32);
    const DbCell cell = tab[(hi >> (20 - HPFW_DB_CELL_BITS)) & ((1u << HPFW_DB_CELL_BITS) - 1)];
    const double m = __builtin_bit_cast(double, (u & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL);
    const double r = __builtin_fma(m, cell.inv_c, -1.0);
    double q = kPoly[HPFW_DB_DEGREE - 1];
    for (int k = HPFW_DB_DEGREE - 2; k >= 0; --k) q = __builtin_fma(q, r, kPoly[k]);
    const double base = __builtin_fma((double)((int)(hi >> 20) - 1023), HPFW_DB_LOG2, cell.t);
    return __builtin_fma(q, r, base);
}

// 1e-10f <= pw < inf, on the bit pattern: negative values, NaN and whatever the clamp would replace fail it
HPFW_DEVICE bool db_fast_in_range(float pw)
{
    constexpr unsigned kLowest = __builtin_bit_cast(unsigned, 1e-10f);
    return __builtin_bit_cast(unsigned, pw) - kLowest < 0x7f800000u - kLowest;
}

// true: t is the dB term of pw.  false: the specified sequence has to say
HPFW_DEVICE bool db_fast_certain(float pw, float &t, const DbCell *tab = kDbTab)
{
    const double y = db_fast_y(pw, tab);
    t = (float)(y - HPFW_DB_DELTA);
    return db_fast_in_range(pw) && t == (float)(y + HPFW_DB_DELTA);
}

HPFW_DEVICE float db_term_fast(float pw, const DbCell *tab = kDbTab)
{
    float t;
    if (db_fast_certain(pw, t, tab)) return t;
    return db_term_spec(pw);
}

// FAST: HPFW_DB_TERM at handle creation (default: the fast evaluation; "spec": the specified sequence only)
template <bool FAST>
HPFW_DEVICE float db_term(float pw)
{
    return FAST ? db_term_fast(pw) : db_term_spec(pw);
}

} // namespace hpfw
