"""Plain restatements of S6's column stage (numpy, int64 and float64 only; nothing of the library or the oracle is used):
the planner's split N = n1 n2, the fixed-point twiddles, the exact integer column DFT before its one rounding, the int16
columns that load the kernels' paired int32 accumulators most, and the lengths the column-stage sweep runs."""
import functools

import numpy as np

N2_MAX = 6826               # the longest row transform (plan.cpp kN2Max)
FIRST_LENGTH = 54243        # below it no clip yields a hashprint
REG_N1 = 224                # n1 up to here: the register-resident kernels (even: split by parity; odd: un-split)
PAIR_N1 = 255               # n1 up to here: int32 pairing acc_0 + 2^8 acc_1, acc_2 + 2^8 acc_3

# beyond the first length of every n1 <= 255:
EXTRA_ODD_N2 = (61250, 71442, 236196, 600250, 1180980)      # even n1 (10, 14, 36, 98, 180) with odd n2
EXTRA_CHUNKS = (1048576, 1620000, 1835008, 2812500)         # n1 = 256, 270, 448 (two full chunks of 224), 450 (a third)


def _factor(n):
    """exponents of 2, 3, 5, 7 in n, or None when another prime is left"""
    e = []
    for p in (2, 3, 5, 7):
        c = 0
        while n % p == 0:
            n //= p
            c += 1
        e.append(c)
    return e if n == 1 else None


def radix_list(n):
    """passes of the length-n transform (plan.cpp make_radix_list): primes descending, pairs of 2 merged into 4"""
    c2, c3, c5, c7 = _factor(n)
    return [7] * c7 + [5] * c5 + [4] * (c2 // 2) + [3] * c3 + [2] * (c2 & 1)


def _divisors(n):
    e = _factor(n)
    ds = [1]
    for p, c in zip((2, 3, 5, 7), e):
        ds = [d * p ** k for d in ds for k in range(c + 1)]
    return sorted(ds)


def split(n):
    """(n1, n2) of a 7-smooth clip length: d0 = the smallest divisor d with n / d <= 6826; among the divisors in
    [d0, 1.25 d0] an even n2 first, then the fewest pairs of radix passes, then the smallest n1"""
    if _factor(n) is None:
        raise ValueError(f"{n} is not 7-smooth")
    d0, best, best_key = None, None, None
    for d in _divisors(n):
        if n // d > N2_MAX:
            continue
        if d0 is None:
            d0 = d
        if 4 * d > 5 * d0:
            break
        key = ((n // d) & 1, (len(radix_list(n // d)) + 1) // 2)
        if best is None or key < best_key:         # (ascending d: a tie keeps the smaller n1)
            best, best_key = d, key
    return best, n // best


def smooth_lengths(lo, hi):
    """every 7-smooth n in [lo, hi], ascending"""
    out = []
    p7 = 1
    while p7 <= hi:
        p5 = p7
        while p5 <= hi:
            p3 = p5
            while p3 <= hi:
                p2 = p3
                while p2 <= hi:
                    if p2 >= lo:
                        out.append(p2)
                    p2 *= 2
                p3 *= 3
            p5 *= 5
        p7 *= 7
    return sorted(out)


@functools.lru_cache(maxsize=None)
def first_lengths():
    """{n1: the smallest 7-smooth n >= 54243 that the rule splits as n1 x n2} for every n1 <= 255 it reaches"""
    first = {}
    for n in smooth_lengths(FIRST_LENGTH, PAIR_N1 * N2_MAX):
        n1 = split(n)[0]
        if n1 <= PAIR_N1 and n1 not in first:
            first[n1] = n
    return dict(sorted(first.items()))


def sweep_lengths():
    """the lengths of the column-stage sweep: first_lengths() in the order of n1, then the extras"""
    return tuple(first_lengths().values()) + EXTRA_ODD_N2 + EXTRA_CHUNKS


@functools.lru_cache(maxsize=None)
def wq(n1):
    """int64 [n1][2]: rint(2^22 cos(2 pi m / n1)), rint(-2^22 sin(2 pi m / n1)), the trigonometry in long double"""
    ld = np.longdouble
    a = 8 * np.arctan(ld(1)) * np.arange(n1, dtype=ld) / ld(n1)
    w = np.stack([np.rint(ld(4194304) * np.cos(a)), np.rint(-ld(4194304) * np.sin(a))], axis=1).astype(np.int64)
    w.setflags(write=False)
    return w


def row_twiddles(w, q1):
    """int64 [rows][n1][2]: wq[(q1 k1) mod n1] for the rows q1 (an int array)"""
    n1 = w.shape[0]
    return w[(np.asarray(q1, np.int64)[:, None] * np.arange(n1, dtype=np.int64)[None, :]) % n1]


def column_dft(w, x):
    """the stage's exact output before its rounding: G[q1] = sum_k1 wq[(q1 k1) mod n1] x[k1] for q1 = 0 .. n1 / 2 and a
    block x [n1][columns] of int16 columns -> int64 [n1 / 2 + 1][2 (Re, Im)][columns]"""
    n1 = w.shape[0]
    t = row_twiddles(np.asarray(w, np.int64), np.arange(n1 // 2 + 1))
    x = np.asarray(x).astype(np.int64)
    return np.stack([t[:, :, 0] @ x, t[:, :, 1] @ x], axis=1)


def balanced_digits(w):
    """three balanced base-256 digits of the twiddles, w = d0 + 2^8 d1 + 2^16 d2 with d0, d1 in [-128, 127]: [3, ...]"""
    w = np.asarray(w, np.int64)
    d0 = ((w + 128) & 255) - 128
    w1 = (w - d0) >> 8
    d1 = ((w1 + 128) & 255) - 128
    return np.stack([d0, d1, (w1 - d1) >> 8])


def sample_digits(x):
    """x = 256 hi + lo + 128: lo = (x & 255) - 128 (sample digit 0), hi = x >> 8 (digit 1), both in [-128, 127]"""
    x = np.asarray(x).astype(np.int64)
    return (x & 255) - 128, x >> 8


def pair_coefficients(w_part, pair):
    """the paired accumulator as a linear form in the sample digits: sum_k1 a[k1] lo[k1] + b[k1] hi[k1].  Digit products
    of weight c = i + j (sample digit i, twiddle digit j) share accumulator acc_c, so
      acc_0 + 2^8 acc_1 = sum lo (d0 + 2^8 d1) + hi 2^8 d0,    acc_2 + 2^8 acc_3 = sum lo d2 + hi (d1 + 2^8 d2)"""
    d0, d1, d2 = balanced_digits(w_part)
    return (d0 + 256 * d1, 256 * d0) if pair == 0 else (d2, d1 + 256 * d2)


def worst_case_columns(n1, q1, part, pair, odd_sign=1):
    """(column int16 [n1], value): the column that drives the paired int32 accumulator `pair` (0: acc_0 + 2^8 acc_1,
    1: acc_2 + 2^8 acc_3) of row q1, part 0 (Re) or 1 (Im), furthest from zero, and the value it reaches.  The
    accumulator is linear in (hi, lo) of every k1, each in [-128, 127]: every k1 takes the best of its four corners.
    odd_sign = -1: the form with the odd k1 negated, E - O of the parity-split kernel."""
    w = wq(n1)[(q1 * np.arange(n1, dtype=np.int64)) % n1, part]
    a, b = pair_coefficients(w, pair)
    if odd_sign < 0:
        a, b = a.copy(), b.copy()
        a[1::2] *= -1
        b[1::2] *= -1
    best = None
    for s in (1, -1):                              # towards +inf and towards -inf
        lo = np.where(s * a > 0, 127, -128)
        hi = np.where(s * b > 0, 127, -128)
        v = int((a * lo + b * hi).sum())
        if best is None or abs(v) > abs(best[2]):
            best = (lo, hi, v)
    lo, hi, v = best
    return (256 * hi + lo + 128).astype(np.int16), v


@functools.lru_cache(maxsize=None)
def worst_case_table(n1):
    """(columns int16 [hq][2 part][2 pair][n1], values int64 [hq][2][2]) of worst_case_columns for every row"""
    hq = n1 // 2 + 1
    cols = np.zeros((hq, 2, 2, n1), np.int16)
    vals = np.zeros((hq, 2, 2), np.int64)
    for q1 in range(hq):
        for part in range(2):
            for pair in range(2):
                cols[q1, part, pair], vals[q1, part, pair] = worst_case_columns(n1, q1, part, pair)
    cols.setflags(write=False)
    vals.setflags(write=False)
    return cols, vals


def noise_clip(n):
    """full-scale noise, seeded with n, with both ends of the int16 range planted"""
    clip = np.random.default_rng(n).integers(-32768, 32768, n).astype(np.int16)
    clip[::97] = 32767
    clip[5::89] = -32768
    return clip


def worst_clip(n):
    """a clip tiled from worst-case columns: column k2 of the [n1][n2] sample matrix is the worst_case_columns column of
    row q1 = k2 mod (n1 / 2 + 1), with (Re, pair 0), (Re, pair 1), (Im, pair 0), (Im, pair 1) in turn from one run of
    rows to the next"""
    n1, n2 = split(n)
    hq = n1 // 2 + 1
    cols = worst_case_table(n1)[0]
    k2 = np.arange(n2)
    v = (k2 // hq) % 4
    return np.ascontiguousarray(cols[k2 % hq, v >> 1, v & 1].T).reshape(-1)      # [n1][n2] as it lies


def float64_error(x, clip, kmin, kmax):
    """largest error of forward bins x [kmax - kmin][2] against the float64 transform of clip / 32768, over max |ref|"""
    ref = np.fft.rfft(np.asarray(clip, np.float64) / 32768.0)[kmin:kmax]
    x = np.asarray(x, np.float64)
    return float(np.abs(x[:, 0] + 1j * x[:, 1] - ref).max() / np.abs(ref).max())
