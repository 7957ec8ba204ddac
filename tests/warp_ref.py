"""numpy restatement of the time-warp contract: a track of int16 PCM read at the affine position
i0 + m + (f0 + m d) 2^-40 through a polyphase windowed sinc, and the mix of such tracks, in exact integer arithmetic.  A test
helper, not part of oracle/."""
from fractions import Fraction

import numpy as np

PB = 12
P = 1 << PB                    # phase rows: row p is the filter of the fractional delay p / P
H = 16                         # taps per row T = 2 H
T = 2 * H
FC, BETA = 1.0, 8.0            # cutoff at Nyquist (row 0 is then the unit impulse), Kaiser beta of section 10
SHIFT = 14                     # taps are fixed point with 14 fraction bits: every row sums to 2^14
FRAC = 40                      # fraction bits of the position
D_MAX, G_MAX, M_END, I0_MAX = 1 << 30, 1 << 17, 1 << 31, 1 << 62


def design():
    """taps int16 [P][T]"""
    p = np.arange(P, dtype=np.float64)[:, None]
    j = np.arange(T, dtype=np.float64)[None, :]
    tau = j - H + 1 - p / P
    win = np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - (tau / H) ** 2))) / np.i0(BETA)
    h = FC * np.sinc(FC * tau) * win
    h = h / h.sum(axis=1, keepdims=True)
    q = np.rint(h * (1 << SHIFT)).astype(np.int64)
    q[:, H - 1] += (1 << SHIFT) - q.sum(axis=1)
    assert (q.sum(axis=1) == 1 << SHIFT).all()
    assert (32768 * np.abs(q).sum(axis=1) < 1 << 31).all()
    assert np.abs(q).max() < 32768
    return q.astype(np.int16)


_TAPS = []


def taps():
    if not _TAPS:
        _TAPS.append(design())
    return _TAPS[0]


def position(i0, f0, d, m):
    """(ip, phase) of outputs m (int64 array): u = f0 + m d, ip = i0 + m + (u >> 40), phase = the top PB bits of u's fraction"""
    m = np.asarray(m, np.int64)
    u = np.int64(f0) + m * np.int64(d)
    return np.int64(i0) + m + (u >> FRAC), (u & ((1 << FRAC) - 1)) >> (FRAC - PB)


def raw(x, i0, f0, d, m0, n_out, h=None):
    """(acc + 2^13) >> 14 before any clamp, int64 [n_out], for outputs m0 .. m0 + n_out - 1 of source x (int16 [src_len])"""
    assert 0 <= f0 < 1 << FRAC and abs(d) <= D_MAX and 0 <= m0 and m0 + n_out <= M_END and abs(i0) <= I0_MAX
    h = np.ascontiguousarray(taps() if h is None else h, np.int16).astype(np.int32)
    n_taps = h.shape[1]
    xp = np.concatenate([[0], np.asarray(x, np.int16).ravel(), [0]]).astype(np.int32)     # x with a zero on either side
    ip, ph = position(i0, f0, d, m0 + np.arange(n_out, dtype=np.int64))
    first = ip - n_taps // 2 + 1
    acc = np.zeros(n_out, np.int32)                         # exact: 32768 sum |h| < 2^31 for every row
    for j in range(n_taps):
        acc += xp[np.clip(first + j, -1, xp.size - 2) + 1] * h[ph, j]
    return (acc.astype(np.int64) + (1 << (SHIFT - 1))) >> SHIFT


def warp(x, i0, f0, d, m0, n_out, gain=1, h=None):
    """one track, int16 [n_out]: a negative gain negates before the clamp, its size is ignored"""
    v = raw(x, i0, f0, d, m0, n_out, h)
    return np.clip(-v if gain < 0 else v, -32768, 32767).astype(np.int16)


def mix_tracks(ys, gains):
    """clamp((sum_k g_k y_k + 2^14) >> 15) of materialised, un-negated tracks ys [n_tracks][n_out]"""
    ys = np.asarray(ys, np.int64).reshape(len(gains), -1)
    s = (ys * np.asarray(gains, np.int64)[:, None]).sum(axis=0)
    return np.clip((s + (1 << 14)) >> 15, -32768, 32767).astype(np.int16)


def mix(sources, maps, gains, m0, n_out, h=None):
    """sources: int16 arrays, maps: (i0, f0, d) per source, gains Q15 with |g| <= 2^17 -> int16 [n_out]"""
    assert all(abs(int(g)) <= G_MAX for g in gains)
    if not len(sources):
        return np.zeros(n_out, np.int16)
    return mix_tracks([warp(x, *mp, m0, n_out, 1, h) for x, mp in zip(sources, maps)], gains)


def time_map_q40(A, B):
    """(i0, f0, d) of the inverse of t = A + (1 + B) n, in exact rationals: output m reads the source at (m - A) / (1 + B)
    = m + pos0 + m r with r = 1 / (1 + B) - 1; d = r 2^40 and i0 2^40 + f0 = pos0 2^40, each rounded to the nearest integer"""
    A, B = Fraction(float(A)), Fraction(float(B))
    r = 1 / (1 + B) - 1
    if abs(r) > Fraction(1, 1 << 10):
        raise ValueError("time map: |1 / (1 + B) - 1| > 2^-10")
    pos = round(-A / (1 + B) * (1 << FRAC))
    return pos >> FRAC, pos & ((1 << FRAC) - 1), round(r * (1 << FRAC))


def time_map_error(A, B, i0, f0, d, m):
    """|i0 + m + (f0 + m d) 2^-40 - (m - A) / (1 + B)| as an exact rational, and its bound 2^-40 + m 2^-41"""
    got = i0 + m + Fraction(f0 + m * d, 1 << FRAC)
    return abs(got - (m - Fraction(float(A))) / (1 + Fraction(float(B)))), Fraction(1, 1 << FRAC) + Fraction(m, 1 << (FRAC + 1))
