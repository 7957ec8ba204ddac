"""numpy restatement of the sample-rate conversion contract: polyphase windowed sinc from an
integer rate fs in [8 000, 192 000] to 44 100 Hz in exact integer arithmetic.  A test helper, not part of oracle/."""
import math

import numpy as np

OUT_RATE = 44100
RHO, ZEROS, BETA = 0.9, 16, 8.0
SHIFT = 14                     # taps are fixed point with 14 fraction bits: every phase sums to 2^14
RATES = (8000, 11025, 16000, 22050, 24000, 32000, 37800, 44056, 48000, 88200, 96000, 192000)


def ratio(fs):
    """(L, M): output sample m sits at input time m * M / L"""
    g = math.gcd(OUT_RATE, fs)
    return OUT_RATE // g, fs // g


def half_taps(fs):
    """H = ceil(Z * max(1, M / L) / rho) in integers (rho = 9 / 10)"""
    L, M = ratio(fs)
    return (10 * ZEROS * max(L, M) + 9 * L - 1) // (9 * L)


def out_length(n_in, fs):
    L, M = ratio(fs)
    return -(-n_in * L // M)


def design(fs):
    """(L, M, taps int16 [L][2H])"""
    L, M = ratio(fs)
    H = half_taps(fs)
    T = 2 * H
    fc = RHO * min(1.0, L / M)
    p = np.arange(L, dtype=np.float64)[:, None]
    j = np.arange(T, dtype=np.float64)[None, :]
    tau = j - H + 1 - p / L
    win = np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - (tau / H) ** 2))) / np.i0(BETA)
    h = fc * np.sinc(fc * tau) * win
    h = h / h.sum(axis=1, keepdims=True)
    q = np.rint(h * (1 << SHIFT)).astype(np.int64)
    q[:, H - 1] += (1 << SHIFT) - q.sum(axis=1)
    assert (q.sum(axis=1) == 1 << SHIFT).all()
    assert (32768 * np.abs(q).sum(axis=1) < 1 << 31).all()
    assert np.abs(q).max() < 32768
    return L, M, q.astype(np.int16)


def resample(x, fs, taps=None):
    """int16 [n] or [clips][n] at fs -> int16 at 44 100 Hz; `taps`: a table to use in place of design(fs)"""
    x = np.asarray(x, np.int16)
    if x.ndim == 2:
        return np.stack([resample(c, fs, taps) for c in x]) if len(x) else np.zeros((0, out_length(x.shape[1], fs)), np.int16)
    if fs == OUT_RATE:
        return x.copy()
    L, M, h = design(fs) if taps is None else (*ratio(fs), np.asarray(taps))
    T = h.shape[1]
    H = T // 2
    n_in = x.size
    n_out = out_length(n_in, fs)
    m = np.arange(n_out, dtype=np.int64)
    i0 = m * M // L
    p = m * M % L
    xp = np.concatenate([np.zeros(H, np.int64), x.astype(np.int64), np.zeros(H + 1, np.int64)])
    acc = np.zeros(n_out, np.int64)
    hh = h.astype(np.int64)
    for jj in range(T):
        acc += xp[i0 + jj + 1] * hh[p, jj]          # x[i0 - H + 1 + jj], x padded with H zeros in front
    return np.clip((acc + (1 << (SHIFT - 1))) >> SHIFT, -32768, 32767).astype(np.int16)
