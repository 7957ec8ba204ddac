"""The exact windowed cross-correlation of int16 PCM in numpy int64 (what hpfw_amd/csrc/k_xcorr.hip must equal bit for
bit), the peak rule and the score of include/hpfw_gpu.h."""
import math

import numpy as np


def window(a, start, n):
    """a[start .. start + n) as int64, 0 outside the array"""
    a = np.asarray(a)
    out = np.zeros(n, np.int64)
    s0, s1 = max(start, 0), min(start + n, a.size)
    if s1 > s0:
        out[s0 - start:s1 - start] = a[s0:s1]
    return out


def xcorr(a, b, p, q, length, radius):
    """r[l + radius] = sum_n a[p + l + n] b[q + n] over n in [0, length), l in [-radius, radius]: one int64 dot product per
    lag, a read as 0 outside [0, len(a))"""
    seg = np.asarray(b)[q:q + length].astype(np.int64)
    assert seg.size == length
    win = window(a, p - radius, length + 2 * radius)
    return np.array([np.dot(win[t:t + length], seg) for t in range(2 * radius + 1)], np.int64)


def peak_lag(r, radius):
    """the lag of the largest |r|; ties: the smaller |lag|, then the negative lag"""
    m = [abs(int(v)) for v in r]
    top = max(m)
    return min((l for l in range(-radius, radius + 1) if m[l + radius] == top), key=lambda l: (abs(l), l))


def peak(a, b, p, q, length, radius, r=None):
    """(lag, r at the lag, energy_a, energy_b) as hpfw_xcorr_peak holds them"""
    r = xcorr(a, b, p, q, length, radius) if r is None else r
    lag = peak_lag(r, radius)
    wa = window(a, p + lag, length)
    seg = np.asarray(b)[q:q + length].astype(np.int64)
    return lag, int(r[lag + radius]), int(np.dot(wa, wa)), int(np.dot(seg, seg))


def score(r, energy_a, energy_b):
    """r / (sqrt(energy_a) sqrt(energy_b)) in float64, 0 when an energy is 0"""
    if energy_a == 0 or energy_b == 0:
        return 0.0
    return float(r) / (math.sqrt(float(energy_a)) * math.sqrt(float(energy_b)))
