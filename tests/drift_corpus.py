"""The corpus of the drift and render tests: four recordings of one 90 s piece, cut off the 441-sample
grid, each on a clock of its own -- 0, +60, -250 and +400 ppm, warped by tests/warp_ref.py -- with independent noise 20 dB
below, one at gain -0.5, one behind 1.5 s of digital silence.  A test helper."""
import numpy as np

from hpfw_amd import synth

import warp_ref

SR = synth.SR
PPM = (0, 60, -250, 400)
D = tuple(int(round(p * 1e-6 * 2 ** 40)) for p in PPM)              # the clocks in the warp's fixed point
RATES = tuple(1.0 + d / 2.0 ** 40 for d in D)                       # source samples per sample of the recording
CUTS = (2 * SR + 17, 5 * SR + 230, 123, 7 * SR + 400)               # where each recording starts in the piece: off the grid
GAIN = (1.0, 1.0, -0.5, 1.0)
SILENCE = (0, int(1.5 * SR), 0, 0)
REC_LEN = 80 * SR
SNR_DB = 20.0


def recordings():
    """int16 recordings; sample n of recording k sits at A[k] + RATES[k] n of the piece"""
    src = synth.gen_clip(91, 90.0)
    out = []
    for k in range(4):
        assert CUTS[k] % 441 and CUTS[k] + RATES[k] * REC_LEN + warp_ref.T < src.size
        seg = warp_ref.warp(src, CUTS[k], 0, D[k], 0, REC_LEN).astype(np.float64)
        rng = np.random.default_rng([synth.SEED, 1600 + k])
        noise = np.sqrt(float(np.mean(seg ** 2)) / 10 ** (SNR_DB / 10)) * rng.standard_normal(seg.size)
        x = np.clip(np.round(GAIN[k] * (seg + noise)), -32768, 32767).astype(np.int16)
        out.append(np.concatenate([np.zeros(SILENCE[k], np.int16), x]))
    return out


A = tuple(CUTS[k] - RATES[k] * SILENCE[k] for k in range(4))


def pair_truth(i, j):
    """(offset, drift) of query i against recording j: query[n + offset + drift n] ~ recording[n]"""
    return (A[j] - A[i]) / RATES[i], RATES[j] / RATES[i] - 1.0


def component_truth():
    """(starts, rates) on the clock of recording 0, the earliest start at 0"""
    starts = [(A[k] - A[0]) / RATES[0] for k in range(4)]
    return tuple(s - min(starts) for s in starts), tuple(RATES[k] / RATES[0] for k in range(4))
