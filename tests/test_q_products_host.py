"""The six-product split of the hashprint kernel on the CPU: the digit classes restated in numpy
(tests/q_products_ref.py) against the oracle's exact integer sums, the bound on the low part, and the rule that calls a
sign certain."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q_products_ref as ref  # noqa: E402
from hpfw_amd import synth  # noqa: E402


def db_of(u):
    """a dB spectrogram that quantises to the int grid values u (-80 * 98304 <= u <= 0): u / 98304 in float32 is off by
    less than 2^-24 |u| / 98304, so rint(S * 98304) gives u back -- checked by the caller through oracle.quantise_db"""
    return (np.asarray(u, np.float64) / 98304.0).astype(np.float32)


def check(oracle, filt, db, need_open=False):
    d, dp, dl, lm, is_open, _ = ref.split(oracle, filt, db)
    assert np.array_equal(d, oracle.delta_q(filt, db))                       # sum_c 2^(8c) A_c is the oracle's D
    assert np.array_equal((dp << 16) + dl, d)
    assert (np.abs(dl) <= lm[:, None]).all()                                 # |Dl| <= Lmax_r for every row
    certain = ~is_open
    assert np.array_equal((dp >= 0)[certain], (d >= 0)[certain])             # the sign of Dp is the sign of D
    assert not is_open[lm == 0].any()                                        # Lmax_r = 0: D = 2^16 Dp, never open
    if need_open:
        assert is_open.any()
    return d, dp, dl, lm, is_open


def test_split_on_a_clip(oracle, filters):
    clip = synth.gen_clip(0, 30.0)
    plan = oracle.Plan(clip.size)
    db = oracle.db(plan.cqmag(plan.spectrum(clip)))
    _, _, dl, lm, is_open = check(oracle, filters, db)
    assert 0 < is_open.sum() < 1e-3 * is_open.size                           # a few values in ten thousand are open
    assert np.abs(dl).max() < lm.max()


def test_split_on_random_input(oracle):
    rng = np.random.default_rng(8)
    filt = rng.standard_normal(2420 * 64).astype(np.float32) * 0.05
    db = rng.uniform(-80, 0, (121, 400)).astype(np.float32)
    check(oracle, filt, db)


def test_split_with_a_zero_row_and_a_row_of_one_tap(oracle):
    rng = np.random.default_rng(9)
    f = rng.standard_normal((2420, 64)).astype(np.float32) * 0.03            # [k][r]
    f[:, 0] = 0.0
    f[:, 1] = 0.0
    f[17, 1] = 1.0                                                           # fq = 2^21: digits 0 and 1 are zero
    f[:, 2] = 0.0
    f[40, 2] = 0.7519                                                        # a tap with low digits
    filt = np.ascontiguousarray(f).ravel()
    db = rng.uniform(-80, 0, (121, 300)).astype(np.float32)
    db[:, 100:] = db[:, 99:100]                                              # a stretch of zero differences
    d, dp, dl, lm, is_open = check(oracle, filt, db, need_open=True)
    assert lm[0] == 0 and lm[1] == 0 and lm[2] > 0
    assert (d[0] == 0).all() and not is_open[:2].any()


def test_split_on_a_constant_spectrogram(oracle, filters):
    db = np.full((121, 260), -37.25, np.float32)
    d, dp, dl, lm, is_open = check(oracle, filters, db, need_open=True)
    assert (d == 0).all() and is_open[lm > 0].all()                          # Dp = 0 <= Lmax: open wherever the row has low digits


def driven(oracle, fq_row, b0, b1):
    """filters whose row 5 quantises to fq_row, and a spectrogram of one hashprint whose Du at tap k has the low digits
    b0[k], b1[k] (third digit 0): (Dl of row 5, Lmax of row 5)"""
    f = np.zeros((2420, 64), np.float32)
    f[:, 5] = (fq_row.astype(np.float64) / 2.0 ** 21).astype(np.float32)     # max |fq| in [2^21, 2^22): the row scale is 2^21
    filt = f.ravel()
    assert np.array_equal(oracle.quantise_filters(filt)[5], fq_row)
    du = (b0 + 256 * b1).reshape(121, 20).astype(np.int64)                   # Du[b][t], hashprint 0
    u = np.zeros((121, 100), np.int64)
    u[:, :20] = np.minimum(du, 0)
    u[:, 80:] = np.minimum(-du, 0)
    db = db_of(u)
    assert np.array_equal(oracle.quantise_db(db), u)                         # the spectrogram is reachable
    got = ref.digits(u[:, :20] - u[:, 80:])
    assert np.array_equal(got[0].ravel(), b0) and np.array_equal(got[1].ravel(), b1) and not got[2].any()
    d, dp, dl, lm, is_open = check(oracle, filt, db)
    return int(dl[5, 0]), int(lm[5])


def test_rows_driven_to_the_bound(oracle, filters):
    """Digits inside [-127, 127] reach 127/128 of the bound, one unit per digit inside it: for a row of the fixture
    filters, b1 = 127 sign(a0) and b0 = 127 sign(a0 + 256 a1) give |Dl| = 127 sum(|a0 + 256 a1| + 256 |a0|), which is
    127/128 Lmax_r where a0 and a1 agree in sign at every tap.  The bound itself is met with the digit -128, which the
    balanced split does produce: a row whose digits 0 and 1 have one sign, Du = -128 - 2^8 128 at every tap."""
    rng = np.random.default_rng(10)
    # (a) a row of the fixture filters, digits of Du of magnitude 127
    fq = oracle.quantise_filters(filters)[11].astype(np.int64)
    a0, a1, _ = ref.digits(fq)
    sg = lambda x: np.where(x >= 0, 1, -1)
    dl, lm = driven(oracle, fq, 127 * sg(a0 + 256 * a1), 127 * sg(a0))
    want = 127 * int((np.abs(a0 + 256 * a1) + 256 * np.abs(a0)).sum())
    assert dl == want and lm > 0 and want <= lm * 127 // 128
    # (b) one sign per row and digits of magnitude 127: exactly 127/128 of the bound
    m0, m1, m2 = rng.integers(0, 128, 2420), rng.integers(0, 128, 2420), rng.integers(0, 32, 2420)
    m2[3] = 40                                                               # the largest tap: 2^21 <= |fq| < 2^22
    row = m0 + 256 * m1 + 65536 * m2
    for sign in (1, -1):
        dl, lm = driven(oracle, sign * row, np.full(2420, 127 * sign), np.full(2420, 127 * sign))
        assert lm == 128 * int(m0.sum() + 256 * (m0.sum() + m1.sum())) and dl * 128 == lm * 127
        # (c) the digit -128 in both places: |Dl| = Lmax_r exactly
        dl, lm = driven(oracle, sign * row, np.full(2420, -128), np.full(2420, -128))
        assert abs(dl) == lm and lm > 0
    # (d) a row of one tap with S0 = 0, S1 > 0
    one = np.zeros(2420, np.int64)
    one[77] = 2 ** 21 + 256 * 90
    dl, lm = driven(oracle, one, np.full(2420, -128), np.full(2420, -128))
    assert lm == 128 * 256 * 90 and abs(dl) == lm
