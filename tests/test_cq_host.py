"""The constant-Q stage without a GPU, at every chirp-z class the planner admits (tests/cq_ref.py): which classes the
sweep's clip lengths reach, the restated class rule against the oracle's, the length limit, the oracle's magnitudes
against float64 from the same forward bins, the smallest class any clip reaches, and the reciprocal by which the stage
addresses the rows layout of the forward bins."""
import time

import numpy as np
import pytest

import cols_ref
import cq_ref
import hpfw_amd

BAR = 1e-4                  # BASELINE.json north_star: |CQ| within 1e-4 of each band's maximum against float64

# (p, outer, len0) of every class above the LDS limit: frozen, so that a change of the peel rule shows as a diff here
BIG = ((24576, 1, 6144), (32768, 1, 8192), (49152, 2, 3072), (65536, 2, 4096), (98304, 2, 6144), (131072, 2, 8192),
       (196608, 3, 3072), (262144, 3, 4096), (393216, 3, 6144), (524288, 3, 8192))

# every clip length tests/test_gpu_parity.py runs: its clips of whole and fractional seconds, then the lengths it names
PARITY_LENGTHS = tuple(int(round(s * 44100)) for s in (2.0, 3.0, 4.0, 4.2, 5.0, 6.0, 7.0, 10.0, 12.5, 20.0, 30.0, 45.0, 49.0,
                                                       60.0, 100.0, 180.0)) + (
    1323000, 110250, 99225, 2646000, 1323001, 352799, 99991, 220499, 220500, 54254, 1764001, 132299, 88205, 132307, 7938001)

ROWS_LENGTH = 26460000      # 600 s: the rows-layout case of tests/test_gpu_cq_sweep.py


def test_lengths_reach_every_admitted_class():
    """23 classes: 2^8 .. 2^19 and 3 * 2^7 .. 3 * 2^17.  Above the LDS limit: outer = 1, 2, 3, every len0, and the
    8192-point block kernel under one, two and three global-memory passes."""
    reached, big = set(), set()
    for n in cq_ref.LENGTHS:
        for p, (outer, len0, bands) in cq_ref.classes(n).items():
            assert bands and (outer == 0) == (p <= cq_ref.LDS_MAX) and len0 * 4 ** outer == p
            reached.add(p)
            if outer:
                big.add((p, outer, len0))
    want = {p for a in range(7, 20) for p in (2 ** a, 3 * 2 ** a) if 256 <= p <= 2 ** 19}
    assert want == cq_ref.admitted() and len(want) == 23
    assert reached == want, sorted(want ^ reached)
    assert tuple(sorted(big)) == BIG
    assert {o for _, o, _ in big} == {1, 2, 3} and {l for _, _, l in big} == {3072, 4096, 6144, 8192}
    assert {o for _, o, l in big if l == 8192} == {1, 2, 3}
    # the rows-layout case: bins past 2^21 and an outer == 3 class
    assert cq_ref.extent(ROWS_LENGTH)[1] > 2 ** 21
    assert {p: v[:2] for p, v in cq_ref.classes(ROWS_LENGTH).items()} == {
        65536: (2, 4096), 98304: (2, 6144), 131072: (2, 8192), 196608: (3, 3072)}


@pytest.mark.parametrize("n", cq_ref.LENGTHS + (ROWS_LENGTH,) + PARITY_LENGTHS)
def test_classes_agree_with_the_oracle(oracle, n):
    plan = oracle.Plan(n)
    assert cq_ref.extent(n) == (plan.kmin, plan.kmax, plan.m, plan.c)
    posit, lg = cq_ref.geometry(n)
    assert np.array_equal(lg, plan.lg) and np.array_equal(posit - lg // 2, plan.start)
    psize = np.zeros(cq_ref.BINS, np.int64)
    for p, (_, _, bands) in cq_ref.classes(n).items():
        psize[bands] = p
    assert np.array_equal(psize, plan.psize)


def test_length_limit(oracle):
    """54 190 080 = 8064 x 6720 is the longest clip the sweep runs and the library takes it as it is; 55 125 000 =
    8750 x 6300 (1250 s) needs n1 > 8192 and is refused"""
    assert cols_ref.split(54190080) == (8064, 6720)
    assert hpfw_amd.supported_length(54190080) == 54190080
    assert cols_ref.split(55125000) == (8750, 6300)
    with pytest.raises(hpfw_amd.HpfwError):
        hpfw_amd.plan_checksum(55125000)
    assert hpfw_amd.supported_length(55125000) != 55125000
    # the oracle has no limit on n1 and accepts the length (its chirp-z classes still fit 2^19): not a defect, the
    # limit is the library's row layout (kernels.h XsView, n1 <= 2^13)
    assert max(cq_ref.classes(55125000)) == 2 ** 19
    assert oracle.Plan(55125000).n1 == 8750


@pytest.mark.parametrize("n", cq_ref.LENGTHS)
def test_oracle_against_float64_from_the_same_bins(oracle, n):
    """plan.cqmag on cq_ref.bins() against cq_ref.cq_from_bins, largest error over each band's maximum.  All 121 bands up
    to 240 s; at the two longest lengths the first and the last band of every class (the float64 side alone takes 6 and
    8 s for all bands there, on top of 5 to 6 s of the oracle's tables and magnitudes).  Measured, in the order of
    LENGTHS: 2.9e-7, 4.0e-7, 4.4e-7, 4.3e-7, 6.8e-7 over all bands; 2.4e-7 and 6.3e-7 over the sampled bands of the two
    longest (6.8e-7 and 6.3e-7 when all their bands are taken)."""
    t0 = time.time()
    plan = oracle.Plan(n)
    x = cq_ref.bins(n, plan.kmax - plan.kmin, n)
    got = plan.cqmag(x)
    bands = list(range(cq_ref.BINS)) if n <= 10584000 else cq_ref.first_and_last_bands(n)
    want = cq_ref.cq_from_bins(x[:, 0].astype(np.float64) + 1j * x[:, 1], plan.kmin, n, bands)
    assert want.shape == (len(bands), plan.c)
    err = float((np.abs(got[bands] - want).max(axis=1) / want.max(axis=1)).max())
    print(f"n = {n}: oracle against float64 {err:.3g} over {len(bands)} bands, {time.time() - t0:.1f} s")
    assert err < BAR, (n, err)


def test_no_clip_reaches_a_class_below_256():
    """the templates of launch_cq_class for p = 64, 96, 128, 192 are unreachable: the smallest window is 96 and the
    shortest clip with a hashprint has C = 100 columns, so every band needs at least 195 points.  Over every 7-smooth
    length in [54243, 2 x 54243] and the sweep's lengths, under the default conventions and all four switched."""
    for conv in (0, 15):
        smallest = {}
        for n in tuple(cols_ref.smooth_lengths(cols_ref.FIRST_LENGTH, 2 * cols_ref.FIRST_LENGTH)) + cq_ref.LENGTHS:
            _, lg = cq_ref.geometry(n, conv)
            assert lg.min() >= cq_ref.MIN_WINDOW
            smallest[n] = min(cq_ref.classes(n, conv))
        assert min(smallest.values()) == 256, (conv, min(smallest.items(), key=lambda kv: kv[1]))
    assert cq_ref.chirpz_length(cq_ref.MIN_WINDOW + 100 - 1) == 256


def test_rows_layout_reciprocal():
    """kernels.h XsView: q2 = (k magic) >> 40 with magic = ceil(2^40 / n1) is k / n1 while k e < 2^40, e = magic n1 -
    2^40 < n1: for every k < 2^27 at n1 <= 2^13.  The 64-bit product holds because k / n1 < n2 / 2 < 2^12.  Checked on
    every bin the stage reads at the sweep's 7-smooth lengths and the rows-layout case, and at the worst k (the last of
    a row, just below 2^27 and just below n / 2) of every n1 up to 2^13."""
    for n in cq_ref.LENGTHS[1:] + (ROWS_LENGTH,):
        n1, n2 = cols_ref.split(n)
        kmin, kmax = cq_ref.extent(n)[:2]
        magic = -(-(1 << 40) // n1)
        assert kmax <= n // 2 and kmax * magic < 1 << 64
        k = np.arange(kmin, kmax, dtype=np.uint64)
        assert np.array_equal((k * np.uint64(magic)) >> np.uint64(40), k // np.uint64(n1)), n
    for n1 in range(2, 8193):
        magic = -(-(1 << 40) // n1)
        assert 0 <= magic * n1 - (1 << 40) < n1
        for top in (1 << 27, n1 * cols_ref.N2_MAX // 2):
            for k in (top // n1 * n1 - 1, top - 1):
                assert (k * magic) >> 40 == k // n1, (n1, k)
        assert (n1 * cols_ref.N2_MAX // 2) * magic < 1 << 64
