"""S15's chirp-z forward transform without a GPU, at every class of its kernels' shapes (tests/bz_ref.py): the frozen list
of lengths, the library's own statement of the shape (hpfw_amd.plan_bz_shape, what plans.hip and k_bluestein.hip's launches
read) against the plain restatement, the classes the list must hold as conditions on those shapes, and the oracle's
forward bins against float64 (tests/test_gpu_bz_sweep.py then holds the kernels to the oracle bit for bit)."""
import pytest

import bz_ref
import cq_ref
import hpfw_amd

# first length of a = 1 .. 17, 32, 33; the exact fits of a = 1, 4, 16; the first length of every class of the last stage up to
# a = 59; the first lengths with 16, 32, 48 consumed rows (17, 33, 49 open a class): frozen, so that a change of the planner's
# rule shows as a diff here and not as silently different coverage
SWEEP = (
    54255, 92039, 184119, 276199, 368281, 460361, 552441, 644515, 736589, 828661, 920735, 1012809, 1104881, 1196955, 1289029,
    1381101, 1473175, 2854275, 2946349,
    92037, 368279, 1473174,
    1032157, 2025615, 2064301, 2117689, 2578055, 3160955, 3222567, 3314641, 4193099, 4235373, 4603667, 5289763, 5340253,
    967649, 1999795, 3096447)
# (step, n_blocks odd, nt2, tile groups, tiles of zeros) of the last stage: every combination a clip with a <= 59 can meet
CLASSES = {
    (14, 0, 1, 1, 0), (15, 0, 1, 1, 0), (16, 0, 1, 1, 0), (14, 0, 2, 1, 0), (15, 0, 2, 1, 0), (16, 0, 2, 1, 0), (16, 1, 2, 1, 0),
    (14, 0, 3, 1, 0), (16, 0, 3, 1, 0), (16, 1, 3, 1, 0), (14, 0, 3, 2, 2), (15, 0, 3, 2, 2), (16, 0, 3, 2, 2),
    (14, 0, 3, 2, 1), (16, 0, 3, 2, 1), (16, 1, 3, 2, 1), (14, 0, 3, 2, 0), (16, 0, 3, 2, 0)}

# Forward bins against np.fft.rfft(clip / 32768) in float64, largest error over the clip's own max |ref|.  The oracle alone
# over the whole sweep, both clip kinds, measured 1.77e-6 at worst (n = 4603667, a = 51, the noise clip), growing with the length
# from 3e-7 at a = 1; the bar is twice that, rounded up to one digit.
FLOAT64_BAR = 4e-6


def test_sweep_is_the_frozen_list():
    assert bz_ref.sweep_lengths() == SWEEP
    assert len(set(SWEEP)) == len(SWEEP)
    assert cq_ref.extent(bz_ref.SHORTEST)[3] - 99 == 1 and cq_ref.extent(bz_ref.SHORTEST - 1)[3] - 99 == 0
    for n in SWEEP:
        assert not bz_ref.is_smooth(n) and n >= bz_ref.SHORTEST
    kmin, kmax = bz_ref.extents(SWEEP)                     # the array form the search for the classes uses
    assert [cq_ref.extent(n)[:2] for n in SWEEP] == list(zip(kmin.tolist(), kmax.tolist()))


def test_sweep_holds_every_class():
    """conditions on the shapes, not measurements"""
    shapes = {n: bz_ref.shape(n) for n in SWEEP}
    # first stage: every a up to one past a full tile of 16 outputs, and the next tile's edge; every a % 4 (prefetch depth)
    for a in bz_ref.A_FIRSTS:
        n = bz_ref.first_length(a)
        assert n in SWEEP and n % 2 == 1 and shapes[n].a == a, (a, n)
        before = n - 2                                                  # the odd length with a prime factor above 7 before it
        while bz_ref.is_smooth(before):
            before -= 2
        assert before < bz_ref.SHORTEST if a == 1 else bz_ref.a_of(before) == a - 1, (a, n, before)
        assert bz_ref.shape(bz_ref.last_length(a)).a == a and bz_ref.a_of(bz_ref.last_length(a) + 1) == a + 1
    assert bz_ref.A_FIRSTS == tuple(range(1, 18)) + (32, 33)
    # the tables: slack 0 at a = 1, 4 and 16
    for a in (1, 4, 16):
        assert any(s.a == a and s.slack == 0 for s in shapes.values()), a
    assert [n for n, s in shapes.items() if s.slack == 0] == [bz_ref.last_length(a) for a in bz_ref.A_EXACT]
    # last stage: every class that occurs up to a = 59 (a search over every odd length there, bz_ref.class_firsts)
    by_class, by_k1n = bz_ref.class_firsts()
    assert set(by_class) == CLASSES
    swept = {bz_ref.last_stage_class(s) for s in shapes.values() if s.a <= bz_ref.A_CLASSES}
    assert swept == CLASSES
    assert any(c[1] == 1 and c[3] == 2 for c in swept)                  # an odd count of register sets with two tile groups
    assert {c[4] for c in swept if c[3] == 2} == {0, 1, 2}              # the second group with 0, 1, 2 tiles of zeros
    assert max(n for n in SWEEP) < 5400000
    # consumed rows that fill a row tile exactly or leave one live row in the next
    assert {16, 17, 32, 33, 48, 49} <= {s.k1n for s in shapes.values()}
    assert all(by_k1n[k] in SWEEP for k in (16, 17, 32, 33, 48, 49))


def test_no_smooth_length_fits_exactly():
    """the forced chirp-z transform of a 7-smooth length (tests/test_gpu_bz_sweep.py) runs at the least slack there is"""
    n, slack = bz_ref.forced_smooth_length()
    assert (n, slack) == (91875, 178) and bz_ref.is_smooth(n)
    s = bz_ref.shape(n)
    assert s._asdict() == {k: v for k, v in hpfw_amd.plan_bz_shape(n, force_bluestein=True).items() if k in s._fields}
    with pytest.raises(hpfw_amd.HpfwError):
        hpfw_amd.plan_bz_shape(n)                                       # unforced it takes the mixed-radix transform


@pytest.mark.parametrize("n", SWEEP)
def test_shape_and_oracle_against_float64(oracle, n):
    s = bz_ref.shape(n)
    t = hpfw_amd.plan_bz_shape(n)                                       # the library's planner: the same shape
    assert s._asdict() == {k: t[k] for k in s._fields}
    kmin, kmax, _, _ = cq_ref.extent(n)
    assert (t["n2"], t["n_tiles1"], t["kmin"], t["kmax"]) == (bz_ref.N2, (s.a + 15) // 16, kmin, kmax)
    assert s.L >= n + (kmax - kmin) - 1 > s.L - 16 * bz_ref.N2           # the smallest n1 = 16 a that fits
    plan = oracle.Plan(n)
    assert (plan.n1, plan.n2, plan.kmin, plan.kmax) == (s.n1, bz_ref.N2, kmin, kmax)
    for kind, clip in (("noise", bz_ref.noise_clip(n)), ("rail", bz_ref.rail_clip(n))):
        err = bz_ref.float64_error(plan.spectrum(clip), clip, kmin, kmax)
        print(f"n = {n}, a = {s.a}, {kind}: {err:.3g}")
        assert err < FLOAT64_BAR, (n, kind, err)
