"""CPU-side checks of the sample-accurate offsets: the numpy reference of the exact cross-correlation (tests/xcorr_ref.py)
against a plain Python loop, its peak rule and score, hpfw_amd.combiner.place (the spanning forest over pairwise offsets),
the segment rule of refine, and the job validation and split of hpfw_amd/csrc/xcorr_plan.h built alone with the address and
undefined-behaviour sanitizers."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from hpfw_amd import _lib
from hpfw_amd.combiner import Component, place, refine_geometry, xcorr_score

import xcorr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _loop(a, b, p, q, length, radius):
    get = lambda i: int(a[i]) if 0 <= i < len(a) else 0
    return [sum(get(p + l + n) * int(b[q + n]) for n in range(length)) for l in range(-radius, radius + 1)]


def test_reference_equals_the_loop():
    rng = np.random.default_rng(1)
    a = rng.integers(-32768, 32768, size=40).astype(np.int16)
    b = rng.integers(-32768, 32768, size=30).astype(np.int16)
    a[3], a[17], b[5], b[6] = -32768, 32767, -32768, -32768
    for p, q, length, radius in [(10, 0, 12, 4), (-3, 5, 20, 6), (30, 10, 20, 9), (60, 0, 5, 3), (-40, 2, 7, 2), (0, 29, 1, 0)]:
        got = xcorr_ref.xcorr(a, b, p, q, length, radius)
        assert got.dtype == np.int64 and got.tolist() == _loop(a, b, p, q, length, radius)
    assert not xcorr_ref.xcorr(a, b, 60, 0, 5, 3).any() and not xcorr_ref.xcorr(a, b, -40, 2, 7, 2).any()
    # the largest sums the limits allow are exact in int64: 2^22 products of 2^30
    big = np.full(1 << 22, -32768, np.int16)
    assert xcorr_ref.xcorr(big, big, 0, 0, 1 << 22, 0).tolist() == [1 << 52]


def test_peak_rule_and_score():
    assert xcorr_ref.peak_lag([1, -9, 3, 9, 0, 9, 2], 3) == 0          # |9| at -2, 0, 2: the smallest |lag|
    assert xcorr_ref.peak_lag([1, -9, 3, 0, 0, 9, 2], 3) == -2         # -2 and 2: the negative one
    assert xcorr_ref.peak_lag([9, 0, 0, 0, 0, -9, 0], 3) == 2          # |lag| 2 before 3, whatever the sign
    assert xcorr_ref.peak_lag([0, 0, 0], 1) == 0
    a = np.array([0, 3, -4, 0, 0], np.int16)
    assert xcorr_ref.peak(a, -a, 0, 0, 5, 2) == (0, -25, 25, 25)
    assert xcorr_ref.score(-25, 25, 25) == -1.0 and xcorr_score(-25, 25, 25) == -1.0
    assert xcorr_ref.score(5, 0, 25) == 0.0 and xcorr_score(5, 25, 0) == 0.0
    for r, ea, eb in [(12345678901234, 98765432109876, 55555555555555), (-(1 << 52), 1 << 52, (1 << 52) - 1), (7, 11, 13)]:
        assert xcorr_score(np.int64(r), np.int64(ea), np.int64(eb)) == xcorr_ref.score(r, ea, eb)


# ---- place -----------------------------------------------------------------------------------------------------------------
def test_place_a_chain():
    got = place(4, [(0, 1, 1000, 0.9, False), (1, 2, -2500, 0.8, False), (3, 2, 40, 0.7, False)])
    # start_1 = start_0 + 1000, start_2 = start_1 - 2500, start_2 = start_3 + 40
    assert got == [Component((0, 1, 2, 3), (1540, 2540, 40, 0), (False,) * 4, ())]


def test_place_a_cycle_with_one_inconsistent_edge():
    edges = [(0, 1, 100, 0.9, False), (1, 2, 200, 0.8, False), (2, 0, -310, 0.3, False)]      # the cycle closes 10 off
    got = place(3, edges)
    assert got == [Component((0, 1, 2), (0, 100, 300), (False,) * 3, ((2, 0, -10),))]
    # the same edge with the best score is a tree edge, and the weakest of the others reports the residual
    edges[2] = (2, 0, -310, 0.95, False)
    got = place(3, edges)
    assert got == [Component((0, 1, 2), (0, 100, 310), (False,) * 3, ((1, 2, -10),))]
    # a negative score counts by its magnitude
    edges[2] = (2, 0, -310, -0.95, True)
    assert place(3, edges)[0].residuals == ((1, 2, -10),)


def test_place_two_components_and_a_loner():
    got = place(6, [(4, 1, -50, 0.5, False), (0, 3, 7, 0.6, True), (3, 5, 1, 0.6, False)])
    assert got == [Component((0, 3, 5), (0, 7, 8), (False, True, True), ()),
                   Component((1, 4), (0, 50), (False, False), ()),
                   Component((2,), (0,), (False,), ())]
    assert place(0, []) == [] and place(2, []) == [Component((0,), (0,), (False,), ()), Component((1,), (0,), (False,), ())]


def test_place_polarity_through_two_inverted_edges():
    got = place(3, [(0, 1, 10, 0.9, True), (1, 2, 10, 0.9, True)])
    assert got == [Component((0, 1, 2), (0, 10, 20), (False, True, False), ())]
    # against the lowest id, whatever the tree's shape
    got = place(3, [(2, 1, 10, 0.9, True), (2, 0, 5, 0.9, False)])
    assert got == [Component((0, 1, 2), (5, 10, 0), (False, True, False), ())]


def test_place_does_not_depend_on_the_order_of_the_edges():
    edges = [(0, 1, 100, 0.9, False), (1, 2, 200, 0.8, True), (2, 0, -310, 0.3, True), (3, 4, 5, 0.8, False),
             (1, 0, -101, 0.8, False), (4, 3, -5, 0.8, False)]                              # equal scores among them
    want = place(6, edges)
    assert len(want) == 3 and sum(len(c.residuals) for c in want) == 3
    for perm in itertools.permutations(edges):
        assert place(6, list(perm)) == want


def test_place_rejects_bad_edges():
    for e in [(0, 0, 1, 0.5, False), (0, 3, 1, 0.5, False), (-1, 1, 1, 0.5, False), (0, 1, 1, float("nan"), False)]:
        with pytest.raises(ValueError):
            place(3, [e])


# ---- the segment rule ----------------------------------------------------------------------------------------------------
def test_refine_geometry():
    fq, fr = np.arange(5, 1005, dtype=np.int32), np.arange(0, 2000, dtype=np.int32)      # the query lost 5 leading frames
    # 900 query columns against 1900: d = -300 puts query column c on recording column c + 300
    d0, q, n = refine_geometry(900, 1900, fq, fr, 441 * 1000, 441 * 2000, -300, 1 << 15)
    o = (300 + 1200 - 1) // 2                                      # the middle of the overlap 300 .. 1199
    assert d0 == 441 * (5 + o - 300 - o) and n == 1 << 15 and q == 441 * o - (1 << 14)
    # a segment longer than the overlap is the overlap; a short one near an end is clamped into it
    d0, q, n = refine_geometry(900, 1900, fq, fr, 441 * 1000, 441 * 2000, -300, 1 << 22)
    assert (q, n) == (-d0, 441 * 1000) and q + n + d0 == 441 * 1000
    fr2 = np.arange(0, 50, dtype=np.int32)
    d0, q, n = refine_geometry(40, 50, np.arange(40, dtype=np.int32), fr2, 441 * 45, 441 * 50, 30, 20000)
    assert d0 == 441 * 30 and (q, n) == (0, 441 * 45 - 441 * 30)   # the recording's first samples, no more than overlap
    assert refine_geometry(40, 50, fq, fr2, 441 * 45, 441 * 50, 40, 1000) is None        # no column overlaps
    assert refine_geometry(40, 50, fq, fr2, 441 * 20, 441 * 50, 30, 1000) is None        # columns do, samples do not


# ---- the host side of the C entry points, alone ----------------------------------------------------------------------------
def test_dtypes_match_the_header():
    assert _lib.XCORR_JOB_DTYPE.itemsize == 64 and _lib.XCORR_PEAK_DTYPE.itemsize == 32
    assert {"hpfw_gpu_xcorr_pcm16", "hpfw_gpu_xcorr_pcm16_host", "hpfw_gpu_mel_kept_frames_pcm16_host"} <= set(_lib.EXPORTS)
    header = open(os.path.join(ROOT, "include", "hpfw_gpu.h")).read()
    for name in _lib.XCORR_JOB_DTYPE.names[:-1] + _lib.XCORR_PEAK_DTYPE.names[:-1]:
        assert name in header


def test_job_validation_and_split_under_sanitizers(tmp_path):
    """xcorr_plan.h is plain C++: every HPFW_E_INVALID case, the limits themselves, and the parts of the split (every lag of
    every sample exactly once, accumulators within int32) in a program of its own under ASan and UBSan"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "xcorr_plan_check"
    src = os.path.join(ROOT, "tests", "emu", "xcorr_plan_check.cpp")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "xcorr_plan_check ok" in r.stdout
