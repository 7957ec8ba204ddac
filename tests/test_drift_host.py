"""CPU tests of clock drift between recorders: the time map's bound in exact rationals, the Theil-Sen
line against a numpy restatement, the anchors of a pair, the affine placement against place(), the WAV writer, and the host
logic under the sanitizers in a program of its own.  The library loads without a device; nothing here touches one."""
import ctypes
import itertools
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib
from hpfw_amd.combiner import Component, WarpedComponent, place, place_affine

import warp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_IO = -1, -6


# ---- the time map -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (0.0, 1e-6, -1e-6, 3e-4, -3e-4, 9.7e-4, -9.7e-4))
def test_time_map_holds_the_derived_bound(B):
    """|i0 + m + (f0 + m d) 2^-40 - (m - A) / (1 + B)| <= 2^-40 + m 2^-41, in exact rationals of the float64 arguments"""
    for A in (0.0, 0.5, -0.25, 1234.5678, -98765.4321, 3969000.75, -3969000.1, 1.5e8 + 0.3, -1.5e8 - 0.7):
        i0, f0, d = _lib.time_map_q40(A, B)
        assert 0 <= f0 < 1 << 40 and abs(d) <= 1 << 30
        for m in (0, 1, 1 << 20, (1 << 31) - 1):
            err, bound = ref.time_map_error(A, B, i0, f0, d, m)
            assert err <= bound, (A, B, m, float(err), float(bound))
        # against the exact rounding: d equal, the start within one unit of 2^-40
        ri0, rf0, rd = ref.time_map_q40(A, B)
        assert d == rd and abs((i0 << 40) + f0 - ((ri0 << 40) + rf0)) <= 1, (A, B)


def test_time_map_special_values_and_limits():
    assert _lib.time_map_q40(0.0, 0.0) == (0, 0, 0) and _lib.time_map_q40(-3.0, 0.0) == (3, 0, 0) and _lib.time_map_q40(2.5, 0.0) == (-3, 1 << 39, 0)
    # a source at 100 ppm fast (B = 1e-4) is read 100 ppm slower: d < 0
    assert _lib.time_map_q40(0.0, 1e-4)[2] == round((Fraction(1) / (1 + Fraction(1e-4)) - 1) * (1 << 40))
    for bad in ((0.0, 0.000979), (0.0, -0.000977), (0.0, 0.5), (0.0, -1.0), (0.0, float("nan")), (float("nan"), 0.0), (float("inf"), 0.0),
                (2.0 ** 30 + 1, 0.0), (-2.0 ** 30 - 1, 0.0)):
        with pytest.raises(hpfw_amd.HpfwError) as e:
            _lib.time_map_q40(*bad)
        assert e.value.status == E_INVALID, bad
    assert _lib.time_map_q40(2.0 ** 30, 0.0) == (-(1 << 30), 0, 0)
    assert abs(_lib.time_map_q40(0.0, 0.000977)[2]) < 1 << 30 and abs(_lib.time_map_q40(0.0, -0.000975)[2]) < 1 << 30
    i0 = ctypes.c_int64()
    assert hpfw_amd.lib().hpfw_gpu_time_map_q40(0.0, 0.0, None, ctypes.byref(i0), ctypes.byref(i0)) == E_INVALID


# ---- Theil-Sen ----------------------------------------------------------------------------------------------------------------
def _theil_sen(n, lag):
    """the numpy restatement: float64, pairs in index order, the median of an even count the mean of the two middle values"""
    n, lag = np.asarray(n, np.int64), np.asarray(lag, np.int64)
    if n.size == 0:
        return 0.0, 0.0, 0.0
    slopes = [np.float64(lag[j] - lag[i]) / np.float64(n[j] - n[i]) for i in range(n.size) for j in range(i + 1, n.size) if n[i] != n[j]]
    if n.size < 3 or not slopes:
        a, b = np.float64(lag[0]), np.float64(0.0)
    else:
        b = np.median(np.array(slopes, np.float64))
        a = np.median(lag.astype(np.float64) - b * n.astype(np.float64))
    e = lag.astype(np.float64) - (a + b * n.astype(np.float64))
    ss = np.float64(0.0)
    for v in e:
        ss = ss + v * v
    return float(a), float(b), float(np.sqrt(ss / np.float64(n.size)))


def _line(rng, count, a, b):
    n = np.sort(rng.choice(np.arange(0, 4_000_000, 1000), count, replace=False)) + 32768
    n = np.concatenate([n[count // 2:count // 2 + 1], n[:count // 2], n[count // 2 + 1:]])       # the centre first
    return n, a + b * n


def test_fit_equals_the_restatement_digit_for_digit():
    rng = np.random.default_rng(5)
    for count in (3, 4, 5, 12, 13, 40):
        for a, b in ((100.0, 0.0), (-5000.25, 3e-4), (77.5, -9.7e-4), (0.0, 6e-5)):
            n, exact = _line(rng, count, a, b)
            for lag in (np.rint(exact), np.floor(exact), np.rint(exact) + rng.integers(-1, 2, count)):
                lag = lag.astype(np.int64)
                assert _lib.drift_fit(n, lag) == _theil_sen(n, lag)


def _majority_separation(n):
    """the largest L such that more than half of the pairs of positions n are at least L apart.  If every lag is within e of
    a line, a pair's slope is within 2 e / (n_j - n_i) of the line's; more than half of the slopes are then within 2 e / L,
    and so is their median (and the mean of the two middle values of an even count)"""
    sep = np.sort(np.abs(n[:, None] - n[None, :])[np.triu_indices(n.size, 1)])[::-1]
    return float(sep[sep.size // 2])


def test_fit_on_exact_rounded_and_wild_lines():
    rng = np.random.default_rng(6)
    for count in (6, 13, 30):
        for a, b in ((250.0, 4e-4), (-8000.0, -6.5e-4), (3.0, 0.0)):
            n, exact = _line(rng, count, a, b)
            L = _majority_separation(n)
            ga, gb, rms = _lib.drift_fit(n, np.rint(exact).astype(np.int64))       # every lag within 1/2 of the line
            assert abs(gb - b) <= 1.0 / L and rms <= 1.0, (count, a, b, gb)
            noisy = (np.rint(exact) + rng.integers(-1, 2, count)).astype(np.int64)   # within 3/2
            ga, gb, rms = _lib.drift_fit(n, noisy)
            assert abs(gb - b) <= 3.0 / L and rms <= 2.5, (count, a, b, gb)
            # a third of the points wild, alternately far above and far below the line: their slopes fall on both sides of
            # the clean ones in equal numbers, and the median stays among the slopes of the clean pairs that are far apart
            wild = noisy.copy()
            bad = np.sort(rng.choice(count, count // 3, replace=False))
            wild[bad] += (5000 + 7 * rng.integers(0, 1000, bad.size)) * np.where(np.arange(bad.size) % 2, -1, 1)
            keep = np.setdiff1d(np.arange(count), bad)
            wa, wb, wrms = _lib.drift_fit(n, wild)
            assert abs(wb - b) <= 3.0 / _majority_separation(n[keep]), (count, a, b, wb)
            assert wrms > 100
    # an exact line comes back exactly
    n = np.array([40000, 10000, 20000, 30000, 50000])
    assert _lib.drift_fit(n, n // 1000 + 7) == (7.0, 0.001, 0.0)


def test_fit_on_0_1_and_2_points_and_bad_arguments():
    assert _lib.drift_fit([], []) == (0.0, 0.0, 0.0)
    assert _lib.drift_fit([500], [42]) == (42.0, 0.0, 0.0)
    a, b, rms = _lib.drift_fit([500, 900], [42, 46])
    assert (a, b) == (42.0, 0.0) and rms == np.sqrt(8.0)
    assert _lib.drift_fit([7, 7, 7], [1, 2, 3])[:2] == (1.0, 0.0)                   # three points, no two positions apart
    L = hpfw_amd.lib()
    x = np.zeros(3, np.int64)
    p, d = x.ctypes.data_as(ctypes.c_void_p), ctypes.c_double()
    assert L.hpfw_gpu_drift_fit(p, p, -1, ctypes.byref(d), ctypes.byref(d), ctypes.byref(d)) == E_INVALID
    assert L.hpfw_gpu_drift_fit(None, p, 3, ctypes.byref(d), ctypes.byref(d), ctypes.byref(d)) == E_INVALID
    assert L.hpfw_gpu_drift_fit(p, p, 3, None, ctypes.byref(d), ctypes.byref(d)) == E_INVALID
    assert L.hpfw_gpu_drift_fit(p, p, (1 << 14) + 1, ctypes.byref(d), ctypes.byref(d), ctypes.byref(d)) == E_INVALID
    with pytest.raises(ValueError):
        _lib.drift_fit([1, 2], [1])


# ---- anchors ------------------------------------------------------------------------------------------------------------------
def test_anchors():
    # an overlap shorter than one anchor and of exactly one anchor: the centre segment alone
    assert _lib.drift_anchors(100, 600, 100, 500, 1000, 300) == (100, [], [])
    assert _lib.drift_anchors(100, 1100, 100, 1000, 1000, 300) == (100, [], [])
    # ragged ends: whole anchors only, going outward
    assert _lib.drift_anchors(7, 3056, 857, 1000, 1000, 300) == (857, [557, 257], [1157, 1457, 1757])
    assert _lib.drift_anchors(7, 3057, 857, 1000, 1000, 300)[2] == [1157, 1457, 1757, 2057]
    assert _lib.drift_anchors(257, 3056, 857, 1000, 1000, 300)[1] == [557, 257] and _lib.drift_anchors(258, 3056, 857, 1000, 1000, 300)[1] == [557]
    # the defaults on a 20 minute overlap: 2^16 samples every 2^21
    n = 20 * 60 * 44100
    c, left, right = _lib.drift_anchors(0, n, n // 2 - (1 << 15), 1 << 16, 1 << 16, 1 << 21)
    assert len(left) == len(right) == 12 and left[-1] >= 0 and right[-1] + (1 << 16) <= n and np.all(np.diff([c] + right) == 1 << 21)
    for bad in ((0, 10000, 4500, 1001, 1000, 1000), (0, 10000, 9500, 1000, 1000, 1000), (50, 10000, 49, 1000, 1000, 1000),
                (0, 10000, 4500, 0, 1000, 1000), (0, 10000, 4500, 1000, 1000, 0), (-1, 10000, 4500, 1000, 1000, 1000)):
        with pytest.raises(hpfw_amd.HpfwError) as e:
            _lib.drift_anchors(*bad)
        assert e.value.status == E_INVALID, bad


# ---- placement ----------------------------------------------------------------------------------------------------------------
PLACE_CASES = [
    (4, [(0, 1, 1000, 0.9, False), (1, 2, -2500, 0.8, False), (3, 2, 40, 0.7, False)]),
    (3, [(0, 1, 100, 0.9, False), (1, 2, 200, 0.8, False), (2, 0, -310, 0.3, False)]),
    (3, [(0, 1, 100, 0.9, False), (1, 2, 200, 0.8, False), (2, 0, -310, -0.95, True)]),
    (6, [(4, 1, -50, 0.5, False), (0, 3, 7, 0.6, True), (3, 5, 1, 0.6, False)]),
    (3, [(2, 1, 10, 0.9, True), (2, 0, 5, 0.9, False)]),
    (6, [(0, 1, 100, 0.9, False), (1, 2, 200, 0.8, True), (2, 0, -310, 0.3, True), (3, 4, 5, 0.8, False), (1, 0, -101, 0.8, False),
         (4, 3, -5, 0.8, False)]),
    (2, []), (0, []),
]


def _with_drift(edges, drift=0.0):
    return [(i, j, off, drift, sc, inv) for i, j, off, sc, inv in edges]


@pytest.mark.parametrize("n_rec, edges", PLACE_CASES)
def test_place_affine_without_drift_is_place(n_rec, edges):
    want, got = place(n_rec, edges), place_affine(n_rec, _with_drift(edges))
    assert len(got) == len(want)
    for w, g in zip(want, got):
        assert isinstance(w, Component) and isinstance(g, WarpedComponent)
        assert g.members == w.members and g.starts == w.starts and g.inverted == w.inverted and g.rates == (1.0,) * len(w.members)
        assert [r[:3] for r in g.residuals] == list(w.residuals) and all(r[3] == 0.0 for r in g.residuals)


def test_place_affine_composes_a_chain_of_three():
    """recording k's sample n at A_k + R_k n of a common clock: the edges are the exact maps between neighbours"""
    A, R = (5000.0, 0.0, 12000.5), (1.0, 1.0004, 0.99975)
    edge = lambda i, j, sc, inv: (i, j, (A[j] - A[i]) / R[i], R[j] / R[i] - 1.0, sc, inv)    # noqa: E731
    for edges in ([edge(0, 1, 0.9, True), edge(1, 2, 0.8, True)], [edge(1, 0, 0.9, True), edge(2, 1, 0.8, True)],
                  [edge(2, 0, 0.9, False), edge(1, 2, 0.8, True)]):
        (c,) = place_affine(3, edges)
        assert c.members == (0, 1, 2) and c.inverted == (False, True, False) and c.residuals == ()
        assert np.allclose(c.rates, [r / R[0] for r in R], rtol=0, atol=1e-15)
        assert np.allclose(c.starts, [(a - min(A)) / R[0] for a in A], rtol=0, atol=1e-8)
    # a third edge, 2 samples and 1 ppm off the others, is the weakest: it reports just that at the centre of its overlap
    off, dr = (A[2] - A[0]) / R[0], R[2] / R[0] - 1.0
    lengths = (100000, 100000, 100000)
    (c,) = place_affine(3, [edge(0, 1, 0.9, True), edge(1, 2, 0.8, True), (0, 2, off + 2.0, dr + 1e-6, 0.5, False)], lengths)
    (i, j, res, ppm), = c.residuals
    centre = (0.0 + min(100000.0, (100000 - (off + 2.0)) / (1.0 + dr + 1e-6))) / 2
    assert (i, j) == (0, 2) and abs(ppm - 1.0) < 1e-6 and abs(res - (2.0 + 1e-6 * centre)) < 1e-6


def test_place_affine_does_not_depend_on_the_order_of_the_edges():
    edges = [(0, 1, 100.5, 1e-4, 0.9, False), (1, 2, 200.25, -2e-4, 0.8, True), (2, 0, -310.0, 1e-4, 0.3, True), (3, 4, 5.0, 0.0, 0.8, False),
             (1, 0, -101.0, -1e-4, 0.8, False), (4, 3, -5.0, 3e-5, 0.8, False)]
    want = place_affine(6, edges, [50000] * 6)
    assert len(want) == 3 and sum(len(c.residuals) for c in want) == 3
    for perm in itertools.permutations(edges):
        assert place_affine(6, list(perm), [50000] * 6) == want


def test_place_affine_rejects_bad_edges():
    for e in [(0, 0, 1, 0.0, 0.5, False), (0, 3, 1, 0.0, 0.5, False), (0, 1, 1, 0.0, float("nan"), False), (0, 1, float("nan"), 0.0, 0.5, False),
              (0, 1, 1, 0.5, 0.5, False), (0, 1, 1, float("nan"), 0.5, False)]:
        with pytest.raises(ValueError):
            place_affine(3, [e])


# ---- the WAV writer -----------------------------------------------------------------------------------------------------------
def test_wav_writer(tmp_path):
    x = np.random.default_rng(8).integers(-32768, 32768, 1001).astype(np.int16)
    p = str(tmp_path / "m.wav")
    _lib.wav_write(p, x)
    raw = open(p, "rb").read()
    assert len(raw) == 44 + 2002 and raw[:4] == b"RIFF" and raw[8:16] == b"WAVEfmt " and raw[36:40] == b"data"
    assert np.array_equal(_lib.wav_read(p), x)
    from hpfw_amd import synth
    synth.write_wav(str(tmp_path / "s.wav"), x)
    assert open(str(tmp_path / "s.wav"), "rb").read() == raw                     # the project's Python writer, byte for byte
    _lib.wav_write(str(tmp_path / "st.wav"), x[:1000], channels=2)
    assert _lib.wav_read(str(tmp_path / "st.wav")).size == 500
    for args in ((x, 2), (x, 3)):
        with pytest.raises(hpfw_amd.HpfwError) as e:
            _lib.wav_write(p, *args)
        assert e.value.status == E_INVALID
    with pytest.raises(hpfw_amd.HpfwError) as e:
        _lib.wav_write(str(tmp_path / "no" / "dir.wav"), x)
    assert e.value.status == E_IO
    assert hpfw_amd.lib().hpfw_gpu_wav_write_pcm16(None, None, 0, 1) == E_INVALID


# ---- the host logic under the sanitizers --------------------------------------------------------------------------------------
def test_drift_plan_and_wav_writer_under_sanitizers(tmp_path):
    """drift_plan.h and wav_file.cpp are plain C++: every refusal, the reach of a track against a scan, the anchors, the
    line, the time map and a file written and read back, in a program of its own under ASan and UBSan"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "drift_plan_check"
    srcs = [os.path.join(ROOT, "tests", "emu", "drift_plan_check.cpp"), os.path.join(ROOT, "hpfw_amd", "csrc", "wav_file.cpp")]
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *srcs, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = tmp_path / "files"
    out.mkdir()
    r = subprocess.run([str(exe), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "drift_plan_check ok" in r.stdout
