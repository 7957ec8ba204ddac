"""CPU tests of the timeline of a long recording: the entry points are declared and exported, bad
arguments are refused before any device is touched, the window count at its edges, and the two host-only functions -- the
score of a hit and the segments -- against the restatements of tests/timeline_ref.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib

import timeline_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
SYMS = ("hpfw_gpu_search_topk_scored_device", "hpfw_gpu_search_topk_scored", "hpfw_gpu_search_topk_transposed_scored_device",
        "hpfw_gpu_search_topk_transposed_scored", "hpfw_gpu_hit_score", "hpfw_gpu_window_count", "hpfw_gpu_extract_windows_pcm16",
        "hpfw_gpu_extract_windows_pcm16_host", "hpfw_gpu_timeline_segments")
WIN, HOP = 220500, 110250


def test_entry_points_are_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hpfw_gpu.h")).read(), flags=re.S)
    for sym in SYMS:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTS and hasattr(hpfw_amd.lib(), sym)
    for name, dtype in (("hpfw_dist_stats", _lib.STATS_DTYPE), ("hpfw_window_hit", _lib.WINDOW_HIT_DTYPE),
                        ("hpfw_segment", _lib.SEGMENT_DTYPE)):
        assert re.search(r"\}\s*" + name + r"\s*;", header), name
    assert _lib.STATS_DTYPE.itemsize == 24 and _lib.WINDOW_HIT_DTYPE.itemsize == 32 and _lib.SEGMENT_DTYPE.itemsize == 80
    assert ctypes.sizeof(_lib.TimelineParams) == 48 and ctypes.sizeof(_lib.DistStats) == 24


def _arr(vals, dtype):
    a = np.ascontiguousarray(vals, dtype)
    return a, a.ctypes.data_as(ctypes.c_void_p), a.size


def test_null_and_bad_arguments_are_refused_without_a_device():
    L = hpfw_amd.lib()
    one = np.zeros(4, np.int64).ctypes.data_as(ctypes.c_void_p)
    # scored searches: null handle, null stats
    assert L.hpfw_gpu_search_topk_scored(None, one, one, 1, 1, one, one) == E_INVALID
    assert L.hpfw_gpu_search_topk_scored_device(None, one, one, 1, 1, one, one, None) == E_INVALID
    assert L.hpfw_gpu_search_topk_transposed_scored(None, one, one, 1, 1, 1, one, one) == E_INVALID
    assert L.hpfw_gpu_search_topk_transposed_scored_device(None, one, one, 1, 1, 1, one, one, None) == E_INVALID
    for rc in (L.hpfw_gpu_search_topk_scored(one, one, one, 1, 1, one, None),
               L.hpfw_gpu_search_topk_scored_device(one, one, one, 1, 1, one, None, None),
               L.hpfw_gpu_search_topk_transposed_scored(one, one, one, 1, 1, 1, one, None),
               L.hpfw_gpu_search_topk_transposed_scored_device(one, one, one, 1, 1, 1, one, None, None)):
        assert rc == E_INVALID and b"null stats" in L.hpfw_gpu_last_error()

    # windows: the variant's own list checks first, with its messages, then the handle
    def calls(tp, nt, sp, ns, win=WIN, hop=HOP):
        return (L.hpfw_gpu_extract_windows_pcm16(None, None, 10 * WIN, win, hop, tp, nt, sp, ns, None, None),
                L.hpfw_gpu_extract_windows_pcm16_host(None, None, 10 * WIN, win, hop, tp, nt, sp, ns, None))
    for bad in ([], [1.0] * 65, [float("nan")], [0.49], [2.01], [1.0, 1.0000001]):
        keep, tp, nt = _arr(bad, np.float32)
        for rc in calls(tp, nt, None, 0):
            assert rc == E_INVALID and b"tempos" in L.hpfw_gpu_last_error(), bad
    for bad in ([2, 2], [121], list(range(65))):
        keep, sp, ns = _arr(bad, np.int32)
        for rc in calls(None, 0, sp, ns):
            assert rc == E_INVALID and b"shifts" in L.hpfw_gpu_last_error(), bad
    for rc in calls(None, 0, None, 2) + calls(None, 2, None, 0):
        assert rc == E_INVALID
    keep, tp, nt = _arr([0.96, 1.0, 1.04], np.float32)
    keep_s, sp, ns = _arr([-2, 0, 2], np.int32)
    for args in ((None, 0, None, 0), (None, 0, sp, ns), (tp, nt, None, 0), (tp, nt, sp, ns)):
        for rc in calls(*args):
            assert rc == E_INVALID and b"null handle" in L.hpfw_gpu_last_error(), args


def test_window_count_edges():
    L = hpfw_amd.lib()
    n = ctypes.c_int64(-7)
    for n_total, win, hop, want in ((0, WIN, HOP, 0), (WIN - 1, WIN, HOP, 0), (WIN, WIN, HOP, 1), (WIN + HOP - 1, WIN, HOP, 1),
                                    (WIN + HOP, WIN, HOP, 2), (10 * WIN, WIN, WIN, 10), (10 * WIN - 1, WIN, WIN, 9),
                                    (WIN + 5, WIN, 1, 6), (3 * 220493 + 44101, 220493, 44101, 11),
                                    (20 * 60 * 44100, WIN, HOP, 479), (4630500, WIN, HOP, 41)):
        assert L.hpfw_gpu_window_count(n_total, win, hop, ctypes.byref(n)) == 0 and n.value == want, (n_total, win, hop)
        assert _lib.window_count(n_total, win, hop) == want == ref.windows_of(np.zeros(0, np.int16), win, hop).shape[0] + want
    for n_total, win, hop in ((-1, WIN, HOP), (WIN, WIN, 0), (WIN, WIN, -3), (WIN, WIN, WIN + 1), (WIN, 1000, 500),
                              (WIN, 0, 0), (WIN, 44100 * 1700, 44100)):
        assert L.hpfw_gpu_window_count(n_total, win, hop, ctypes.byref(n)) == E_INVALID, (n_total, win, hop)
        assert b"windows" in L.hpfw_gpu_last_error()
    assert L.hpfw_gpu_window_count(WIN, WIN, HOP, None) == E_INVALID
    with pytest.raises(hpfw_amd.HpfwError):
        _lib.window_count(WIN, WIN, 0)


def _score(d, counted, n, s, ss):
    st = np.zeros((), _lib.STATS_DTYPE)
    st["n"], st["sum"], st["sum_sq"] = n, s, ss
    return _lib.hit_score(d, counted, st)


def _close(a, b):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12 * abs(b)


def test_hit_score_equals_the_restatement():
    rng = np.random.default_rng(31)
    for trial in range(400):
        n = int(rng.integers(3, 60)) if trial % 4 else int(rng.integers(3, 30000))
        kq = int(rng.choice([1, 60, 304, 16000]))
        d = rng.integers(0, 64 * kq + 1, n)
        if trial % 5 == 0:
            d = np.minimum(d, 64 * kq - rng.integers(0, 50, n))              # crowded near the top of the range
        hit = int(d.min())
        mom = ref.row_moments(d, [True] * n)
        want = ref.hit_score(hit, True, *mom)
        assert _close(_score(hit, True, *mom), want), (trial, mom)
        other = int(d[rng.integers(0, n)])                                   # any counted clip may be scored, not only the best
        assert _close(_score(other, True, *mom), ref.hit_score(other, True, *mom)), (trial, mom)
    # the cases without a score
    assert math.isnan(_score(5, False, 10, 500, 30000))                      # the hit's clip is not counted
    assert math.isnan(_score(5, True, 2, 15, 125)) and math.isnan(_score(0, True, 0, 0, 0))   # n < 3
    assert math.isnan(_score(7, True, 3, 7 + 20 + 20, 49 + 800))             # the others agree: var == 0
    assert math.isnan(ref.hit_score(7, True, 3, 47, 849)) and math.isnan(ref.hit_score(5, True, 2, 15, 125))
    assert not math.isnan(_score(7, True, 3, 7 + 20 + 21, 49 + 400 + 441))
    # a hand case: d = 10 against {40, 50, 60}: mean 50, variance 200 / 3
    assert _close(_score(10, True, 4, 160, 100 + 1600 + 2500 + 3600), 40 / math.sqrt(200 / 3))
    # moments near 2^63: 1.9e9 clips at the largest distance but a few (the sum of squares just below 2^63)
    big = 64 * 16000
    for spread in (1, 1000, 123457):
        n = (2 ** 63 - 1) // big ** 2 - spread
        ds = [big] * 3 + [big - spread, big - 2 * spread, 0]
        s = big * (n - len(ds)) + sum(ds)
        ss = big * big * (n - len(ds)) + sum(x * x for x in ds)
        assert 2 ** 62 < ss < 2 ** 63
        for hit in (0, big - 2 * spread):
            assert _close(_score(hit, True, n, s, ss), ref.hit_score(hit, True, n, s, ss)), (spread, hit)
    # moments no set of distances has
    L = hpfw_amd.lib()
    out = ctypes.c_double()
    for d, n, s, ss in ((10, 3, 5, 100), (10, 3, 50, 99), (1, 3, 3, 1 + 1 + 1 - 1 + 1000000), (1, 5, 2 ** 64 - 1, 2 ** 64 - 1)):
        st = _lib.DistStats(s, ss, n, 0)
        if (d, n, s) == (1, 3, 3):
            continue                                                          # (var > 0: a legal, if odd, row)
        assert L.hpfw_gpu_hit_score(d, 1, ctypes.byref(st), ctypes.byref(out)) == E_INVALID, (d, n, s, ss)
    st = _lib.DistStats(30, 200, 4, 0)                                       # sum^2 > n sum_sq: a negative variance
    assert L.hpfw_gpu_hit_score(1, 1, ctypes.byref(st), ctypes.byref(out)) == E_INVALID
    assert L.hpfw_gpu_hit_score(1, 1, None, ctypes.byref(out)) == E_INVALID
    assert L.hpfw_gpu_hit_score(1, 1, ctypes.byref(st), None) == E_INVALID


def _as_rows(windows):
    rows = np.zeros(len(windows), _lib.WINDOW_HIT_DTYPE)
    for i, (clip, off, variant, tempo, score) in enumerate(windows):
        rows[i] = (ref.NONE if clip is None else clip, off, variant, 0, tempo, score)
    return rows


def _same(got, want):
    assert len(got) == len(want), (got, want)
    for g, w in zip(got, want):
        for key, val in w.items():
            assert g[key] == val, (key, g, w)


def _random_windows(rng):
    """a window list with runs of one clip whose offsets advance by about tempo x hop, broken by noise, other clips, NaN
    scores, gaps and jumps"""
    n_w = int(rng.integers(0, 60))
    hop_cols = float(rng.choice([201.5, 80.6, 403.0, 17.25]))
    out, w = [], 0
    while len(out) < n_w:
        clip = int(rng.integers(0, 6))
        tempo = float(rng.choice([1.0, 1.0, 0.96, 1.04, 0.92]))
        o = int(rng.integers(0, 2000))
        for i in range(int(rng.integers(1, 9))):
            r = rng.random()
            off = int(round(o + tempo * hop_cols * i + rng.normal(0, 0.35 * max(2.0, 0.08 * hop_cols))))
            score = float(rng.choice([3.0, 8.0, 9.99, 10.0, 12.5, 30.0, 55.0]))
            if r < 0.10:
                out.append((None, 0, 0, 1.0, float("nan")))
            elif r < 0.18:
                out.append((clip, off, int(rng.integers(0, 9)), tempo, float("nan")))
            elif r < 0.26:
                out.append((clip, off + int(rng.integers(100, 900)), 0, tempo, score))      # a jump to a repeated section
            elif r < 0.32:
                out.append((int(rng.integers(0, 6)), int(rng.integers(0, 2000)), 0, 1.0, score))
            else:
                out.append((clip, off, int(rng.integers(0, 9)), tempo, score))
    return out[:n_w], hop_cols


def test_segments_equal_the_restatement_on_random_lists():
    rng = np.random.default_rng(77)
    kept = 0
    for trial in range(300):
        windows, hop_cols = _random_windows(rng)
        min_score = float(rng.choice([10.0, 5.0, 12.5]))
        tol = None if trial % 3 else float(rng.choice([2.0, 0.5, 16.0]))
        max_gap, min_windows = int(rng.integers(0, 4)), int(rng.integers(1, 4))
        want = ref.segments(windows, min_score, hop_cols, WIN, HOP, tol, max_gap, min_windows)
        got = _lib.timeline_segments(_as_rows(windows), min_score, hop_cols, WIN, HOP, tol, max_gap, min_windows)
        _same(got, want)
        kept += len(want)
        for s in want:                                                          # what every segment must satisfy
            assert s["n_strong"] >= min_windows and s["first"] <= s["best_window"] <= s["last"]
            assert s["start"] == s["first"] * HOP and s["end"] == s["last"] * HOP + WIN
    assert kept > 300


def test_segments_hand_written_cases():
    hc = 201.5

    def run(windows, **kw):
        want = ref.segments(windows, 10.0, hc, WIN, HOP, **kw)
        _same(_lib.timeline_segments(_as_rows(windows), 10.0, hc, WIN, HOP, **kw), want)
        return [(s["clip"], s["first"], s["last"], s["n_strong"]) for s in want]

    weak = (4, 0, 0, 1.0, 3.0)
    song = lambda w, score=30.0, clip=3, o=100: (clip, int(round(o + hc * w)), 0, 1.0, score)
    # a gap of exactly max_gap windows is bridged, one more splits
    assert run([song(0), song(1), weak, song(3)]) == [(3, 0, 3, 3)]
    assert run([song(0), song(1), weak, weak, song(4)]) == [(3, 0, 1, 2), (3, 4, 4, 1)]
    assert run([song(0), weak, weak, song(3)], max_gap=2) == [(3, 0, 3, 2)]
    assert run([song(0), weak, weak, weak, song(4)], max_gap=2) == [(3, 0, 0, 1), (3, 4, 4, 1)]
    assert run([song(0), song(1)], max_gap=0) == [(3, 0, 1, 2)] and run([song(0), weak, song(2)], max_gap=0) == [(3, 0, 0, 1), (3, 2, 2, 1)]
    # the same clip at an inconsistent offset splits; a consistent one within the tolerance does not
    assert run([song(0), song(1), song(2, o=700), song(3, o=700)]) == [(3, 0, 1, 2), (3, 2, 3, 2)]
    assert run([song(0), song(1, o=110), song(2, o=95)]) == [(3, 0, 2, 3)]
    assert run([song(0), song(1, o=110)], tol_cols=2.0) == [(3, 0, 0, 1), (3, 1, 1, 1)]
    assert run([song(0), weak, song(2, o=125)]) == [(3, 0, 2, 2)]              # the tolerance grows with the distance ...
    assert run([song(0), song(1, o=125)]) == [(3, 0, 0, 1), (3, 1, 1, 1)]      # ... 25 columns over one hop are too many
    # another clip closes the segment; min_windows = 2 drops a lone window
    assert run([song(0), song(1), song(2, clip=5), song(3)]) == [(3, 0, 1, 2), (5, 2, 2, 1), (3, 3, 3, 1)]
    assert run([song(0), song(1), song(2, clip=5), song(3)], min_windows=2) == [(3, 0, 1, 2)]
    assert run([weak, song(1), weak, weak], min_windows=2) == []
    # NaN and scores below the threshold are never strong; exactly the threshold is
    assert run([song(0, float("nan")), song(1, 9.999), song(2, 10.0)]) == [(3, 2, 2, 1)]
    assert run([(None, 0, 0, 1.0, 99.0), song(1)]) == [(3, 1, 1, 1)]
    assert run([]) == []
    # the tempo of the last accepted window sets the expected advance; the best window is the earliest of the highest score
    fast = [(2, int(round(50 + 1.04 * hc * w)), 7, 1.04, s) for w, s in enumerate((20.0, 41.0, 41.0, 25.0))]
    got = _lib.timeline_segments(_as_rows(fast), 10.0, hc, WIN, HOP)
    assert len(got) == 1 and (got[0]["best_window"], got[0]["best_score"], got[0]["best_tempo"], got[0]["best_variant"]) == (1, 41.0, 1.04, 7)
    assert got[0]["first_offset"] == 50 and got[0]["best_offset"] == fast[1][1] and (got[0]["start"], got[0]["end"]) == (0, 3 * HOP + WIN)
    assert run([(2, int(round(50 + 1.04 * hc * w)), 0, 1.0, 30.0) for w in range(4)], tol_cols=2.0) == [(2, w, w, 1) for w in range(4)]


def test_segments_refuse_bad_parameters():
    L = hpfw_amd.lib()
    rows = _as_rows([(3, 100, 0, 1.0, 30.0)])
    out = np.zeros(4, _lib.SEGMENT_DTYPE)
    n = ctypes.c_int64()

    def call(min_score=10.0, hop_cols=201.5, tol=0.0, win=WIN, hop=HOP, max_gap=-1, min_windows=0, w=rows, cap=4, o=out, pn=n):
        p = _lib.TimelineParams(min_score, hop_cols, tol, win, hop, max_gap, min_windows)
        return L.hpfw_gpu_timeline_segments(None if w is None else _lib._hp(w), 0 if w is None else w.size, ctypes.byref(p),
                                            None if o is None else _lib._hp(o), cap, None if pn is None else ctypes.byref(pn))
    assert call() == 0 and n.value == 1 and out[0]["clip"] == 3                 # the defaults: tol 0, max_gap -1, min_windows 0
    assert call(w=None) == 0 and n.value == 0
    assert call(cap=0, o=None) == 0 and n.value == 1                            # counting only
    for kw in (dict(min_score=0.0), dict(min_score=-1.0), dict(min_score=float("nan")), dict(hop_cols=0.0),
               dict(hop_cols=float("inf")), dict(hop_cols=float("nan")), dict(tol=-1.0), dict(tol=float("nan")), dict(hop=0),
               dict(hop=WIN + 1), dict(max_gap=-2), dict(min_windows=-1), dict(pn=None), dict(o=None)):
        assert call(**kw) == E_INVALID, kw
    assert L.hpfw_gpu_timeline_segments(_lib._hp(rows), 1, None, _lib._hp(out), 4, ctypes.byref(n)) == E_INVALID
    with pytest.raises(hpfw_amd.HpfwError):
        _lib.timeline_segments(rows, 0.0, 201.5, WIN, HOP)
    with pytest.raises(ValueError):
        _lib.timeline_segments(rows, 10.0, 201.5, WIN, HOP, tol_cols=0.0)


FACADE = r"""
#include <hpfw/gpu/gpu_collector.h>
#include <hpfw/gpu/gpu_storage.h>
#include <hpfw/gpu/timeline.h>
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    hpfw::db::GpuStorage<hpfw::GpuCollector> storage;
    hpfw_gpu *h = nullptr;
    if (hpfw_gpu_create(0, &h) != 0) return 1;
    hpfw::TimelineOptions opt;
    opt.min_score = 10.0;
    opt.tempos = {0.96f, 1.0f, 1.04f};
    opt.shifts = {-2, 0, 2};
    auto t = hpfw::timeline(storage, h, argv[1], opt);
    hpfw_gpu_destroy(h);
    return t.segments.empty() ? 0 : (int)t.segments[0].clip;
}
"""


def test_timeline_facade_compiles_and_links(tmp_path):
    import subprocess
    src = tmp_path / "timeline.cpp"
    src.write_text(FACADE)
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(tmp_path / "timeline"), "-L", lib_dir, "-lhpfw_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "timeline")], capture_output=True, text=True)   # no argument: no device touched
    assert r.returncode == 2
