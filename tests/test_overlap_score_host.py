"""CPU tests of the scored overlap search and of the timeline under the overlap rule: the new symbols
are declared and exported, every refusal happens before a device is touched, the two host-only functions against exact
arithmetic, the restated moments against a bit-by-bit loop, and the C++ facades compile and link."""
import ctypes
import inspect
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib

import overlap_ref
import overlap_score_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
SYMS = ("hpfw_gpu_search_overlap_scored_device", "hpfw_gpu_search_overlap_scored", "hpfw_gpu_overlap_rate", "hpfw_gpu_overlap_extent")


def test_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "hpfw_gpu.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym in SYMS:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTS and hasattr(hpfw_amd.lib(), sym)
    assert re.search(r"#define\s+HPFW_OVERLAP_RATE_BITS\s+10\b", header) and _lib.OVERLAP_RATE_BITS == ref.RATE_BITS == 10
    assert "no call is refused because a sum could wrap" in re.sub(r"\s*\n \*\s*", " ", text)
    for f in (_lib.Gpu.search_overlap_scored, _lib.Gpu.search_overlap_scored_dev):   # min_overlap has no default in the search
        assert inspect.signature(f).parameters["min_overlap"].default is inspect.Parameter.empty
    for f in (hpfw_amd.LiveSongIdentification.timeline, hpfw_amd.LiveSongIdentification.streams):   # None: the plain rule
        assert inspect.signature(f).parameters["min_overlap"].default is None
    facade = open(os.path.join(ROOT, "include", "hpfw", "gpu", "timeline.h")).read()
    assert re.search(r"int min_overlap = 0;", facade)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_bad_arguments_are_refused_without_a_device():
    """the handle here is a buffer of zeros: a call that got as far as using it would not return a status"""
    L = hpfw_amd.lib()
    buf = np.zeros(64, np.int64)
    one = _p(buf)
    off = np.array([0, 4, 8], np.int64)

    def both(h=one, q=one, q_off=off, n_q=2, ex=None, mo=2, k=1, out=one, stats=one):
        qo = None if q_off is None else _p(q_off)
        e = None if ex is None else _p(ex)
        rcs = []
        for rc in (L.hpfw_gpu_search_overlap_scored(h, q, qo, n_q, e, mo, k, out, stats),
                   L.hpfw_gpu_search_overlap_scored_device(h, q, qo, n_q, e, mo, k, out, stats, None)):
            rcs.append((rc, L.hpfw_gpu_last_error()))
        assert rcs[0][0] == rcs[1][0], rcs
        return rcs[0]

    for kw in (dict(h=None), dict(q_off=None), dict(out=None), dict(n_q=-1), dict(q=None)):
        assert both(**kw)[0] == E_INVALID, kw
    rc, msg = both(stats=None)
    assert rc == E_INVALID and b"null stats" in msg
    for k in (0, -1, 65):
        rc, msg = both(k=k)
        assert rc == E_INVALID and b"k must be in 1..64" in msg
    for mo in (0, -5, 16001):
        rc, msg = both(mo=mo)
        assert rc == E_INVALID and b"min_overlap" in msg
    rc, msg = both(q_off=np.array([0, 8, 4], np.int64))
    assert rc == E_INVALID and b"non-decreasing" in msg
    rc, msg = both(q_off=np.array([0, 4, 16005], np.int64))
    assert rc == E_UNSUPPORTED and b"16000" in msg
    rc, msg = both(ex=np.array([-1, -2], np.int32))
    assert rc == E_INVALID and b"exclude" in msg


def test_timeline_refusals_need_no_device():
    """min_overlap with shifts or tempos, and on a sharded identifier, is refused before the collector or a device is asked
    for anything: the identifier here has neither"""
    lsi = hpfw_amd.LiveSongIdentification.__new__(hpfw_amd.LiveSongIdentification)
    lsi._gpu = object()
    for kw in (dict(shifts=[0, 2]), dict(tempos=[1.0, 1.04]), dict(shifts=[0], tempos=[1.0])):
        for call in (lambda: lsi.timeline("x.wav", 10.0, min_overlap=100, **kw), lambda: lsi.streams(2, 10.0, min_overlap=100, **kw)):
            with pytest.raises(hpfw_amd.HpfwError) as e:
                call()
            assert e.value.status == _lib.E_UNSUPPORTED
    lsi._gpu = object.__new__(hpfw_amd.liveid._ShardedIndex)
    for call in (lambda: lsi.timeline("x.wav", 10.0, min_overlap=100), lambda: lsi.streams(2, 10.0, min_overlap=100),
                 lambda: lsi.top_overlap(["x.wav"], 1, 100)):
        with pytest.raises(hpfw_amd.HpfwError) as e:
            call()
        assert e.value.status == _lib.E_UNSUPPORTED


def test_overlap_rate_is_the_floor_of_the_fraction():
    n = 0
    for L in list(range(1, 41)) + [16000]:
        for dist in (range(0, 64 * L + 1) if L <= 40 else (0, 1, 64 * L - 1, 64 * L)):
            want = (Fraction(dist, L) * 1024).__floor__()
            assert _lib.overlap_rate(dist, L) == want == ref.rate(dist, L), (dist, L)
            n += 1
    assert n == sum(64 * L + 1 for L in range(1, 41)) + 4
    assert _lib.overlap_rate(64 * 16000, 16000) == 1 << 16
    out = ctypes.c_uint32()
    for dist, L in ((0, 0), (1, 16001), (65, 1), (64 * 40 + 1, 40)):
        assert hpfw_amd.lib().hpfw_gpu_overlap_rate(dist, L, ctypes.byref(out)) == E_INVALID, (dist, L)
    assert hpfw_amd.lib().hpfw_gpu_overlap_rate(1, 1, None) == E_INVALID


WIN, M, S = 220500, 1209, 100                              # 5 s: 403 columns (M = 1209), 304 hashprints of 100 columns


def test_overlap_extent():
    col = 3.0 * WIN / M
    # the hand cases: a 304 window on a song of 707 hashprints
    n, k = 707, 304
    assert _lib.overlap_extent(-121, n, k, S, WIN, M) == (int(121 * col + 0.5), WIN)      # begins 121 columns before the song
    assert _lib.overlap_extent(484, n, k, S, WIN, M) == (0, int((707 + 99 - 484) * col + 0.5))   # runs 81 columns past its end
    assert _lib.overlap_extent(0, n, k, S, WIN, M) == (0, WIN) == _lib.overlap_extent(n - k, n, k, S, WIN, M)   # inside: whole
    # (a column is 661500 / 1209 = 547.15 samples: 121 of them 66204.7, 322 of them 176181.1)
    assert _lib.overlap_extent(-121, n, k, S, WIN, M)[0] == 66205 and _lib.overlap_extent(484, n, k, S, WIN, M)[1] == 176181
    # the 143-hashprint item (242 columns) inside a window, from column 40
    assert _lib.overlap_extent(-40, 143, k, S, WIN, M) == (int(40 * col + 0.5), int(282 * col + 0.5))
    rng = np.random.default_rng(1801)
    for _ in range(2000):
        n, k = int(rng.integers(1, 3000)), int(rng.integers(1, 1200))
        d = int(rng.integers(-k + 1, n))                     # every lag with an overlap of at least one hashprint
        span = int(rng.integers(1, 200))
        m = int(rng.integers(3 * (k + span - 1) - 2, 3 * (k + span - 1) + 1))         # c = ceil(m / 3) = k + span - 1
        win = int(rng.integers(m, 400 * m))
        got = _lib.overlap_extent(d, n, k, span, win, m)
        assert got == ref.extent(d, n, k, span, win, m), (d, n, k, span, win, m)
        assert 0 <= got[0] < got[1] <= win
        if 0 <= d <= n - k:
            assert got == (0, win)
    a, b = ctypes.c_int64(), ctypes.c_int64()
    f = hpfw_amd.lib().hpfw_gpu_overlap_extent
    for args in ((304, 707, 0, S, WIN, M), (0, 0, 304, S, WIN, M), (0, 707, 304, 0, WIN, M), (0, 707, 304, S, 0, M), (0, 707, 304, S, WIN, 0),
                 (707, 707, 304, S, WIN, M), (-304, 707, 304, S, WIN, M)):
        assert f(*args, ctypes.byref(a), ctypes.byref(b)) == E_INVALID, args
    assert f(0, 707, 304, S, WIN, M, None, ctypes.byref(b)) == E_INVALID


def test_restated_moments_equal_a_bit_by_bit_loop():
    """a small ragged index: the moments over overlap_ref.clip_candidate's candidates against rates from the bit-by-bit
    candidates, with and without an excluded clip"""
    rng = np.random.default_rng(1802)
    lengths = [0, 1, 2, 3, 5, 8, 4, 7]
    clips = [rng.integers(0, 2 ** 64, n, dtype=np.uint64) for n in lengths]
    clips[6][:] = clips[5][2:6]                                  # (one clip is part of another)
    db_hp, db_off = _lib._ragged(clips, np.uint64)
    for k in (1, 3, 6):
        q = rng.integers(0, 2 ** 64, k, dtype=np.uint64)
        q[:min(k, 4)] = clips[5][1:1 + min(k, 4)]
        for mo in (1, 2, 4, 7):
            cands = ref.candidates(db_hp, db_off, q, mo)
            loop = [overlap_ref.loop_candidate(q, c, mo) if k >= mo and len(c) >= mo else None for c in clips]
            assert cands == loop == [overlap_ref.clip_candidate(q, c, mo) for c in clips]
            for ex in (-1, 5, 0):
                rates = [(d << 10) // L for c, cand in enumerate(loop) if cand is not None and c != ex for d, L, _ in [cand]]
                assert ref.row_moments(cands, ex) == (len(rates), sum(rates), sum(r * r for r in rates))
            assert ref.row_moments(cands)[0] == (sum(n >= mo for n in lengths) if k >= mo else 0)
            assert ref.row_moments(cands, 0) == ref.row_moments(cands)      # excluding a clip without a candidate changes nothing
            got = ref.search_scored(db_hp, db_off, q, mo)
            want = overlap_ref.search_overlap(db_hp, db_off, q, np.array([0, k]), 1, mo)[0, 0]
            if got[0] is None:
                assert want["clip"] == 0xFFFFFFFF
            else:
                assert (got[1], got[0], got[2], got[3]) == tuple(int(v) for v in want)


def test_tiny_reference_equals_the_restatement():
    rng = np.random.default_rng(1803)
    db = rng.integers(0, 4, (40, 8)).astype(np.uint64) * np.uint64(0x8000000000000001)     # few distinct words: ties abound
    db[20:] = rng.integers(0, 2 ** 64, (20, 8), dtype=np.uint64)
    queries = np.concatenate([db[3:4], rng.integers(0, 2 ** 64, (2, 8), dtype=np.uint64), db[[30]] ^ np.uint64(5)])
    for mo in (1, 4, 8):
        for q, row in zip(queries, ref.tiny_rows(db, queries, mo)):
            for c in range(40):
                assert (int(row[0][c]), int(row[1][c]), int(row[2][c])) == overlap_ref.clip_candidate(q, db[c], mo), (mo, c)
            db_hp, db_off = db.ravel(), np.arange(41) * 8
            want = overlap_ref.search_overlap(db_hp, db_off, q, np.array([0, 8]), 1, mo)[0, 0]
            assert ref.tiny_best(row) == tuple(int(v) for v in want)
            assert ref.tiny_moments(row) == ref.row_moments(ref.candidates(db_hp, db_off, q, mo))


FACADE = r"""
#include <hpfw/gpu/gpu_collector.h>
#include <hpfw/gpu/gpu_storage.h>
#include <hpfw/gpu/live_streams.h>
#include <hpfw/gpu/timeline.h>
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    hpfw::db::GpuStorage<hpfw::GpuCollector> storage;
    hpfw::GpuCollector::Hashprint hp(304, 0);
    auto hits = storage.find_overlap_scored(hp, 3, 100);
    hpfw::TimelineOptions opt;
    opt.min_score = 10;
    opt.min_overlap = 100;
    auto tl = hpfw::timeline(storage, storage.handle(), argv[1], opt);
    hpfw::LiveStreamsOptions lo;
    lo.min_score = 10;
    lo.min_overlap = 100;
    hpfw::LiveStreams<hpfw::db::GpuStorage<hpfw::GpuCollector>> live(storage, storage.handle(), 2, lo);
    auto segs = live.push({});
    auto rest = live.finish();
    return (int)(hits.size() + tl.segments.size() + tl.overlaps.size() + segs.size() + rest.size() + (live.open(0) ? 1 : 0)) +
           (hits.empty() ? 0 : (int)(hits[0].score + (double)hits[0].lag));
}
"""


def test_facades_compile_and_link(tmp_path):
    src = tmp_path / "overlap_timeline.cpp"
    src.write_text(FACADE)
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(tmp_path / "overlap_timeline"), "-L", lib_dir, "-lhpfw_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "overlap_timeline")], capture_output=True, text=True)   # no argument: no device touched
    assert r.returncode == 2
