"""CPU tests of the live feeds: the entry points are declared and exported, bad arguments are refused
before any device is touched, and the incremental segmenter against hpfw_gpu_timeline_segments byte for byte: random window
lists cut into pushes at random, and the closing rule case by case."""
import ctypes
import os
import re

import numpy as np

import hpfw_amd
from hpfw_amd import _lib

from test_timeline_host import _as_rows, _random_windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
SYMS = ("hpfw_gpu_streams_create", "hpfw_gpu_streams_destroy", "hpfw_gpu_streams_push", "hpfw_gpu_streams_push_device",
        "hpfw_gpu_streams_room", "hpfw_gpu_streams_extract", "hpfw_gpu_streams_extract_host", "hpfw_gpu_streams_reset",
        "hpfw_gpu_streams_info", "hpfw_gpu_timeline_tracker_create", "hpfw_gpu_timeline_tracker_destroy",
        "hpfw_gpu_timeline_tracker_push", "hpfw_gpu_timeline_tracker_pop", "hpfw_gpu_timeline_tracker_open",
        "hpfw_gpu_timeline_tracker_finish")
WIN, HOP = 220500, 110250


def test_entry_points_are_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hpfw_gpu.h")).read(), flags=re.S)
    for sym in SYMS:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTS and hasattr(hpfw_amd.lib(), sym)
    for name in ("hpfw_streams_params", "hpfw_stream_window", "hpfw_streams_info"):
        assert re.search(r"\}\s*" + name + r"\s*;", header), name
    assert ctypes.sizeof(_lib.StreamsParams) == 56 and ctypes.sizeof(_lib.StreamsInfo) == 40
    assert _lib.STREAM_WINDOW_DTYPE.itemsize == 16


def _create(h=None, n_streams=3, win=WIN, hop=HOP, capacity=0, tempos=None, shifts=None, n_tempos=None, n_shifts=None):
    t = None if tempos is None else np.ascontiguousarray(tempos, np.float32)
    sh = None if shifts is None else np.ascontiguousarray(shifts, np.int32)
    p = _lib.StreamsParams(n_streams, (0 if t is None else t.size) if n_tempos is None else n_tempos,
                           (0 if sh is None else sh.size) if n_shifts is None else n_shifts, 0, win, hop, capacity,
                           None if t is None else _lib._hp(t), None if sh is None else _lib._hp(sh))
    out = ctypes.c_void_p()
    rc = hpfw_amd.lib().hpfw_gpu_streams_create(h, ctypes.byref(p), ctypes.byref(out))
    assert out.value is None
    return rc, hpfw_amd.lib().hpfw_gpu_last_error()


def test_null_and_bad_arguments_are_refused_without_a_device():
    L = hpfw_amd.lib()
    one = np.zeros(8, np.int64).ctypes.data_as(ctypes.c_void_p)
    n = ctypes.c_int64()
    # a set that does not exist
    assert L.hpfw_gpu_streams_push(None, one, one, ctypes.byref(n)) == E_INVALID
    assert L.hpfw_gpu_streams_push_device(None, one, one, ctypes.byref(n), None) == E_INVALID
    assert L.hpfw_gpu_streams_room(None, one) == E_INVALID
    assert L.hpfw_gpu_streams_extract(None, 1, one, None, one, ctypes.byref(n), None) == E_INVALID
    assert L.hpfw_gpu_streams_extract_host(None, 1, one, None, one, ctypes.byref(n)) == E_INVALID
    assert L.hpfw_gpu_streams_reset(None, 0) == E_INVALID
    assert L.hpfw_gpu_streams_info(None, None, one, one) == E_INVALID
    L.hpfw_gpu_streams_destroy(None)
    p = _lib.StreamsParams(3, 0, 0, 0, WIN, HOP, 0, None, None)
    out = ctypes.c_void_p()
    assert L.hpfw_gpu_streams_create(None, None, ctypes.byref(out)) == E_INVALID
    assert L.hpfw_gpu_streams_create(None, ctypes.byref(p), None) == E_INVALID
    # the set's own parameters, then the lists with their messages, then the handle
    for n_streams in (0, -1, 4097):
        rc, msg = _create(n_streams=n_streams)
        assert rc == E_INVALID and b"n_streams" in msg
    for win, hop in ((WIN, WIN + 1), (WIN, 0), (1000, 500), (0, 0)):          # hop > win, no hop, unsupported lengths
        rc, msg = _create(win=win, hop=hop)
        assert rc == E_INVALID and b"windows" in msg, (win, hop)
    for capacity in (WIN - 1, 1, -5):
        rc, msg = _create(capacity=capacity)
        assert rc == E_INVALID and b"capacity" in msg
    for bad in ([], [1.0] * 65, [float("nan")], [0.49], [2.01], [1.0, 1.0000001]):
        rc, msg = _create(tempos=bad)
        assert rc == E_INVALID and b"tempos" in msg, bad
    for bad in ([2, 2], [121], list(range(65))):
        rc, msg = _create(shifts=bad)
        assert rc == E_INVALID and b"shifts" in msg, bad
    assert _create(n_shifts=2)[0] == E_INVALID and _create(n_tempos=2)[0] == E_INVALID      # counts without lists
    for kw in (dict(), dict(shifts=[-2, 0, 2]), dict(tempos=[0.96, 1.0, 1.04]), dict(tempos=[0.96, 1.0, 1.04], shifts=[-2, 0, 2]),
               dict(capacity=WIN), dict(n_streams=4096)):
        rc, msg = _create(**kw)
        assert rc == E_INVALID and b"null handle" in msg, kw
    # tracker
    assert L.hpfw_gpu_timeline_tracker_create(None, ctypes.byref(out)) == E_INVALID
    tp = _lib.TimelineParams(10.0, 201.5, 0.0, WIN, HOP, -1, 0)
    assert L.hpfw_gpu_timeline_tracker_create(ctypes.byref(tp), None) == E_INVALID
    for kw in (dict(min_score=0.0), dict(min_score=float("nan")), dict(hop_cols=0.0), dict(hop_cols=float("inf")), dict(tol_cols=-1.0),
               dict(hop=0), dict(hop=WIN + 1), dict(max_gap=-2), dict(min_windows=-1)):
        args = dict(min_score=10.0, hop_cols=201.5, tol_cols=0.0, win=WIN, hop=HOP, max_gap=-1, min_windows=0)
        args.update(kw)
        bad = _lib.TimelineParams(*args.values())
        assert L.hpfw_gpu_timeline_tracker_create(ctypes.byref(bad), ctypes.byref(out)) == E_INVALID and out.value is None, kw
        assert b"timeline" in L.hpfw_gpu_last_error()
    assert L.hpfw_gpu_timeline_tracker_push(None, one, 1) == E_INVALID
    assert L.hpfw_gpu_timeline_tracker_pop(None, one, 1, ctypes.byref(n)) == E_INVALID
    assert L.hpfw_gpu_timeline_tracker_open(None, one, ctypes.byref(ctypes.c_int())) == E_INVALID
    assert L.hpfw_gpu_timeline_tracker_finish(None) == E_INVALID
    L.hpfw_gpu_timeline_tracker_destroy(None)
    t = _lib.TimelineTracker(10.0, 201.5, WIN, HOP)
    try:
        assert L.hpfw_gpu_timeline_tracker_push(t._t, None, 1) == E_INVALID
        assert L.hpfw_gpu_timeline_tracker_pop(t._t, None, 1, ctypes.byref(n)) == E_INVALID
        assert L.hpfw_gpu_timeline_tracker_pop(t._t, one, 1, None) == E_INVALID
    finally:
        t.close()


def _cut_at_random(rng, n):
    """a partition of range(n) into pushes: empty pushes, one window per push, and runs"""
    cuts, at = [], 0
    while at < n:
        r = rng.random()
        step = 0 if r < 0.15 else 1 if r < 0.5 else int(rng.integers(1, 12))
        cuts.append((at, min(at + step, n)))
        at = min(at + step, n)
    cuts.append((n, n))
    return cuts


def test_tracker_equals_the_offline_segments_on_random_lists():
    """300 window lists as tests/test_timeline_host.py draws them, each cut into pushes at random: what was popped along the
    way plus what finish() releases is hpfw_gpu_timeline_segments' output byte for byte, and a segment is popped neither
    before nor after the push that holds its closing window"""
    rng = np.random.default_rng(91)
    kept = early = 0
    for trial in range(300):
        windows, hop_cols = _random_windows(rng)
        rows = _as_rows(windows)
        assert (rows["pad"] == 0).all()
        min_score = float(rng.choice([10.0, 5.0, 12.5]))
        tol = None if trial % 3 else float(rng.choice([2.0, 0.5, 16.0]))
        max_gap, min_windows = int(rng.choice([0, 1, 3])), int(rng.choice([1, 2]))
        want = _lib.timeline_segments(rows, min_score, hop_cols, WIN, HOP, tol, max_gap, min_windows)
        t = _lib.TimelineTracker(min_score, hop_cols, WIN, HOP, tol, max_gap, min_windows)
        try:
            got = []
            for a, b in _cut_at_random(rng, len(windows)):
                t.push(rows[a:b])
                new = t.pop() if trial % 2 else t.pop(1)                       # (a small cap only delays)
                for sg in new:
                    # closed by window `closer`, which this push holds: the first strong window behind it (one that did not
                    # continue it) or window last + max_gap + 1, whichever comes first
                    strong = [w for w in range(int(sg["last"]) + 1, len(windows))
                              if windows[w][0] is not None and windows[w][4] >= min_score]
                    closer = min(strong[:1] + [int(sg["last"]) + max_gap + 1])
                    assert closer < b and (trial % 2 == 0 or a <= closer), (trial, sg, a, b)
                got.extend(new)
            early += len(got)
            t.finish()
            got.extend(t.pop())
            assert t.open() is None and t.pop().size == 0
        finally:
            t.close()
        got = np.array(got, _lib.SEGMENT_DTYPE)
        assert got.tobytes() == want.tobytes(), (trial, got, want)
        kept += len(want)
    assert kept > 300 and early > kept // 2


def _rows(windows):
    return _as_rows(windows)


def test_tracker_hand_written_cases():
    hc = 201.5
    weak = (4, 0, 0, 1.0, 3.0)
    song = lambda w, score=30.0, clip=3, o=100: (clip, int(round(o + hc * w)), 0, 1.0, score)

    def ranges(segs):
        return [(int(s["clip"]), int(s["first"]), int(s["last"]), int(s["n_strong"])) for s in segs]

    # poppable exactly at the push that holds window l + max_gap + 1, not one window earlier
    for max_gap in (0, 1, 3):
        t = _lib.TimelineTracker(10.0, hc, WIN, HOP, max_gap=max_gap)
        t.push(_rows([song(0), song(1)]))                                       # l = 1
        for w in range(2, 2 + max_gap):
            t.push(_rows([weak]))
            assert t.pop().size == 0 and ranges([t.open()]) == [(3, 0, 1, 2)], (max_gap, w)
        t.push(_rows([weak]))                                                   # window l + max_gap + 1
        assert ranges(t.pop()) == [(3, 0, 1, 2)] and t.open() is None, max_gap
        t.close()
    # ... and that window continues the segment when it can
    t = _lib.TimelineTracker(10.0, hc, WIN, HOP, max_gap=1)
    t.push(_rows([song(0), weak, song(2)]))
    assert t.pop().size == 0 and ranges([t.open()]) == [(3, 0, 2, 2)]
    # at once on a strong window of another clip, or of the same clip at an inconsistent offset
    t.push(_rows([song(3, clip=5)]))
    assert ranges(t.pop()) == [(3, 0, 2, 2)] and ranges([t.open()]) == [(5, 3, 3, 1)]
    t.push(_rows([song(4, clip=5, o=700)]))
    assert ranges(t.pop()) == [(5, 3, 3, 1)] and ranges([t.open()]) == [(5, 4, 4, 1)]
    t.finish()
    assert ranges(t.pop()) == [(5, 4, 4, 1)] and t.open() is None
    # the numbering goes on after finish()
    t.push(_rows([song(5)]))
    assert ranges([t.open()]) == [(3, 5, 5, 1)] and int(t.open()["start"]) == 5 * HOP
    t.close()
    # pop with cap = 1 loses nothing
    t = _lib.TimelineTracker(10.0, hc, WIN, HOP, max_gap=0)
    t.push(_rows([song(w, clip=w) for w in range(5)]))
    assert [ranges(t.pop(1)) for _ in range(5)] == [[(w, w, w, 1)] for w in range(4)] + [[]]
    assert t.pop(0).size == 0
    t.finish()
    assert ranges(t.pop(1)) == [(4, 4, 4, 1)] and t.pop(1).size == 0
    t.close()
    # open() shows a lone strong window under min_windows = 2; the segment is then dropped
    t = _lib.TimelineTracker(10.0, hc, WIN, HOP, max_gap=1, min_windows=2)
    t.push(_rows([weak, song(1)]))
    assert ranges([t.open()]) == [(3, 1, 1, 1)]
    t.push(_rows([weak, weak]))
    assert t.open() is None and t.pop().size == 0
    t.push(_rows([song(4), song(5)]))
    t.finish()
    assert ranges(t.pop()) == [(3, 4, 5, 2)]
    t.close()


FACADE = r"""
#include <hpfw/gpu/gpu_collector.h>
#include <hpfw/gpu/gpu_storage.h>
#include <hpfw/gpu/sharded_storage.h>
#include <hpfw/gpu/live_streams.h>
template <typename Storage>
int run(const Storage &storage, hpfw_gpu *h)
{
    hpfw::LiveStreamsOptions opt;
    opt.min_score = 10.0;
    opt.tempos = {0.96f, 1.0f, 1.04f};
    opt.shifts = {-2, 0, 2};
    opt.keep_windows = true;
    hpfw::LiveStreams<Storage> live(storage, h, 2, opt);
    std::vector<int16_t> a(22050), b;
    auto closed = live.push({{0, a.data(), (int64_t)a.size()}, {1, b.data(), 0}});
    auto now = live.open(0);
    for (auto &c : live.finish()) closed.push_back(c);
    live.reset(1);
    return (int)closed.size() + (now ? 1 : 0) + (int)live.windows().size();
}
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    hpfw_gpu *h = nullptr;
    if (hpfw_gpu_create(0, &h) != 0) return 1;
    int n;
    if (argv[1][0] == 's') {
        hpfw::db::ShardedGpuStorage<hpfw::GpuCollector> storage(std::vector<int>{0, 0});
        n = run(storage, h);
    } else {
        hpfw::db::GpuStorage<hpfw::GpuCollector> storage;
        n = run(storage, h);
    }
    hpfw_gpu_destroy(h);
    return n;
}
"""


def test_live_streams_facade_compiles_and_links(tmp_path):
    import subprocess
    src = tmp_path / "live_streams.cpp"
    src.write_text(FACADE)
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(tmp_path / "live_streams"), "-L", lib_dir, "-lhpfw_gpu_multi", "-lhpfw_gpu", "-Wl,-rpath," + lib_dir,
           "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "live_streams")], capture_output=True, text=True)   # no argument: no device touched
    assert r.returncode == 2
