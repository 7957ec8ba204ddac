"""CPU tests of the warped search: the entry points are declared and exported, every refusal happens
before a device is touched, and the restatement of tests/dtw_ref.py against an exhaustive enumeration of the admissible
paths, against the plain search, and on the planted case."""
import ctypes
import inspect
import itertools
import os
import re

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib

import dtw_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
SYMS = ("hpfw_gpu_dtw_pairs_device", "hpfw_gpu_dtw_pairs", "hpfw_gpu_search_dtw_device", "hpfw_gpu_search_dtw",
        "hpfw_gpu_dtw_path_device", "hpfw_gpu_dtw_path", "hpfw_gpu_dtw_geometry")


def test_entry_points_are_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hpfw_gpu.h")).read(), flags=re.S)
    for sym in SYMS:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTS and hasattr(hpfw_amd.lib(), sym)
    assert re.search(r"\}\s*hpfw_dtw_hit\s*;", header)
    assert _lib.DTW_HIT_DTYPE.itemsize == 16 and _lib.DTW_HIT_DTYPE == ref.DTW_HIT_DTYPE and hpfw_amd.DTW_HIT_DTYPE is _lib.DTW_HIT_DTYPE
    assert _lib.DTW_HIT_DTYPE.names == ("dist", "clip", "start", "end")
    assert _lib.DTW_MAX_PATH_CELLS == ref.MAX_PATH_CELLS == 1 << 31
    # candidates has no default in any binding
    for f in (_lib.Gpu.search_dtw, _lib.Gpu.search_dtw_dev, hpfw_amd.LiveSongIdentification.top_warped):
        assert inspect.signature(f).parameters["candidates"].default is inspect.Parameter.empty
    for name in ("dtw_pairs", "dtw_pairs_dev", "dtw_path", "dtw_path_dev"):
        assert callable(getattr(_lib.Gpu, name))
    assert callable(hpfw_amd.LiveSongIdentification.warp_path) and callable(hpfw_amd.LiveSongIdentification.columns_to_seconds)
    facade = open(os.path.join(ROOT, "include", "hpfw", "gpu", "gpu_storage.h")).read()
    assert re.search(r"find_warped\(const typename Collector::Hashprint &hp, int k, int candidates\)", facade)
    assert re.search(r"warp_path\(const typename Collector::Hashprint &hp, size_t clip\)", facade)
    makefile = open(os.path.join(ROOT, "hpfw_amd", "csrc", "Makefile")).read()
    assert " k_dtw.hip " in makefile and " dtw.hip " in makefile
    strip, block = ctypes.c_int32(0), ctypes.c_int32(0)
    assert hpfw_amd.lib().hpfw_gpu_dtw_geometry(ctypes.byref(strip), ctypes.byref(block)) == 0
    assert strip.value >= 2 and block.value == 64 * strip.value
    assert (_lib.DTW_STRIP, _lib.DTW_BLOCK) == (strip.value, block.value)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_bad_arguments_are_refused_without_a_device():
    """the handle here is a buffer of zeros: a call that got as far as using it would not return a status"""
    L = hpfw_amd.lib()
    buf = np.zeros(64, np.int64)
    one = _p(buf)
    off = np.array([0, 4, 8], np.int64)
    two_pairs = np.array([[0, 0], [1, 0]], np.int32)

    def pairs(h=one, q=one, q_off=off, n_q=2, pr=two_pairs, n_pairs=2, out=one):
        qo = None if q_off is None else _p(q_off)
        pp = None if pr is None else _p(pr)
        a = (L.hpfw_gpu_dtw_pairs(h, q, qo, n_q, pp, n_pairs, out), L.hpfw_gpu_last_error())
        b = (L.hpfw_gpu_dtw_pairs_device(h, q, qo, n_q, pp, n_pairs, out, None), L.hpfw_gpu_last_error())
        assert a[0] == b[0], (a, b)
        return a

    def search(h=one, q=one, q_off=off, n_q=2, cand=0, k=1, out=one):
        qo = None if q_off is None else _p(q_off)
        a = (L.hpfw_gpu_search_dtw(h, q, qo, n_q, cand, k, out), L.hpfw_gpu_last_error())
        b = (L.hpfw_gpu_search_dtw_device(h, q, qo, n_q, cand, k, out, None), L.hpfw_gpu_last_error())
        assert a[0] == b[0], (a, b)
        return a

    def path(h=one, q=one, k_q=4, clip=0, pth=one, hit=one):
        a = (L.hpfw_gpu_dtw_path(h, q, k_q, clip, pth, hit), L.hpfw_gpu_last_error())
        b = (L.hpfw_gpu_dtw_path_device(h, q, k_q, clip, pth, hit, None), L.hpfw_gpu_last_error())
        assert a[0] == b[0], (a, b)
        return a

    # null pointers, negative counts
    for kw in (dict(h=None), dict(q_off=None), dict(out=None), dict(n_q=-1), dict(pr=None), dict(n_pairs=-1)):
        assert pairs(**kw)[0] == E_INVALID, kw
    for kw in (dict(h=None), dict(q_off=None), dict(out=None), dict(n_q=-1), dict(q=None)):
        assert search(**kw)[0] == E_INVALID, kw
    for kw in (dict(h=None), dict(q=None), dict(pth=None), dict(hit=None), dict(k_q=-1)):
        assert path(**kw)[0] == E_INVALID, kw
    # a decreasing q_off
    for f in (pairs, search):
        rc, msg = f(q_off=np.array([0, 8, 4], np.int64))
        assert rc == E_INVALID and b"non-decreasing" in msg
    # k, candidates
    for k in (0, -1, 65):
        rc, msg = search(k=k)
        assert rc == E_INVALID and b"k must be in 1..64" in msg
    for cand, k in ((-1, 1), (65, 1), (3, 4), (1, 2), (100, 64)):
        rc, msg = search(cand=cand, k=k)
        assert rc == E_INVALID and b"candidates" in msg, (cand, k)
    # a negative pair or clip index
    for bad in ([[0, 0], [-1, 0]], [[0, -3], [1, 0]]):
        rc, msg = pairs(pr=np.array(bad, np.int32))
        assert rc == E_INVALID and b"negative" in msg
    rc, msg = path(clip=-1)
    assert rc == E_INVALID and b"negative" in msg
    # a query above 16000 hashprints
    for f in (pairs, search):
        rc, msg = f(q_off=np.array([0, 4, 16005], np.int64))
        assert rc == E_UNSUPPORTED and b"16000" in msg
    rc, msg = path(k_q=16001)
    assert rc == E_UNSUPPORTED and b"16000" in msg
    # nothing to do is not an error, and touches nothing
    assert pairs(n_pairs=0)[0] == 0
    # (a pair or clip index at or above the number of queries or clips, and the cell cap, need an index: tests/test_gpu_dtw.py)
    # the bindings take pairs as [n][2]
    with pytest.raises(ValueError):
        _lib.Gpu._pairs([0, 1, 2])


def _admissible_paths(k, n):
    """every admissible path of k rows over n columns, written without the recurrence: any first column, increments 1 or 2,
    or 0 directly after a 1 (so never at row 1)"""
    for first in range(n):
        for inc in itertools.product((0, 1, 2), repeat=k - 1):
            if any(d == 0 and (t == 0 or inc[t - 1] != 1) for t, d in enumerate(inc)):
                continue
            p = np.concatenate([[first], first + np.cumsum(inc, dtype=np.int64)]).astype(np.int64) if k > 1 else np.array([first])
            if p[-1] < n:
                yield p


def test_restatement_equals_the_enumeration_of_all_paths():
    rng = np.random.default_rng(2001)
    n_cases = 0
    for k in range(1, 7):
        for n in range(1, 9):
            paths = list(_admissible_paths(k, n))
            assert bool(paths) == ref.reachable(k, n) == (n >= k // 2 + 1), (k, n)
            for rep in range(4):
                # 4-bit hashprints: many ties
                q = rng.integers(0, 16, k).astype(np.uint64)
                r = rng.integers(0, 16, n).astype(np.uint64)
                if rep == 3:
                    q[:] = r[0]
                    r[:] = r[0]                          # every cell ties
                got = ref.pair(q, r, want_path=True)
                if not paths:
                    assert got is None
                    continue
                c = ref.costs(q, r)
                cost = np.array([int(c[np.arange(k), p].sum()) for p in paths])
                best = int(cost.min())
                dist, start, end, path = got
                assert dist == best, (q, r)
                assert end == min(int(p[-1]) for p, d in zip(paths, cost) if d == best), (q, r)
                assert any(d == best and p[0] == start and p[-1] == end for p, d in zip(paths, cost)), (q, r)
                assert ref.path_identities(q, r, dist, start, end, path) == [], (q, r, path)
                assert ref.pair(q, r) == (dist, start, end)
                n_cases += 1
    assert n_cases > 150


def test_tie_order_and_start_propagation():
    """all-equal hashprints: every cell ties at 0; the smallest end is the one the slowest path reaches (C steps), and at a
    cell where A and C tie A is taken"""
    z = np.zeros(5, np.uint64)
    for n in (3, 9):
        d, s, e, p = ref.pair(z, np.zeros(n, np.uint64), want_path=True)
        assert (d, s, e) == (0, 0, 2) and list(p) == [0, 1, 1, 2, 2]     # (4, 2) from (2, 1) by C alone; (2, 1) by C alone
        assert ref.path_identities(z, np.zeros(n, np.uint64), d, s, e, p) == []
    # D(2, 2) is reached by A from (1, 1), by B from (1, 0) and by C from (0, 1), all at 0: A, and S follows it
    c, D, S, ch = ref.tables(np.zeros(3, np.uint64), np.zeros(4, np.uint64))
    assert ch[2, 2] == 0 and S[2, 2] == 0 and ch[1, 2] == 0 and S[1, 2] == 1 and ch[2, 3] == 0 and S[2, 3] == 1
    # distinct columns force the rigid path
    r = np.uint64(1) << np.arange(9, dtype=np.uint64)
    d, s, e, p = ref.pair(r[2:7], r, want_path=True)
    assert (d, s, e) == (0, 2, 6) and list(p) == [2, 3, 4, 5, 6]
    assert ref.pair(z, np.zeros(2, np.uint64)) is None and ref.pair(np.zeros(0, np.uint64), z) is None


def test_never_above_the_plain_search(oracle):
    lengths = [40, 41, 64, 100, 57]
    rng = np.random.default_rng(31)
    clips = [rng.integers(0, 2 ** 64, n, dtype=np.uint64) for n in lengths]
    db_hp, db_off = _lib._ragged(clips, np.uint64)
    queries = [clips[2][10:50] ^ (np.uint64(1) << rng.integers(0, 64, 40, dtype=np.uint64)), rng.integers(0, 2 ** 64, 40, dtype=np.uint64),
               clips[3][::2][:40].copy()]
    q_hp, q_off = _lib._ragged(queries, np.uint64)
    plain = oracle.search_topk(db_hp, db_off, q_hp, q_off, len(lengths))
    for qi, q in enumerate(queries):
        for h in plain[qi]:
            ci = int(h["clip"])
            assert lengths[ci] >= q.size
            d, s, e = ref.pair(q, clips[ci])
            assert d <= int(h["dist"])
            assert (d, ref.rigid_best(q, clips[ci])[0]) <= (int(h["dist"]), int(h["dist"]))
    # the query read off every second column is found by B steps at distance 0, which no rigid offset reaches
    assert ref.pair(queries[2], clips[3]) == (0, 0, 78) and ref.rigid_best(queries[2], clips[3])[0] > 500


def test_planted_case():
    flips = 200
    r, q, planted = ref.planted(flips=flips)
    assert q.size == 305 and r.size == 2320
    inc = np.diff(planted)
    assert (inc == 0).any() and (inc == 2).any() and ref.path_identities(q, r, flips, planted[0], planted[-1], planted) == []
    dist, start, end, path = ref.pair(q, r, want_path=True)
    assert (start, end) == (int(planted[0]), int(planted[-1]))
    # the planted path is admissible and costs exactly the flipped bits: there is no detour to pay for
    assert dist <= flips
    assert ref.path_identities(q, r, dist, start, end, path) == []
    rigid, _ = ref.rigid_best(q, r)
    assert rigid >= 5 * dist, (rigid, dist)


FACADE = r"""
#include <hpfw/gpu/gpu_collector.h>
#include <hpfw/gpu/gpu_storage.h>
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    hpfw::db::GpuStorage<hpfw::GpuCollector> storage;
    hpfw::GpuCollector::Hashprint hp(304, 0);
    auto hits = storage.find_warped(hp, 3, 0);
    auto path = storage.warp_path(hp, 0);
    if (hits.empty() || !path) return 0;
    return (int)(hits[0].cnt + (size_t)hits[0].start + (size_t)hits[0].end + hits[0].filename.size() + path->cnt + path->columns.size());
}
"""


def test_warped_facade_compiles_and_links(tmp_path):
    import subprocess
    src = tmp_path / "warped.cpp"
    src.write_text(FACADE)
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(tmp_path / "warped"), "-L", lib_dir, "-lhpfw_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "warped")], capture_output=True, text=True)   # no argument: no device touched
    assert r.returncode == 2
