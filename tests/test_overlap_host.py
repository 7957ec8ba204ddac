"""CPU tests of the overlap search: the entry points are declared and exported, every refusal happens
before a device is touched, and the restatement of tests/overlap_ref.py against a bit-by-bit loop, against the plain search
where the two rules coincide, and on hand-built orderings."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, synth

import overlap_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
SYMS = ("hpfw_gpu_search_overlap_device", "hpfw_gpu_search_overlap")


def test_entry_points_are_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hpfw_gpu.h")).read(), flags=re.S)
    for sym in SYMS:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTS and hasattr(hpfw_amd.lib(), sym)
    assert re.search(r"\}\s*hpfw_overlap_hit\s*;", header)
    assert _lib.OVERLAP_HIT_DTYPE.itemsize == 16 and _lib.OVERLAP_HIT_DTYPE == ref.OVERLAP_HIT_DTYPE
    assert _lib.OVERLAP_HIT_DTYPE.names == ("dist", "clip", "lag", "overlap")
    # min_overlap has no default in any binding
    import inspect
    for f in (_lib.Gpu.search_overlap, _lib.Gpu.search_overlap_dev, hpfw_amd.LiveSongIdentification.top_overlap):
        assert inspect.signature(f).parameters["min_overlap"].default is inspect.Parameter.empty
    facade = open(os.path.join(ROOT, "include", "hpfw", "gpu", "gpu_storage.h")).read()
    assert re.search(r"find_overlap\(const typename Collector::Hashprint &hp, int k, int min_overlap\)", facade)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_bad_arguments_are_refused_without_a_device():
    """the handle here is a buffer of zeros: a call that got as far as using it would not return a status"""
    L = hpfw_amd.lib()
    buf = np.zeros(64, np.int64)
    one = _p(buf)
    off = np.array([0, 4, 8], np.int64)

    def both(h=one, q=one, q_off=off, n_q=2, ex=None, mo=2, k=1, out=one):
        qo = None if q_off is None else _p(q_off)
        e = None if ex is None else _p(ex)
        rcs = []
        for rc in (L.hpfw_gpu_search_overlap(h, q, qo, n_q, e, mo, k, out),
                   L.hpfw_gpu_search_overlap_device(h, q, qo, n_q, e, mo, k, out, None)):
            rcs.append((rc, L.hpfw_gpu_last_error()))
        assert rcs[0][0] == rcs[1][0], rcs
        return rcs[0]

    for kw in (dict(h=None), dict(q_off=None), dict(out=None), dict(n_q=-1), dict(q=None)):
        assert both(**kw)[0] == E_INVALID, kw
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
    # (an exclude entry at or above the number of clips needs an index to count: tests/test_gpu_overlap.py)
    # the bindings take one exclude entry per query
    with pytest.raises(ValueError):
        _lib.Gpu._exclude([0, 1, 2], 2)


def test_restatement_equals_a_bit_by_bit_loop():
    rng = np.random.default_rng(1701)
    n_cases = 0
    for k in range(1, 7):
        for n in range(0, 9):
            for rep in range(3):
                # few distinct words and few bits set: ties in dist / L across different L are common
                q = rng.integers(0, 4, k).astype(np.uint64) * np.uint64(0x8000000000000001)
                r = rng.integers(0, 4, n).astype(np.uint64) * np.uint64(0x8000000000000001)
                if rep == 2:
                    q, r = rng.integers(0, 2 ** 64, k, dtype=np.uint64), rng.integers(0, 2 ** 64, n, dtype=np.uint64)
                for mo in range(1, 10):
                    want = ref.loop_candidate(q, r, mo)
                    assert ref.clip_candidate(q, r, mo) == want, (q, r, mo)
                    assert ref.clip_candidate_fast(q, r, mo) == want, (q, r, mo)
                    assert (want is None) == (k < mo or n < mo)
                    n_cases += 1
    assert n_cases == 6 * 9 * 3 * 9
    for k, n in ((3, 5), (5, 3), (4, 4)):
        for d in range(-k - 1, n + 2):
            assert max(ref.overlap(k, n, d), 0) == len([j for j in range(k) if 0 <= d + j < n])


def test_min_overlap_k_is_the_plain_search(oracle):
    """no clip shorter than the query, min_overlap = k: the lags are the offsets 0 .. n - k, every L is k, and the order
    (dist / k, clip) is (dist, clip)"""
    lengths = [304, 305, 400, 1024, 310, 2320, 304, 777]
    full = synth.random_hashprints(len(lengths), max(lengths), 21)
    db_hp, db_off = _lib._ragged([full[i, :n] for i, n in enumerate(lengths)], np.uint64)
    rng = np.random.default_rng(22)
    queries = []
    for c, o in ((1, 1), (3, 720), (5, 2016), (6, 0), (2, 50)):
        q = db_hp[db_off[c] + o:db_off[c] + o + 304].copy()
        q ^= np.uint64(1) << rng.integers(0, 64, 304, dtype=np.uint64)
        queries.append(q)
    queries.append(rng.integers(0, 2 ** 64, 304, dtype=np.uint64))
    q_hp, q_off = _lib._ragged(queries, np.uint64)
    for top_k in (1, 3, 8, 10):
        got = ref.search_overlap(db_hp, db_off, q_hp, q_off, top_k, 304)
        want = oracle.search_topk(db_hp, db_off, q_hp, q_off, top_k)
        assert np.array_equal(got["dist"], want["dist"]) and np.array_equal(got["clip"], want["clip"])
        assert np.array_equal(got["lag"], want["offset"])
        assert (got["overlap"][want["clip"] != 0xFFFFFFFF] == 304).all() and (got["overlap"][want["clip"] == 0xFFFFFFFF] == 0).all()
    assert [int(c) for c in ref.search_overlap(db_hp, db_off, q_hp, q_off, 1, 304)["clip"][:5, 0]] == [1, 3, 5, 6, 2]


def _search(clips, queries, top_k, mo, **kw):
    db_hp, db_off = _lib._ragged([np.asarray(c, np.uint64) for c in clips], np.uint64)
    q_hp, q_off = _lib._ragged([np.asarray(q, np.uint64) for q in queries], np.uint64)
    return ref.search_overlap(db_hp, db_off, q_hp, q_off, top_k, mo, **kw)


def test_ordering():
    ones = np.uint64(0xFFFFFFFFFFFFFFFF)
    # all-zero query against all-zero clips: rate 0 at every lag, so the largest L wins, then the smallest lag
    got = _search([np.zeros(10), np.zeros(3), np.zeros(7)], [np.zeros(5)], 3, 2)[0]
    assert [tuple(int(v) for v in h) for h in got] == [(0, 0, 0, 5), (0, 2, 0, 5), (0, 1, -2, 3)]
    # all-ones against zeros: rate 64 everywhere
    got = _search([np.zeros(10), np.zeros(3)], [np.full(5, ones)], 2, 2)[0]
    assert [tuple(int(v) for v in h) for h in got] == [(320, 0, 0, 5), (192, 1, -2, 3)]
    # two clips with equal content: the smaller id wins; exclude and clip_base
    r = np.arange(1, 9, dtype=np.uint64) * np.uint64(0x0123456789ABCDEF)
    got = _search([r[::-1].copy(), r, r], [r[2:6]], 3, 4)[0]
    assert [(int(h["dist"]), int(h["clip"]), int(h["lag"])) for h in got[:2]] == [(0, 1, 2), (0, 2, 2)] and got[2]["clip"] == 0
    got = _search([r[::-1].copy(), r, r], [r[2:6]], 3, 4, exclude=[1], clip_base=100)[0]
    assert [int(h["clip"]) for h in got] == [102, 100, 0xFFFFFFFF] and tuple(int(v) for v in got[2]) == ref.PAD
    # 32 / 64 against 64 / 128 -- the same rate in other terms: the larger overlap wins whichever clip comes first
    q = np.zeros(128, np.uint64)
    a = np.full(64, np.uint64(1))                         # one bit at every position: 64 / 64 against 128 / 128 first
    b = np.full(128, np.uint64(1))
    for clips, want in (([a, b], 1), ([b, a], 0)):
        got = _search(clips, [q], 2, 64)[0]
        assert int(got[0]["clip"]) == want and (int(got[0]["dist"]), int(got[0]["overlap"])) == (128, 128)
        assert (int(got[1]["dist"]), int(got[1]["overlap"])) == (64, 64)
        assert Fraction(int(got[0]["dist"]), int(got[0]["overlap"])) == Fraction(int(got[1]["dist"]), int(got[1]["overlap"]))
    half = np.zeros(64, np.uint64)
    half[::2] = 1                                         # 32 / 64
    full = np.zeros(128, np.uint64)
    full[32:96] = 1                                       # 64 / 128, and no prefix or suffix of 64 or more below 1 / 2
    got = _search([half, full], [q], 2, 64)[0]
    assert [(int(h["dist"]), int(h["clip"]), int(h["overlap"])) for h in got] == [(64, 1, 128), (32, 0, 64)]
    # a strictly smaller rate beats a larger overlap: 31 / 64 < 64 / 128
    half[0] = 0
    got = _search([half, full], [q], 2, 64)[0]
    assert [(int(h["dist"]), int(h["clip"])) for h in got] == [(31, 0), (64, 1)]
    # a query below min_overlap, a clip below min_overlap, an empty index
    assert tuple(int(v) for v in _search([np.zeros(10)], [np.zeros(3)], 1, 4)[0, 0]) == ref.PAD
    assert tuple(int(v) for v in _search([np.zeros(3)], [np.zeros(10)], 1, 4)[0, 0]) == ref.PAD
    assert tuple(int(v) for v in ref.search_overlap(np.zeros(0, np.uint64), np.zeros(1, np.int64), np.zeros(4, np.uint64),
                                                    np.array([0, 4]), 1, 1)[0, 0]) == ref.PAD


FACADE = r"""
#include <hpfw/gpu/gpu_collector.h>
#include <hpfw/gpu/gpu_storage.h>
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    hpfw::db::GpuStorage<hpfw::GpuCollector> storage;
    hpfw::GpuCollector::Hashprint hp(304, 0);
    auto hits = storage.find_overlap(hp, 3, 100);
    if (hits.empty()) return 0;
    return (int)(hits[0].cnt + hits[0].overlap + (size_t)hits[0].lag + hits[0].filename.size());
}
"""


def test_overlap_facade_compiles_and_links(tmp_path):
    import subprocess
    src = tmp_path / "overlap.cpp"
    src.write_text(FACADE)
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(tmp_path / "overlap"), "-L", lib_dir, "-lhpfw_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "overlap")], capture_output=True, text=True)   # no argument: no device touched
    assert r.returncode == 2
