"""CPU tests of the local self-join: the entry points are declared, exported and bound, every refusal
happens before a device is touched, and the restatement of tests/localjoin_ref.py against the enumeration of every run, with
the claim that lags below ceil(min_score / T) of overlap may be left out, and the order of ties."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np

import hpfw_amd
from hpfw_amd import _lib

import local_ref
import localjoin_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
SYMS = ("hpfw_gpu_index_localjoin_device", "hpfw_gpu_index_localjoin", "hpfw_gpu_localjoin_geometry")


def test_entry_points_are_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hpfw_gpu.h")).read(), flags=re.S)
    for sym in SYMS:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTS and hasattr(hpfw_amd.lib(), sym)
    assert re.search(r"\}\s*hpfw_passage_pair\s*;", header)
    assert _lib.PASSAGE_PAIR_DTYPE.itemsize == 32 and _lib.PASSAGE_PAIR_DTYPE == ref.PASSAGE_PAIR_DTYPE
    assert _lib.PASSAGE_PAIR_DTYPE.names == ("a", "b", "score", "lag", "a_start", "length", "dist", "pad")
    assert [_lib.PASSAGE_PAIR_DTYPE.fields[n][1] for n in _lib.PASSAGE_PAIR_DTYPE.names] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert hpfw_amd.PASSAGE_PAIR_DTYPE is _lib.PASSAGE_PAIR_DTYPE
    srcs = re.search(r"^SRCS\s*:=(.*)$", open(os.path.join(ROOT, "hpfw_amd", "csrc", "Makefile")).read(), re.M).group(1).split()
    assert "k_localjoin.hip" in srcs and "localjoin.hip" in srcs
    # neither max_rate nor min_score has a default in any binding
    for f in (_lib.Gpu.index_localjoin, _lib.Gpu.index_localjoin_dev, hpfw_amd.LiveSongIdentification.shared_passages):
        for name in ("max_rate", "min_score"):
            assert inspect.signature(f).parameters[name].default is inspect.Parameter.empty, (f, name)
    facade = open(os.path.join(ROOT, "include", "hpfw", "gpu", "gpu_storage.h")).read()
    assert re.search(r"shared_passages\(int max_rate, int min_score\)", facade)
    # the rule's bound on a recording's length is asserted beside the packing of the table's keys
    kernels = open(os.path.join(ROOT, "hpfw_amd", "csrc", "kernels.h")).read()
    assert re.search(r"static_assert\(2 \* 31 \* \(int64_t\)kSelfjoinMaxLen \+ 64 < \(1 << 24\)", kernels)
    assert 2 * 31 * ref.MAX_LEN + 64 < 2 ** 24 <= 2 * 32 * (ref.MAX_LEN + 1)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_bad_arguments_are_refused_without_a_device():
    """the handle here is a buffer of zeros: a call that got as far as using it would not return a status"""
    L = hpfw_amd.lib()
    buf = np.zeros(64, np.int64)
    one = _p(buf)
    count = ctypes.c_int64(0)

    def both(h=one, T=22, ms=100, out=one, cap=2, cnt=True):
        rcs = []
        for rc in (L.hpfw_gpu_index_localjoin(h, T, ms, out, cap, ctypes.byref(count) if cnt else None),
                   L.hpfw_gpu_index_localjoin_device(h, T, ms, out, cap, one if cnt else None, None)):
            rcs.append((rc, L.hpfw_gpu_last_error()))
        assert rcs[0][0] == rcs[1][0], rcs
        return rcs[0]

    rc, msg = both(h=None)
    assert rc == E_INVALID and b"null handle" in msg
    for T in (0, -1, 32, 64):
        rc, msg = both(T=T)
        assert rc == E_INVALID and b"max_rate" in msg
    for ms in (0, -5):
        rc, msg = both(ms=ms)
        assert rc == E_INVALID and b"min_score" in msg
    rc, msg = both(cap=-1)
    assert rc == E_INVALID and b"cap" in msg
    rc, msg = both(out=None)
    assert rc == E_INVALID and b"null out" in msg
    rc, msg = both(cnt=False)
    assert rc == E_INVALID and b"null count" in msg


def test_geometry():
    sl, ch = ctypes.c_int32(0), ctypes.c_int32(0)
    L = hpfw_amd.lib()
    assert L.hpfw_gpu_localjoin_geometry(ctypes.byref(sl), ctypes.byref(ch)) == 0
    assert sl.value >= 16 and ch.value >= 32 and ch.value % 32 == 0
    assert _lib.localjoin_geometry() == (sl.value, ch.value)
    assert L.hpfw_gpu_localjoin_geometry(None, ctypes.byref(ch)) == E_INVALID
    assert L.hpfw_gpu_localjoin_geometry(ctypes.byref(sl), None) == E_INVALID


W = np.uint64(0x0123456789ABCDEF)


def _tiny(rng, n, rep):
    """a few words that differ in 0, 1, 2 or 64 bits, so that runs and ties of runs are common at every T; rep 1: random words"""
    if rep == 1:
        return rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    return np.array([W, W ^ np.uint64(1), W ^ np.uint64(3), ~W], np.uint64)[rng.integers(0, 4, n)]


def test_restatement_equals_enumeration_of_all_runs():
    rng = np.random.default_rng(2610)
    n_cases = n_pairs = 0
    for n_a in range(0, 7):
        for n_b in range(0, 7):
            a, b = _tiny(rng, n_a, (n_a + n_b) % 3 == 2), _tiny(rng, n_b, 0)
            db_hp, db_off = _lib._ragged([a, b], np.uint64)
            for T in (1, 2, 16, 31):
                want = local_ref.enumerate_candidate(a, b, T)
                got = ref.localjoin(db_hp, db_off, T, 1, clip_base=7)
                if want is None:
                    assert got.size == 0, (a, b, T)
                else:
                    assert [tuple(int(v) for v in p) for p in got] == [(7, 8) + want + (0,)], (a, b, T)
                    assert want[0] == T * want[3] - want[4]
                    # one more than the score: not reported
                    assert ref.localjoin(db_hp, db_off, T, want[0]).size == 1 and ref.localjoin(db_hp, db_off, T, want[0] + 1).size == 0
                    n_pairs += 1
                n_cases += 1
    assert n_cases == 7 * 7 * 4 and n_pairs > n_cases // 3


def test_lags_below_the_shortest_reportable_overlap_may_be_left_out():
    """a run that scores min_score has at least ceil(min_score / T) positions, so what is reported does not change when the lags
    that overlap less are not looked at -- for every min_score up to one above the pair's score"""
    rng = np.random.default_rng(2611)
    n_checked = n_differ = 0
    for case in range(60):
        n_a, n_b = (int(v) for v in rng.integers(1, 13, 2))
        a, b = _tiny(rng, n_a, case % 4 == 3), _tiny(rng, n_b, 0)
        for T in (1, 2, 5, 16, 31):
            full = local_ref.clip_candidate(a, b, T)
            assert full == ref.candidate_pruned(a, b, T, 1)
            top = full[0] if full else 0
            for min_score in range(1, top + 2):
                min_len = -(-min_score // T)
                pruned = ref.candidate_pruned(a, b, T, min_len)
                n_differ += pruned != full
                rep_full = full if full and full[0] >= min_score else None
                rep_pruned = pruned if pruned and pruned[0] >= min_score else None
                assert rep_full == rep_pruned, (a, b, T, min_score)
                n_checked += 1
    assert n_checked > 2000 and n_differ > 20             # (the pruned scan does see other candidates: below min_score)


def _join(clips, T, min_score=1):
    db_hp, db_off = _lib._ragged([np.asarray(c, np.uint64) for c in clips], np.uint64)
    return [tuple(int(v) for v in p)[:7] for p in ref.localjoin(db_hp, db_off, T, min_score)]


def test_tie_order():
    a, b, c = (np.uint64(v) for v in (0x0123456789ABCDEF, 0x0F1E2D3C4B5A6978, 0x13579BDF02468ACE))
    d, e = np.uint64(0x2468ACE013579BDF), np.uint64(0x0FEDCBA987654321)
    # the passage (a, b) lies at two lags of the second clip: the smaller lag wins
    assert _join([[a, b], [c, a, b, ~c, a, b, c]], 8) == [(0, 1, 16, 1, 0, 2, 0)]
    # ... and at two positions of the first: the smaller lag is the later position
    assert _join([[c, a, b, ~c, a, b, c], [a, b]], 8) == [(0, 1, 16, -4, 4, 2, 0)]
    # two runs of one diagonal with the same score: the one that ends first; an all-mismatch hashprint parts them
    assert _join([[a, b, c, d, e], [a, b, ~c, d, e]], 8) == [(0, 1, 16, 0, 0, 2, 0)]
    # the same end, two starts: a hashprint with exactly T mismatching bits adds 0 -- the smaller start wins
    assert _join([[a, b, c], [a ^ np.uint64(0xFF), b, c]], 8) == [(0, 1, 16, 0, 0, 3, 8)]
    # ... and at the end of a run the shorter one
    assert _join([[a, b, c], [a, b, c ^ np.uint64(0xFF)]], 8) == [(0, 1, 16, 0, 0, 2, 0)]
    # three clips: pairs in ascending (a, b); an empty clip and an all-mismatch clip never appear
    r = np.arange(1, 9, dtype=np.uint64) * a
    assert _join([r, [], r[2:6], ~r, r], 20) == [(0, 2, 80, -2, 2, 4, 0), (0, 4, 160, 0, 0, 8, 0), (2, 4, 80, 2, 0, 4, 0)]
    assert _join([r, [], r[2:6], ~r, r], 20, 81) == [(0, 4, 160, 0, 0, 8, 0)]
    assert _join([np.zeros(10), np.full(5, 0xFFFFFFFFFFFFFFFF, np.uint64)], 31) == []


FACADE = r"""
#include <hpfw/gpu/gpu_collector.h>
#include <hpfw/gpu/gpu_storage.h>
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    hpfw::db::GpuStorage<hpfw::GpuCollector> storage;
    auto pairs = storage.shared_passages(22, 1000);
    if (pairs.empty()) return 0;
    return (int)(pairs[0].score + pairs[0].lag + (int64_t)(pairs[0].a_start + pairs[0].length + pairs[0].cnt + pairs[0].name_a.size() +
                                                           pairs[0].name_b.size()));
}
"""


def test_shared_passages_facade_compiles_and_links(tmp_path):
    src = tmp_path / "passages.cpp"
    src.write_text(FACADE)
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(tmp_path / "passages"), "-L", lib_dir, "-lhpfw_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "passages")], capture_output=True, text=True)   # no argument: no device touched
    assert r.returncode == 2
