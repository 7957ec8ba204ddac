"""CPU tests of the catalogue self-join: the entry points are declared, exported and bound, every
refusal happens before a device is touched, and the restatement of tests/selfjoin_ref.py against a bit-by-bit loop and
against the overlap search all-against-all."""
import ctypes
import inspect
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, liveid

import overlap_ref
import selfjoin_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
SYMS = ("hpfw_gpu_index_selfjoin_device", "hpfw_gpu_index_selfjoin", "hpfw_gpu_selfjoin_geometry")


def test_entry_points_are_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hpfw_gpu.h")).read(), flags=re.S)
    for sym in SYMS:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTS and hasattr(hpfw_amd.lib(), sym)
    assert re.search(r"\}\s*hpfw_dup_pair\s*;", header)
    assert _lib.DUP_PAIR_DTYPE.itemsize == 24 and _lib.DUP_PAIR_DTYPE == ref.DUP_PAIR_DTYPE
    assert _lib.DUP_PAIR_DTYPE.names == ("a", "b", "dist", "overlap", "lag", "pad")
    srcs = re.search(r"^SRCS\s*:=(.*)$", open(os.path.join(ROOT, "hpfw_amd", "csrc", "Makefile")).read(), re.M).group(1).split()
    assert "k_selfjoin.hip" in srcs and "selfjoin.hip" in srcs
    # neither min_overlap nor the threshold has a default in any binding
    for f, params in ((_lib.Gpu.index_selfjoin, ("min_overlap", "rate_num", "rate_den")),
                      (_lib.Gpu.index_selfjoin_dev, ("min_overlap", "rate_num", "rate_den")),
                      (hpfw_amd.LiveSongIdentification.duplicates, ("max_rate", "min_overlap"))):
        for name in params:
            assert inspect.signature(f).parameters[name].default is inspect.Parameter.empty, (f, name)
    facade = open(os.path.join(ROOT, "include", "hpfw", "gpu", "gpu_storage.h")).read()
    assert re.search(r"duplicates\(int min_overlap, int rate_num, int rate_den\)", facade)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_bad_arguments_are_refused_without_a_device():
    """the handle here is a buffer of zeros: a call that got as far as using it would not return a status"""
    L = hpfw_amd.lib()
    buf = np.zeros(64, np.int64)
    one = _p(buf)
    count = ctypes.c_int64(0)

    def both(h=one, mo=8, num=16, den=1, out=one, cap=2, cnt=True):
        rcs = []
        for rc in (L.hpfw_gpu_index_selfjoin(h, mo, num, den, out, cap, ctypes.byref(count) if cnt else None),
                   L.hpfw_gpu_index_selfjoin_device(h, mo, num, den, out, cap, one if cnt else None, None)):
            rcs.append((rc, L.hpfw_gpu_last_error()))
        assert rcs[0][0] == rcs[1][0], rcs
        return rcs[0]

    rc, msg = both(h=None)
    assert rc == E_INVALID and b"null handle" in msg
    for den in (0, -1, 1025):
        rc, msg = both(den=den)
        assert rc == E_INVALID and b"rate_den" in msg
    for num, den in ((-1, 1), (65, 1), (64 * 1024 + 1, 1024), (129, 2)):
        rc, msg = both(num=num, den=den)
        assert rc == E_INVALID and b"rate_num" in msg
    for mo in (0, -3, 2 ** 18):
        rc, msg = both(mo=mo)
        assert rc == E_INVALID and b"min_overlap" in msg
    rc, msg = both(cap=-1)
    assert rc == E_INVALID and b"cap" in msg
    rc, msg = both(out=None)
    assert rc == E_INVALID and b"null out" in msg
    rc, msg = both(cnt=False)
    assert rc == E_INVALID and b"null count" in msg


def test_geometry():
    sl, ch = ctypes.c_int32(0), ctypes.c_int32(0)
    L = hpfw_amd.lib()
    assert L.hpfw_gpu_selfjoin_geometry(ctypes.byref(sl), ctypes.byref(ch)) == 0
    assert sl.value >= 16 and ch.value >= 32 and ch.value % 32 == 0
    assert _lib.selfjoin_geometry() == (sl.value, ch.value)
    assert L.hpfw_gpu_selfjoin_geometry(None, ctypes.byref(ch)) == E_INVALID
    assert L.hpfw_gpu_selfjoin_geometry(ctypes.byref(sl), None) == E_INVALID


def _tiny(rng, n, rep):
    """few distinct words and few bits set, so that ties in dist / L across different L are common; rep 2: random words"""
    if rep == 2:
        return rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    return rng.integers(0, 4, n).astype(np.uint64) * np.uint64(0x8000000000000001)


def test_restatement_equals_a_bit_by_bit_loop():
    rng = np.random.default_rng(2210)
    n_cases = 0
    for n_a in range(0, 7):
        for n_b in range(0, 7):
            for rep in range(3):
                a, b = _tiny(rng, n_a, rep), _tiny(rng, n_b, rep)
                for mo in range(1, 8):
                    want = overlap_ref.loop_candidate(a, b, mo)
                    assert ref.pair_candidate(a, b, mo) == want, (a, b, mo)
                    assert (want is None) == (n_a < mo or n_b < mo)
                    n_cases += 1
    assert n_cases == 7 * 7 * 3 * 7


def test_restatement_equals_the_overlap_search_all_against_all():
    """per pair a < b the (dist, L, lag) of search_overlap with every clip as a query and itself excluded"""
    rng = np.random.default_rng(2211)
    lengths = [0, 1, 3, 5, 8, 8, 13, 21, 40, 64, 7]
    clips = [_tiny(rng, n, i % 3) for i, n in enumerate(lengths)]
    clips[5] = clips[4].copy()
    clips[8][10:23] = clips[6]
    db_hp, db_off = _lib._ragged(clips, np.uint64)
    me = np.arange(len(clips), dtype=np.int32)
    for mo in (1, 3, 8):
        cand = ref.candidates(db_hp, db_off, mo)
        hits = overlap_ref.search_overlap(db_hp, db_off, db_hp, db_off, 64, mo, exclude=me)
        by_pair = {(a, int(h["clip"])): (int(h["dist"]), int(h["overlap"]), int(h["lag"]))
                   for a, row in enumerate(hits) for h in row if h["clip"] != 0xFFFFFFFF}
        m = sum(n >= mo for n in lengths)
        assert len(cand) == m * (m - 1) // 2 and {p for p in by_pair if p[0] < p[1]} == set(cand)
        for pair, c in cand.items():
            assert by_pair[pair] == c, (pair, mo)
        full = ref.selfjoin(db_hp, db_off, mo, 64, 1, clip_base=100)
        assert [(int(p["a"]) - 100, int(p["b"]) - 100) for p in full] == sorted(cand) and (full["pad"] == 0).all()


def test_the_thresholds_edge():
    """dist * rate_den == rate_num * L is reported, one more mismatching bit is not"""
    a = np.zeros(12, np.uint64)
    b = np.zeros(12, np.uint64)
    b[:9] = 1                                             # 9 bits over 12 hashprints: 3 / 4 (min_overlap 12: lag 0 alone)
    db_hp, db_off = _lib._ragged([a, b], np.uint64)
    assert ref.pair_candidate(a, b, 12) == (9, 12, 0)
    assert ref.selfjoin(db_hp, db_off, 12, 3, 4).size == 1 and ref.selfjoin(db_hp, db_off, 12, 768, 1024).size == 1
    assert ref.selfjoin(db_hp, db_off, 12, 767, 1024).size == 0
    b[9] = 1                                              # 10 / 12 > 3 / 4
    db_hp, db_off = _lib._ragged([a, b], np.uint64)
    assert ref.pair_candidate(a, b, 12) == (10, 12, 0)
    assert ref.selfjoin(db_hp, db_off, 12, 3, 4).size == 0 and ref.selfjoin(db_hp, db_off, 12, 5, 6).size == 1
    assert ref.reported(0, 5, 0, 1) and not ref.reported(1, 2 ** 18 - 1, 0, 1) and ref.reported(64 * 7, 7, 64, 1)
    # the products need more than the overlap search's two 24-bit multiplies and 14-bit L: 2^24 * 2^18
    assert ref.reported(2 ** 24 - 64, 2 ** 18 - 1, 64 * 1024, 1024) and not ref.reported(2 ** 24 - 63, 2 ** 18 - 1, 65535, 1024)


def test_duplicate_groups():
    names = [f"n{i}" for i in range(12)]

    def pair(a, b):
        return (names[a], names[b], 0, 100, 0)

    chain = [pair(2, 5), pair(5, 9), pair(9, 11)]
    star = [pair(0, 3), pair(0, 4), pair(0, 10)]
    isolated = [pair(6, 7)]
    assert liveid.duplicate_groups(chain, names) == [["n2", "n5", "n9", "n11"]]
    assert liveid.duplicate_groups(star, names) == [["n0", "n3", "n4", "n10"]]
    assert liveid.duplicate_groups(isolated, names) == [["n6", "n7"]]
    everything = [star[2], chain[2], isolated[0], chain[0], star[0], chain[1], star[1]]          # in any order
    assert liveid.duplicate_groups(everything, names) == [["n0", "n3", "n4", "n10"], ["n2", "n5", "n9", "n11"], ["n6", "n7"]]
    assert liveid.duplicate_groups(everything + [pair(4, 11)], names) == [["n0", "n2", "n3", "n4", "n5", "n9", "n10", "n11"], ["n6", "n7"]]
    assert liveid.duplicate_groups([], names) == []
    # the method takes the identifier's live names
    lsi = hpfw_amd.LiveSongIdentification.__new__(hpfw_amd.LiveSongIdentification)
    lsi.names, lsi._removed = names, {1}
    assert lsi.duplicate_groups(chain + isolated) == [["n2", "n5", "n9", "n11"], ["n6", "n7"]]


def test_max_rate_conversion():
    assert liveid.rate_fraction(16) == (16, 1) and liveid.rate_fraction(0) == (0, 1) and liveid.rate_fraction(64) == (64, 1)
    assert liveid.rate_fraction(Fraction(33, 2)) == (33, 2) and liveid.rate_fraction(Fraction(65535, 1024)) == (65535, 1024)
    assert liveid.rate_fraction(16.5) == (33, 2) and liveid.rate_fraction(0.1) == (1, 10)
    num, den = liveid.rate_fraction(19.38)
    assert den <= 1024 and Fraction(num, den) == Fraction(19.38).limit_denominator(1024)
    for bad in (-1, 65, Fraction(-1, 3), Fraction(1, 1025), 64.5, -0.25, float("nan"), float("inf"), "16", None, True):
        with pytest.raises(hpfw_amd.HpfwError) as e:
            liveid.rate_fraction(bad)
        assert e.value.status == E_INVALID, bad
    # refused before the index is asked, and a sharded identifier has no self-join
    sharded = hpfw_amd.LiveSongIdentification.__new__(hpfw_amd.LiveSongIdentification)
    sharded._gpu = object.__new__(liveid._ShardedIndex)
    with pytest.raises(hpfw_amd.HpfwError) as e:
        sharded.duplicates(65, 100)
    assert e.value.status == E_INVALID
    with pytest.raises(hpfw_amd.HpfwError) as e:
        sharded.duplicates(16, 100)
    assert e.value.status == E_UNSUPPORTED


FACADE = r"""
#include <hpfw/gpu/gpu_collector.h>
#include <hpfw/gpu/gpu_storage.h>
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    hpfw::db::GpuStorage<hpfw::GpuCollector> storage;
    auto pairs = storage.duplicates(100, 16, 1);
    if (pairs.empty()) return 0;
    return (int)(pairs[0].dist + pairs[0].overlap + (size_t)pairs[0].lag + pairs[0].name_a.size() + pairs[0].name_b.size());
}
"""


def test_duplicates_facade_compiles_and_links(tmp_path):
    src = tmp_path / "duplicates.cpp"
    src.write_text(FACADE)
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(tmp_path / "duplicates"), "-L", lib_dir, "-lhpfw_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "duplicates")], capture_output=True, text=True)   # no argument: no device touched
    assert r.returncode == 2
