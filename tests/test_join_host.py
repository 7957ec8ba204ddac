"""CPU tests of the ingest check: the entry points are declared, exported and bound, every refusal
happens before a device is touched, hpfw_gpu_join_plan covers every pair once, the restatement of tests/join_ref.py against a
bit-by-bit loop, and the host rule of add_new()."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, liveid

import join_ref as ref
import overlap_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
SYMS = ("hpfw_gpu_index_join_device", "hpfw_gpu_index_join", "hpfw_gpu_join_plan")


def test_entry_points_are_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hpfw_gpu.h")).read(), flags=re.S)
    for sym in SYMS:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTS and hasattr(hpfw_amd.lib(), sym)
    # neither min_overlap nor the threshold nor among_new has a default in the low-level bindings
    for f in (_lib.Gpu.index_join, _lib.Gpu.index_join_dev):
        for name in ("min_overlap", "rate_num", "rate_den", "among_new"):
            assert inspect.signature(f).parameters[name].default is inspect.Parameter.empty, (f, name)
    known = inspect.signature(hpfw_amd.LiveSongIdentification.known).parameters
    assert list(known) == ["self", "filenames", "max_rate", "min_overlap", "among_new"] and known["among_new"].default is True
    add_new = inspect.signature(hpfw_amd.LiveSongIdentification.add_new).parameters
    assert list(add_new) == ["self", "filenames", "max_rate", "min_overlap"]
    for p in (known, add_new):
        assert p["max_rate"].default is inspect.Parameter.empty and p["min_overlap"].default is inspect.Parameter.empty
    facade = open(os.path.join(ROOT, "include", "hpfw", "gpu", "gpu_storage.h")).read()
    assert re.search(r"join\(Range &&hashprints, int min_overlap, int rate_num, int rate_den, bool among_new\)", facade)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_bad_arguments_are_refused_without_a_device():
    """the handle here is a buffer of zeros: a call that got as far as using it would not return a status"""
    L = hpfw_amd.lib()
    buf = np.zeros(64, np.int64)
    one = _p(buf)
    count = ctypes.c_int64(0)
    good_off = np.array([0, 5, 5, 12], np.int64)

    def both(h=one, x=one, off=good_off, n_x=None, among=1, mo=8, num=16, den=1, out=one, cap=2, cnt=True):
        n_x = (0 if off is None else off.size - 1) if n_x is None else n_x
        p_off = None if off is None else _p(off)
        rcs = []
        for rc in (L.hpfw_gpu_index_join(h, x, p_off, n_x, among, mo, num, den, out, cap, ctypes.byref(count) if cnt else None),
                   L.hpfw_gpu_index_join_device(h, x, p_off, n_x, among, mo, num, den, out, cap, one if cnt else None, None)):
            rcs.append((rc, L.hpfw_gpu_last_error()))
        assert rcs[0][0] == rcs[1][0], rcs
        return rcs[0]

    # everything the self-join refuses
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
    # the join's own
    rc, msg = both(off=None)
    assert rc == E_INVALID and b"null x_off" in msg
    rc, msg = both(n_x=-1)
    assert rc == E_INVALID and b"n_x" in msg
    for bad in ([0, 5, 4, 12], [3, 0], [0, 10, 20, 19]):
        rc, msg = both(off=np.array(bad, np.int64))
        assert rc == E_INVALID and b"non-decreasing" in msg, bad
    rc, msg = both(x=None)
    assert rc == E_INVALID and b"null hashprints" in msg
    for among in (-1, 2, 7):
        rc, msg = both(among=among)
        assert rc == E_INVALID and b"among_new" in msg
    # a recording of the batch above 2^18 - 1 hashprints: known from the offsets alone
    for off in ([0, 2 ** 18], [7, 9, 9 + 2 ** 18, 10 + 2 ** 18]):
        rc, msg = both(off=np.array(off, np.int64))
        assert rc == E_UNSUPPORTED and b"262143" in msg, off


def test_plan_refusals():
    L = hpfw_amd.lib()
    pf = np.zeros(8, np.uint32)
    assert L.hpfw_gpu_join_plan(10, 3, 1, 0, 2, _p(pf)) == 0
    for args in ((-1, 3, 1, 0, 2), (10, -1, 1, 0, 2), (10, 3, 2, 0, 2), (10, 3, -1, 0, 2), (10, 3, 1, -1, 2), (10, 3, 1, 0, -1)):
        assert L.hpfw_gpu_join_plan(*args, _p(pf)) == E_INVALID, args
    assert L.hpfw_gpu_join_plan(10, 3, 1, 0, 2, None) == E_INVALID
    assert L.hpfw_gpu_join_plan(2 ** 21, 1, 1, 0, 2, _p(pf)) == E_UNSUPPORTED
    assert L.hpfw_gpu_join_plan(2 ** 21 - 1, 1, 1, 0, 2, _p(pf)) == 0


def test_plan_covers_every_pair_once():
    """for every n, m <= 70, both flags and passes of 1 to 3 row groups: each pair (a, b) with n <= b < n + m, a < b (a < n
    without among_new) lies in exactly one (group, b) item of exactly one pass, and no item is empty.  Item pair_first[i] + j
    of a pass from group0 on is (group0 + i, b = max(n, 32 (group0 + i) + 1) + j); its rows are a = 32 g .. 32 g + 31 below b
    (and below n without among_new)."""
    rows32 = np.arange(32)[:, None]
    for n in range(71):
        for m in range(71):
            for among in (0, 1):
                row_end = n + m if among else n
                a_ids, b_ids = np.arange(160)[:, None], n + np.arange(m)[None, :]
                want = ((a_ids < b_ids) & (a_ids < row_end)).astype(np.int32)
                for per_pass in (1, 2, 3):
                    seen = np.zeros((160, m), np.int32)
                    for g0 in range(0, 5, per_pass):                 # (5 groups reach id 159 >= n + m; the last ones are empty)
                        pf = _lib.join_plan(n, m, among, g0, per_pass).astype(np.int64)
                        assert pf[0] == 0 and (np.diff(pf) >= 0).all()
                        for i in range(per_pass):
                            g, items = g0 + i, int(pf[i + 1] - pf[i])
                            if g >= 5:
                                assert items == 0
                                continue
                            b = max(n, 32 * g + 1) + np.arange(items)
                            assert items == 0 or b[-1] == n + m - 1, (n, m, among, g)      # b runs to the last external
                            covered = (32 * g + rows32 < np.minimum(b, row_end)[None, :])
                            assert covered.any(axis=0).all(), ("an empty item", n, m, among, g)
                            seen[32 * g:32 * g + 32, b - n] += covered
                    assert np.array_equal(seen, want), (n, m, among, per_pass)


def _tiny(rng, n, rep):
    """few distinct words and few bits set, so that ties in dist / L across different L are common; rep 2: random words"""
    if rep == 2:
        return rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    return rng.integers(0, 4, n).astype(np.uint64) * np.uint64(0x8000000000000001)


def test_restatement_equals_a_bit_by_bit_loop():
    """one indexed recording a against one external b, and the two as a batch against an empty index"""
    rng = np.random.default_rng(2310)
    n_cases = 0
    empty = (np.zeros(1, np.uint64), np.zeros(1, np.int64))
    for n_a in range(0, 7):
        for n_b in range(0, 7):
            for rep in range(3):
                a, b = _tiny(rng, n_a, rep), _tiny(rng, n_b, rep)
                db, x, ab = _lib._ragged([a], np.uint64), _lib._ragged([b], np.uint64), _lib._ragged([a, b], np.uint64)
                for mo in range(1, 8):
                    cand = overlap_ref.loop_candidate(a, b, mo)
                    want = [] if cand is None else [(1000, 1001) + cand + (0,)]
                    for among in (0, 1):
                        got = ref.join(*db, *x, mo, 64, 1, among, clip_base=1000)
                        assert [tuple(int(v) for v in p) for p in got] == want, (a, b, mo, among)
                    assert [tuple(int(v) for v in p) for p in ref.join(*empty, *ab, mo, 64, 1, 1, clip_base=1000)] == want
                    assert ref.join(*empty, *ab, mo, 64, 1, 0).size == 0
                    n_cases += 1
    assert n_cases == 7 * 7 * 3 * 7


def test_restatement_is_what_add_then_selfjoin_adds():
    """on a small index and batch: selfjoin(index + batch) = selfjoin(index) + join(among_new = 1), as sets and in order"""
    import selfjoin_ref
    rng = np.random.default_rng(2311)
    clips = [_tiny(rng, n, i % 3) for i, n in enumerate([0, 3, 8, 8, 13, 21])]
    batch = [_tiny(rng, n, i % 3) for i, n in enumerate([8, 0, 5, 13])]
    batch[0] = clips[2].copy()
    batch[3] = batch[0].tolist() + batch[2].tolist()
    db, x = _lib._ragged(clips, np.uint64), _lib._ragged(batch, np.uint64)
    x = (np.concatenate([np.full(3, 7, np.uint64), x[0]]), x[1] + 3)                     # (offsets that do not begin at 0)
    for mo in (1, 4):
        before = selfjoin_ref.selfjoin(*db, mo, 40, 1, clip_base=50)
        after = selfjoin_ref.selfjoin(*ref.appended(*db, *x), mo, 40, 1, clip_base=50)
        new = ref.join(*db, *x, mo, 40, 1, 1, clip_base=50)
        assert new.size and (new["b"] >= 50 + len(clips)).all() and before.size + new.size == after.size
        assert np.array_equal(np.sort(np.concatenate([before, new]), order=("a", "b")), after)
        old_only = ref.join(*db, *x, mo, 40, 1, 0, clip_base=50)
        assert np.array_equal(old_only, new[new["a"] < 50 + len(clips)]) and 0 < old_only.size < new.size


def test_keep_new():
    def pairs(*ab):
        return [(a, b, 0, 100, 0) for a, b in ab]

    keep = liveid.keep_new
    assert keep([], 5, 3) == [True, True, True] and keep([], 0, 0) == []
    # a chain: x0 duplicates an indexed recording and x1 duplicates only x0, which is dropped -- so x1 is kept
    assert keep(pairs((2, 5), (5, 6)), 5, 2) == [False, True]
    # a longer chain x0 - x1 - x2 - x3 of new recordings: every other one goes
    assert keep(pairs((5, 6), (6, 7), (7, 8)), 5, 4) == [True, False, True, False]
    # a star around an indexed recording, and around the batch's first
    assert keep(pairs((1, 5), (1, 6), (1, 8)), 5, 4) == [False, False, True, False]
    assert keep(pairs((5, 6), (5, 7), (5, 8)), 5, 4) == [True, False, False, False]
    # the same new song twice, beside one the index holds and one it does not: in any order of the pairs
    assert keep(pairs((6, 8), (0, 5)), 5, 4) == [False, True, True, False]
    assert keep(pairs((0, 5), (6, 8)), 5, 4) == [False, True, True, False]
    # a file that pairs with a dropped file and with a kept one
    assert keep(pairs((0, 5), (5, 7), (6, 7)), 5, 3) == [False, True, False]
    # an empty index
    assert keep(pairs((0, 1), (0, 2), (1, 2)), 0, 3) == [True, False, False]
    # records of the binding as well as tuples
    rec = np.array([(2, 5, 0, 9, 0, 0), (5, 6, 0, 9, 0, 0)], _lib.DUP_PAIR_DTYPE)
    assert keep([(int(p["a"]), int(p["b"])) for p in rec], 5, 2) == [False, True]
    for bad in ((5, 5), (6, 5), (0, 4), (0, 7), (-1, 5)):
        with pytest.raises(ValueError):
            keep(pairs(bad), 5, 2)


def test_refused_before_any_file_is_read():
    sharded = hpfw_amd.LiveSongIdentification.__new__(hpfw_amd.LiveSongIdentification)
    sharded._gpu = object.__new__(liveid._ShardedIndex)
    for call in (lambda r: sharded.known(["/nonexistent.wav"], r, 100), lambda r: sharded.add_new(["/nonexistent.wav"], r, 100)):
        with pytest.raises(hpfw_amd.HpfwError) as e:
            call(65)
        assert e.value.status == E_INVALID
        with pytest.raises(hpfw_amd.HpfwError) as e:
            call(16)
        assert e.value.status == E_UNSUPPORTED


def test_pass_plan_under_sanitizers(tmp_path):
    """join_plan.h is plain C++: the passes of the three joins for 0 to 70 clips and recordings, both entry sizes, tables
    that force 1, 2, 3 and many passes and forced splits -- the plan's properties and the formulas the joins had before
    the header, in a program of its own under ASan and UBSan"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "join_plan_check"
    src = os.path.join(ROOT, "tests", "emu", "join_plan_check.cpp")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "join_plan_check ok" in r.stdout


FACADE = r"""
#include <hpfw/gpu/gpu_collector.h>
#include <hpfw/gpu/gpu_storage.h>
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    hpfw::db::GpuStorage<hpfw::GpuCollector> storage;
    std::vector<hpfw::GpuCollector::FilenameFingerprintPair> batch;
    auto pairs = storage.join(batch, 100, 16, 1, true);
    if (pairs.empty()) return 0;
    return (int)(pairs[0].dist + pairs[0].overlap + (size_t)pairs[0].lag + pairs[0].name_a.size() + pairs[0].name_b.size());
}
"""


def test_join_facade_compiles_and_links(tmp_path):
    src = tmp_path / "join.cpp"
    src.write_text(FACADE)
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(tmp_path / "join"), "-L", lib_dir, "-lhpfw_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "join")], capture_output=True, text=True)         # no argument: no device touched
    assert r.returncode == 2
