"""CPU tests of index maintenance: the entry points are declared and exported, every refusal happens
before a device is touched, and the plan of a removal (hpfw_amd/csrc/index_plan.h), executed pessimistically in numpy,
gives what tests/index_ref.py states -- for every subset of every small ragged index, at several chunk sizes."""
import ctypes
import itertools
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib

import index_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
SYMS = ("hpfw_gpu_index_remove", "hpfw_gpu_index_reserve", "hpfw_gpu_index_capacity", "hpfw_gpu_index_remove_plan",
        "hpfw_gpu_index_remove_geometry")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_entry_points_are_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hpfw_gpu.h")).read(), flags=re.S)
    for sym in SYMS:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTS and hasattr(hpfw_amd.lib(), sym)
    assert re.search(r"\}\s*hpfw_index_move\s*;", header)
    assert _lib.INDEX_MOVE_DTYPE.itemsize == 40 and _lib.INDEX_MOVE_DTYPE.names == ("dst", "src", "len", "chunk", "staged", "pad")
    for name in ("index_remove", "index_reserve", "index_capacity"):
        assert callable(getattr(_lib.Gpu, name))
    makefile = open(os.path.join(ROOT, "hpfw_amd", "csrc", "Makefile")).read()
    assert " k_index.hip " in makefile and " index_plan.h " in makefile
    tile, chunk = ctypes.c_int64(0), ctypes.c_int64(0)
    assert hpfw_amd.lib().hpfw_gpu_index_remove_geometry(ctypes.byref(tile), ctypes.byref(chunk)) == 0
    assert tile.value >= 2 and tile.value % 2 == 0 and chunk.value >= tile.value
    assert hpfw_amd.lib().hpfw_gpu_index_remove_geometry(None, ctypes.byref(chunk)) == E_INVALID
    # the kernels hold none of the forms the issue forbids
    kernel = open(os.path.join(ROOT, "hpfw_amd", "csrc", "k_index.hip")).read()
    code = re.sub(r"//[^\n]*", "", kernel)
    assert "atomic" not in code and "asm" not in code and "__syncthreads" not in code


def test_sharded_entry_point_is_declared_and_exported():
    from hpfw_amd import multi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hpfw_gpu_multi_index.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(hpfw_gpu_(?:group|shard)_\w+)\s*\(", header))
    assert declared == set(multi.INDEX_EXPORTS) == {"hpfw_gpu_group_index_remove"}
    assert all(hasattr(multi.lib(), s) for s in declared)
    assert callable(multi.GpuGroup.index_remove)
    assert "out of scope" in open(os.path.join(ROOT, "include", "hpfw_gpu_multi_index.h")).read()


def test_bad_arguments_are_refused_without_a_device():
    """the handle here is a buffer of zeros (an index of no clips, not even the leading offset): a call that got as far as
    using it would not return a status"""
    L = hpfw_amd.lib()
    buf = np.zeros(4096, np.int64)
    h = _p(buf)
    ids = np.array([0, 1], np.int64)
    for args in ((None, _p(ids), 2, None), (h, _p(ids), -1, None), (h, None, 2, None)):
        assert L.hpfw_gpu_index_remove(*args) == E_INVALID, args
    rc = L.hpfw_gpu_index_remove(h, _p(ids), 2, None)          # no clip: every id is outside
    assert rc == E_INVALID and b"outside" in L.hpfw_gpu_last_error()
    assert L.hpfw_gpu_index_remove(h, _p(np.array([-1], np.int64)), 1, None) == E_INVALID
    assert not buf.any()
    assert L.hpfw_gpu_index_reserve(None, 8) == E_INVALID and L.hpfw_gpu_index_reserve(h, -1) == E_INVALID
    assert L.hpfw_gpu_index_reserve(h, 0) == 0 and L.hpfw_gpu_index_capacity(h) == 0 and L.hpfw_gpu_index_capacity(None) == 0
    assert not buf.any()
    # the plan: null arrays, a decreasing offset, ids that do not ascend strictly or lie outside, chunk < 1, too small a cap
    off = np.array([0, 2, 5], np.int64)
    new = np.zeros(3, np.int64)
    n = ctypes.c_int64(0)
    moves = np.zeros(4, _lib.INDEX_MOVE_DTYPE)

    def plan(o=off, rem=(0,), chunk=4, out=new, mv=moves, cap=4, count=n):
        r = np.array(rem, np.int64)
        return L.hpfw_gpu_index_remove_plan(None if o is None else _p(o), o.size - 1 if o is not None else 2, _p(r) if r.size else None, r.size,
                                            chunk, None if out is None else _p(out), None if mv is None else _p(mv), cap,
                                            None if count is None else ctypes.byref(count))

    assert plan() == 0 and n.value == 1 and list(new) == [0, 0, 3]
    assert (moves[0]["dst"], moves[0]["src"], moves[0]["len"], moves[0]["chunk"], moves[0]["staged"]) == (0, 2, 3, 0, 1)
    assert plan(mv=None) == 0 and n.value == 1
    for kw in (dict(o=None), dict(out=None), dict(count=None), dict(o=np.array([0, 3, 2], np.int64)), dict(rem=(1, 1)), dict(rem=(1, 0)),
               dict(rem=(2,)), dict(rem=(-1,)), dict(chunk=0), dict(cap=0)):
        assert plan(**kw) == E_INVALID, kw


def _plan(off, removed, chunk, new_off, moves):
    n = ctypes.c_int64(0)
    rc = hpfw_amd.lib().hpfw_gpu_index_remove_plan(_p(off), off.size - 1, _p(removed) if removed.size else None, removed.size, chunk,
                                                   _p(new_off), _p(moves), moves.size, ctypes.byref(n))
    assert rc == 0
    return moves[:n.value].tolist()                               # (dst, src, len, chunk, staged, pad)


def test_plan_against_the_rule_for_every_small_index():
    """every subset of the clips of every ragged index of at most 6 clips of 0 to 3 hashprints, at chunk sizes 1, 2, 3 and 7.
    The executor is pessimistic: chunks in order; a staged chunk is read whole, then written; inside a direct chunk the
    elements move in a random order, after the assertion that its sources and destinations are disjoint."""
    rng = random.Random(2101)
    moves = np.zeros(64, _lib.INDEX_MOVE_DTYPE)
    n_cases = n_direct = n_staged = 0
    for n_clips in range(7):
        new_off = np.zeros(n_clips + 1, np.int64)
        for lengths in itertools.product(range(4), repeat=n_clips):
            off = np.concatenate([[0], np.cumsum(lengths, dtype=np.int64)]).astype(np.int64)
            total = int(off[-1])
            hp = ref.mixed(total, seed=n_clips)
            hp_list = hp.tolist()
            for r in range(n_clips + 1):
                for subset in itertools.combinations(range(n_clips), r):
                    removed = np.array(subset, np.int64)
                    want_hp, want_off = ref.remove(hp, off, subset)
                    want_hp, first_removed = want_hp.tolist(), int(off[subset[0]]) if subset else total
                    for chunk in (1, 2, 3, 7):
                        mv = _plan(off, removed, chunk, new_off, moves)
                        assert new_off.tolist() == want_off.tolist(), (lengths, subset, chunk)
                        buf = list(hp_list)
                        shift = 0
                        for k, pieces in itertools.groupby(mv, key=lambda m: m[3]):
                            pieces = list(pieces)
                            lo, hi = pieces[0][0], pieces[-1][0] + pieces[-1][2]
                            assert hi - lo <= chunk and all(p[4] == pieces[0][4] for p in pieces)
                            pairs = []
                            for dst, src, length, _, staged, _ in pieces:
                                assert length > 0 and dst >= first_removed and src - dst >= max(shift, 1), (lengths, subset, chunk, mv)
                                shift = src - dst
                                pairs += [(dst + i, src + i) for i in range(length)]
                            assert [d for d, _ in pairs] == list(range(lo, hi)), (lengths, subset, chunk, mv)   # adjacent, ascending
                            if pieces[0][4]:
                                staged = [buf[s] for _, s in pairs]                   # read whole ...
                                buf[lo:hi] = staged                                   # ... then written
                                n_staged += 1
                            else:
                                assert min(s for _, s in pairs) >= hi, (lengths, subset, chunk, mv)    # sources and destinations disjoint
                                rng.shuffle(pairs)
                                for d, s in pairs:
                                    buf[d] = buf[s]
                                n_direct += 1
                        assert buf[:len(want_hp)] == want_hp, (lengths, subset, chunk, mv)
                        n_cases += 1
    assert n_cases == 4 * sum(8 ** c for c in range(7)) and n_direct > 1000 and n_staged > 1000


def test_plan_under_sanitizers(tmp_path):
    """index_plan.h is plain C++: the same enumeration against a plain loop, the refusals and positions beyond 2^32 in a
    program of its own under ASan and UBSan"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "index_plan_check"
    src = os.path.join(ROOT, "tests", "emu", "index_plan_check.cpp")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "index_plan_check ok" in r.stdout


FACADE = r"""
#include <hpfw/gpu/gpu_collector.h>
#include <hpfw/gpu/gpu_storage.h>
#include <hpfw/gpu/sharded_storage.h>
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    using Pair = hpfw::GpuCollector::FilenameFingerprintPair;
    hpfw::db::GpuStorage<hpfw::GpuCollector> storage;
    std::vector<Pair> more;
    storage.add(more);
    size_t n = storage.remove({"a", "b"}) + storage.live() + storage.size() + storage.names().size() + (size_t)storage.added_length(0);
    storage.save(std::nullopt);
    hpfw::db::ShardedGpuStorage<hpfw::GpuCollector> sharded;
    n += sharded.remove({"a"}) + sharded.live() + sharded.size() + sharded.index_offsets().size();
    return (int)n;
}
"""


def test_facades_compile_and_link(tmp_path):
    src = tmp_path / "maintain.cpp"
    src.write_text(FACADE)
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(tmp_path / "maintain"), "-L", lib_dir, "-lhpfw_gpu_multi", "-lhpfw_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "maintain")], capture_output=True, text=True)   # no argument: no device touched
    assert r.returncode == 2


class _StubIndex:
    """what LiveSongIdentification asks of its index handle, recorded"""

    def __init__(self):
        self.calls = []

    def index_clear(self):
        self.calls.append(("clear",))

    def index_add(self, hp, off):
        self.calls.append(("add", int(np.asarray(off).size) - 1))

    def index_remove(self, ids):
        self.calls.append(("remove", list(ids)))


def _stub_identifier(index):
    lsi = hpfw_amd.LiveSongIdentification.__new__(hpfw_amd.LiveSongIdentification)
    lsi._gpu = index
    lsi.names = []
    return lsi


def test_identifier_remove_bookkeeping():
    index = _StubIndex()
    lsi = _stub_identifier(index)
    pairs = [(np.arange(n, dtype=np.uint64), name) for n, name in ((5, "a"), (7, "b"), (3, "a"), (0, "c"), (9, "d"))]
    lsi.build(pairs)
    assert lsi.names == ["a", "b", "a", "c", "d"] == lsi.live_names()
    n_calls = len(index.calls)
    for bad in (["x"], ["b", "x"], ["a", "b", "nope", "d"]):               # KeyError before any change
        with pytest.raises(KeyError):
            lsi.remove(bad)
        assert len(index.calls) == n_calls and lsi.live_names() == lsi.names
    assert lsi.remove(["a", "d", "a"]) == 3                                # every live slot of a name, a repeated name once
    assert index.calls[-1] == ("remove", [0, 2, 4]) and len(index.calls) == n_calls + 1
    assert lsi.names == ["a", "b", "a", "c", "d"] and lsi.live_names() == ["b", "c"]
    for bad in (["a"], ["b", "d"]):                                        # already removed: unknown
        with pytest.raises(KeyError):
            lsi.remove(bad)
        assert len(index.calls) == n_calls + 1 and lsi.live_names() == ["b", "c"]
    with pytest.raises(KeyError):
        lsi._no_shards = lambda what: None
        lsi.warp_path("q.wav", "a")                                        # ... to warp_path too (before the file is read)
    assert lsi.remove([]) == 0 and len(index.calls) == n_calls + 1
    assert lsi.remove(["c"]) == 1 and index.calls[-1] == ("remove", [3]) and lsi.live_names() == ["b"]
    assert lsi._added_len == [5, 7, 3, 0, 9]                               # the lengths as added, which _trim reads
    lsi.build(pairs[:3])                                                   # a fresh index forgets all removals
    assert lsi.live_names() == ["a", "b", "a"] and lsi.remove(["a"]) == 2 and index.calls[-1] == ("remove", [0, 2])
    # a sharded identifier removes through the group and refuses add before anything is read
    sharded = _stub_identifier(object.__new__(hpfw_amd.liveid._ShardedIndex))
    with pytest.raises(hpfw_amd.HpfwError) as e:
        sharded.add(["x.wav"])
    assert e.value.status == _lib.E_UNSUPPORTED
    assert "index_remove" in open(os.path.join(ROOT, "hpfw_amd", "liveid.py")).read().split("class LiveSongIdentification")[0]
