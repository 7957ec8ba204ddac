"""CPU tests of the search within sets of clips: the new symbols are declared, exported and bound, the
set arguments have no default, every refusal of the rule happens before a device is touched, the identifier's refusals and
KeyErrors need no device, names become sorted live slots, the restatement (within_ref.py) agrees with a bit-by-bit loop and
with the oracle on the whole index, and the C++ facade compiles and links."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib

import within_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
SYMS = ("hpfw_gpu_search_topk_within_device", "hpfw_gpu_search_topk_within", "hpfw_gpu_search_topk_transposed_within_device",
        "hpfw_gpu_search_topk_transposed_within")


def test_entry_points_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "hpfw_gpu.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = hpfw_amd.lib()
    for sym in SYMS:
        m = re.search(r"\b" + sym + r"\s*\(([^;]*)\)\s*;", header)
        assert m, sym
        assert "=" not in m.group(1)                                                   # C: no default anywhere
        assert sym in _lib.EXPORTS and hasattr(L, sym)
        assert len(getattr(L, sym).argtypes) == len(m.group(1).split(",")), sym          # the binding has the declaration's arity
        for arg in ("set_off", "n_sets", "set_clips", "q_set"):
            assert re.search(r"\b" + arg + r"\b", m.group(1)), (sym, arg)
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in ("STRICTLY ASCENDING inside a set", "an index that holds only the clips of set s", "gets the bytes of the unrestricted call"):
        assert phrase in flat, phrase
    for f in (_lib.Gpu.search_topk_within, _lib.Gpu.search_topk_within_dev, _lib.Gpu.search_topk_transposed_within,
              _lib.Gpu.search_topk_transposed_within_dev):
        for arg in ("set_off", "set_clips", "q_set"):
            assert inspect.signature(f).parameters[arg].default is inspect.Parameter.empty, (f, arg)
    for f in (hpfw_amd.LiveSongIdentification.top, hpfw_amd.LiveSongIdentification.timeline, hpfw_amd.LiveSongIdentification.streams):
        assert inspect.signature(f).parameters["within"].default is None
    for f in (hpfw_amd.LiveSongIdentification.top_overlap, hpfw_amd.LiveSongIdentification.top_votes,
              hpfw_amd.LiveSongIdentification.top_warped, hpfw_amd.LiveSongIdentification.duplicates,
              hpfw_amd.LiveSongIdentification.known):
        assert "within" not in inspect.signature(f).parameters
    facade = open(os.path.join(ROOT, "include", "hpfw", "gpu", "timeline.h")).read()
    assert re.search(r"std::vector<std::optional<std::vector<int32_t>>> within;", facade)
    sharded = open(os.path.join(ROOT, "include", "hpfw", "gpu", "sharded_storage.h")).read()
    assert "find_within" not in sharded


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_bad_arguments_are_refused_without_a_device():
    """the handle here is a buffer of zeros: a call that got as far as using it would not return a status"""
    L = hpfw_amd.lib()
    buf = np.zeros(64, np.int64)
    one = _p(buf)
    i32 = lambda *v: np.array(v, np.int32)
    i64 = lambda *v: np.array(v, np.int64)

    def all4(h=one, q=one, q_off=i64(0, 4, 8), n_q=2, k=1, set_off=i64(0, 2, 3), n_sets=2, set_clips=i32(0, 5, 2), q_set=i32(0, -1),
             out=one, stats=one):
        """the status and message of the four entry points (the transposed ones with n_shifts = 1), which must agree"""
        a = (_p(set_off), n_sets, _p(set_clips), _p(q_set))
        rcs = []
        for call in (lambda: L.hpfw_gpu_search_topk_within(h, q, _p(q_off), n_q, k, *a, out, stats),
                     lambda: L.hpfw_gpu_search_topk_within_device(h, q, _p(q_off), n_q, k, *a, out, stats, None),
                     lambda: L.hpfw_gpu_search_topk_transposed_within(h, q, _p(q_off), n_q, 1, k, *a, out, stats),
                     lambda: L.hpfw_gpu_search_topk_transposed_within_device(h, q, _p(q_off), n_q, 1, k, *a, out, stats, None)):
            rcs.append((call(), L.hpfw_gpu_last_error()))
        assert len({rc for rc, _ in rcs}) == 1, rcs
        return rcs[0]

    for kw in (dict(h=None), dict(q_off=None), dict(out=None), dict(n_q=-1)):
        assert all4(**kw)[0] == E_INVALID, kw
    for k in (0, -1, 65):
        assert all4(k=k)[0] == E_INVALID
    rc, msg = all4(n_sets=-1)
    assert rc == E_INVALID and b"n_sets" in msg
    rc, msg = all4(set_off=None)
    assert rc == E_INVALID and b"null set_off" in msg
    rc, msg = all4(set_off=i64(1, 2, 3))
    assert rc == E_INVALID and b"set_off[0]" in msg
    rc, msg = all4(set_off=i64(0, 3, 2))
    assert rc == E_INVALID and b"must not decrease" in msg
    rc, msg = all4(set_clips=None)
    assert rc == E_INVALID and b"null set_clips" in msg
    for clips in (i32(5, 0, 2), i32(3, 3, 2), i32(-1, 5, 2), i32(0, 5, -2)):           # descending, repeated, negative
        rc, msg = all4(set_clips=clips)
        assert rc == E_INVALID and b"strictly ascending" in msg, clips
    rc, msg = all4(q_set=None)
    assert rc == E_INVALID and b"null q_set" in msg
    for qs in (i32(0, -2), i32(2, 0), i32(0, 7)):
        rc, msg = all4(q_set=qs)
        assert rc == E_INVALID and b"q_set" in msg, qs
    rc, msg = all4(n_sets=0, set_off=None, set_clips=None, q_set=i32(0, -1))                # no sets: only -1 is a set
    assert rc == E_INVALID and b"q_set" in msg
    rc, msg = all4(q_off=i64(0, 8, 4))
    assert rc == E_INVALID and b"non-decreasing" in msg
    rc, msg = all4(q_off=i64(0, 4, 16005))
    assert rc == E_UNSUPPORTED and b"16000" in msg
    rc, msg = all4(q_off=i64(0, 16005, 10))                   # both faults: the first faulty query's is reported
    assert rc == E_UNSUPPORTED and b"16000" in msg
    # the transposed forms refuse a bad n_shifts as the unrestricted ones do
    a = (_p(i64(0, 2, 3)), 2, _p(i32(0, 5, 2)), _p(i32(0, -1)))
    for n_shifts in (0, -1, 65):
        assert L.hpfw_gpu_search_topk_transposed_within(one, one, _p(i64(0, 4, 8)), 2, n_shifts, 1, *a, one, one) == E_INVALID
        assert L.hpfw_gpu_search_topk_transposed_within_device(one, one, _p(i64(0, 4, 8)), 2, n_shifts, 1, *a, one, one, None) == E_INVALID
    # q_set has one entry per query, not per variant: 2 queries of 2 variants read 2 entries (the third would be refused)
    qs3 = i32(0, -1, 9)
    rc = L.hpfw_gpu_search_topk_transposed_within(one, one, _p(i64(0, 4, 8, 8, 4)), 2, 2, 1, _p(i64(0, 2, 3)), 2, _p(i32(0, 5, 2)), _p(qs3), one, one)
    assert rc == E_INVALID and b"non-decreasing" in L.hpfw_gpu_last_error()


def test_gpu_wrappers_check_their_arrays():
    g = _lib.Gpu.__new__(_lib.Gpu)
    g._h = None
    q, off = np.zeros(8, np.uint64), np.array([0, 4, 8])
    with pytest.raises(ValueError):
        g.search_topk_within(q, off, 1, [0, 1], [0], [0])                               # one q_set entry for two queries
    with pytest.raises(ValueError):
        g.search_topk_within(q, off, 1, [0, 3], [0], [0, 0])                            # set_clips shorter than set_off says
    with pytest.raises(ValueError):
        g.search_topk_transposed_within(q, off, 2, 1, [0, 1], [0], [0, 0])              # one query of two variants
    with pytest.raises(hpfw_amd.HpfwError) as e:                                        # the null handle is the library's to refuse
        g.search_topk_within(q, off, 1, [0, 1], [0], [0, -1])
    assert e.value.status == E_INVALID


def _identifier(names, removed=()):
    lsi = hpfw_amd.LiveSongIdentification.__new__(hpfw_amd.LiveSongIdentification)
    lsi._gpu = object()
    lsi.names = list(names)
    lsi._removed = set(removed)
    return lsi


def test_names_become_sorted_live_slots():
    lsi = _identifier(["a", "b", "c", "b", "d", "a"], removed={3, 4})
    assert lsi._within_slots(["c", "a"]) == [0, 2, 5]
    assert lsi._within_slots(["b", "b", "a"]) == [0, 1, 5]                             # unique, the removed slot 3 left out
    assert lsi._within_slots([]) == []
    for bad in (["d"], ["a", "zz"]):                                                   # removed, unknown
        with pytest.raises(KeyError):
            lsi._within_slots(bad)
    so, sc, qs = lsi._one_set(["c", "a"], 3)
    assert so.tolist() == [0, 3] and sc.tolist() == [0, 2, 5] and qs.tolist() == [0, 0, 0] and sc.dtype == np.int32
    assert lsi._one_set(None, 3) is None


def test_identifier_refusals_need_no_device():
    """within with min_overlap, within on a sharded identifier, and an unknown or removed name are refused before the
    collector or a device is asked for anything: the identifier here has neither"""
    lsi = _identifier(["a", "b", "c"], removed={1})
    for call in (lambda: lsi.timeline("x.wav", 10.0, min_overlap=100, within=["a"]),
                 lambda: lsi.streams(2, 10.0, min_overlap=100, within=["a"])):
        with pytest.raises(hpfw_amd.HpfwError) as e:
            call()
        assert e.value.status == _lib.E_UNSUPPORTED
    for within in (["b"], ["a", "nope"]):
        for call in (lambda: lsi.top(["x.wav"], 1, within=within), lambda: lsi.top(["x.wav"], 1, shifts=[0, 2], within=within),
                     lambda: lsi.top(["x.wav"], 1, tempos=[1.0], within=within), lambda: lsi.timeline("x.wav", 10.0, within=within),
                     lambda: lsi.streams(2, 10.0, within=within), lambda: lsi.streams(2, 10.0, within=[["a"], within]),
                     lambda: lsi.streams(2, 10.0, within=[None, within])):
            with pytest.raises(KeyError):
                call()
    with pytest.raises(ValueError):
        lsi.streams(3, 10.0, within=[["a"], None])                                     # three feeds, two entries
    lsi._gpu = object.__new__(hpfw_amd.liveid._ShardedIndex)
    for call in (lambda: lsi.top(["x.wav"], 1, within=["a"]), lambda: lsi.timeline("x.wav", 10.0, within=["a"]),
                 lambda: lsi.streams(2, 10.0, within=["a"])):
        with pytest.raises(hpfw_amd.HpfwError) as e:
            call()
        assert e.value.status == _lib.E_UNSUPPORTED


def _small_index(rng):
    lengths = [0, 1, 2, 3, 5, 8, 4, 7, 8, 6]
    clips = [rng.integers(0, 4, n).astype(np.uint64) * np.uint64(0x8000000000000001) for n in lengths]   # few words: ties abound
    clips[7] = rng.integers(0, 2 ** 64, 7, dtype=np.uint64)
    clips[6][:] = clips[5][2:6]                                                         # (one clip is part of another)
    clips[8][:] = clips[5]                                                              # (and one repeats another: a tie on every query)
    return _lib._ragged(clips, np.uint64)


def test_restatement_equals_a_bit_by_bit_loop(oracle):
    rng = np.random.default_rng(2401)
    db_hp, db_off = _small_index(rng)
    sets = [[], [5], [0, 2, 4, 6, 8], list(range(10)), [9], [5, 8], [0, 1], [1, 5, 6]]
    set_off = np.concatenate([[0], np.cumsum([len(s) for s in sets])])
    set_clips = np.array([c for s in sets for c in s], np.int64)
    queries = [db_hp[db_off[5] + 1:db_off[5] + 4], rng.integers(0, 2 ** 64, 1, dtype=np.uint64), db_hp[db_off[5]:db_off[6]],
               rng.integers(0, 4, 10).astype(np.uint64) * np.uint64(0x8000000000000001)]
    for k in (1, 3, 12):
        for s in range(-1, len(sets)):
            q_off = np.concatenate([[0], np.cumsum([q.size for q in queries])])
            q_set = np.full(len(queries), s)
            got = ref.search_within(oracle, db_hp, db_off, np.concatenate(queries), q_off, k, set_off, set_clips, q_set, clip_base=100)
            mom = ref.moments_within(oracle, db_hp, db_off, np.concatenate(queries), q_off, set_off, set_clips, q_set)
            clips = range(10) if s < 0 else sets[s]
            for q, row, m in zip(queries, got, mom):
                want = ref.brute_force(db_hp, db_off, q, clips, k, clip_base=100)
                assert [(int(h["dist"]), int(h["clip"]), int(h["offset"])) for h in row] == want, (k, s)
                every = ref.brute_force(db_hp, db_off, q, clips, 10)
                d = [dd for dd, c, _ in every if c != ref.NONE and db_off[c + 1] - db_off[c] >= q.size]
                assert m == (len(d), sum(d), sum(x * x for x in d)), (k, s)


def test_restatement_with_every_clip_is_the_oracle(oracle):
    rng = np.random.default_rng(2402)
    db_hp, db_off = _small_index(rng)
    queries = [rng.integers(0, 4, n).astype(np.uint64) * np.uint64(0x8000000000000001) for n in (1, 3, 6, 9)]
    q_off = np.concatenate([[0], np.cumsum([q.size for q in queries])])
    for k in (1, 4, 64):
        want = oracle.search_topk(db_hp, db_off, np.concatenate(queries), q_off, k)
        for q_set in (np.zeros(4, np.int64), np.full(4, -1), np.array([0, -1, 0, -1])):
            got = ref.search_within(oracle, db_hp, db_off, np.concatenate(queries), q_off, k, [0, 10], np.arange(10), q_set)
            assert got.tobytes() == want.tobytes()


def test_restatement_refuses_what_the_rule_refuses():
    ok = dict(set_off=[0, 2, 3], set_clips=[0, 5, 2], q_set=[0, -1], n_q=2, n_slots=6)
    ref.check_sets(**ok)
    for kw in (dict(set_off=[1, 2, 3]), dict(set_off=[0, 3, 2]), dict(set_clips=[5, 0, 2]), dict(set_clips=[0, 0, 2]), dict(set_clips=[-1, 0, 2]),
               dict(q_set=[0, 2]), dict(q_set=[0, -2]), dict(q_set=[0]), dict(n_slots=5)):
        with pytest.raises(ValueError):
            ref.check_sets(**{**ok, **kw})


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
    auto hits = storage.find_within(hp, 3, {0, 2});
    auto scored = storage.find_within_scored(hp, 3, {0, 2});
    hpfw::TimelineOptions opt;
    opt.min_score = 10;
    opt.within = {std::vector<int32_t>{0, 2}};
    auto tl = hpfw::timeline(storage, storage.handle(), argv[1], opt);
    hpfw::LiveStreamsOptions lo;
    lo.min_score = 10;
    lo.within = {std::vector<int32_t>{0, 2}, std::nullopt};
    hpfw::LiveStreams<hpfw::db::GpuStorage<hpfw::GpuCollector>> live(storage, storage.handle(), 2, lo);
    auto segs = live.push({});
    auto rest = live.finish();
    return (int)(hits.size() + scored.size() + tl.segments.size() + segs.size() + rest.size()) + (scored.empty() ? 0 : (int)scored[0].score);
}
"""


def test_facade_compiles_and_links(tmp_path):
    src = tmp_path / "within_facade.cpp"
    src.write_text(FACADE)
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(tmp_path / "within_facade"), "-L", lib_dir, "-lhpfw_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "within_facade")], capture_output=True, text=True)   # no argument: no device touched
    assert r.returncode == 2
