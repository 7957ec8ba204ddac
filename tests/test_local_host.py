"""CPU tests of the local search: the entry points are declared and exported, every refusal happens
before a device is touched, the restatement of tests/local_ref.py against enumeration of every run, its tie order, an exact
excerpt, and the half-shared query the rule was made for, on the oracle's hashprints."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, synth

import local_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
SYMS = ("hpfw_gpu_search_local_device", "hpfw_gpu_search_local")


def test_entry_points_are_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hpfw_gpu.h")).read(), flags=re.S)
    for sym in SYMS:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTS and hasattr(hpfw_amd.lib(), sym)
    assert re.search(r"\}\s*hpfw_local_hit\s*;", header)
    assert _lib.LOCAL_HIT_DTYPE.itemsize == 24 and _lib.LOCAL_HIT_DTYPE == ref.LOCAL_HIT_DTYPE and hpfw_amd.LOCAL_HIT_DTYPE is _lib.LOCAL_HIT_DTYPE
    assert _lib.LOCAL_HIT_DTYPE.names == ("score", "clip", "lag", "q_start", "length", "dist")
    # max_rate has no default in any binding
    for f in (_lib.Gpu.search_local, _lib.Gpu.search_local_dev, hpfw_amd.LiveSongIdentification.top_local):
        assert inspect.signature(f).parameters["max_rate"].default is inspect.Parameter.empty
    # a sharded identifier has no local search
    sharded = hpfw_amd.LiveSongIdentification.__new__(hpfw_amd.LiveSongIdentification)
    sharded._gpu = object.__new__(hpfw_amd.liveid._ShardedIndex)
    with pytest.raises(hpfw_amd.HpfwError) as e:
        sharded.top_local(["a.wav"], 1, 22)
    assert e.value.status == E_UNSUPPORTED
    facade = open(os.path.join(ROOT, "include", "hpfw", "gpu", "gpu_storage.h")).read()
    assert re.search(r"find_local\(const typename Collector::Hashprint &hp, int k, int max_rate\)", facade)
    kernels = open(os.path.join(ROOT, "hpfw_amd", "csrc", "kernels.h")).read()
    for launch in ("launch_local_mfma", "launch_local_popc", "launch_local_ends"):
        assert re.search(r"void " + launch + r"\(", kernels), launch


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_bad_arguments_are_refused_without_a_device():
    """the handle here is a buffer of zeros: a call that got as far as using it would not return a status"""
    L = hpfw_amd.lib()
    buf = np.zeros(64, np.int64)
    one = _p(buf)
    off = np.array([0, 4, 8], np.int64)

    def both(h=one, q=one, q_off=off, n_q=2, rate=22, k=1, out=one):
        qo = None if q_off is None else _p(q_off)
        rcs = []
        for rc in (L.hpfw_gpu_search_local(h, q, qo, n_q, rate, k, out), L.hpfw_gpu_search_local_device(h, q, qo, n_q, rate, k, out, None)):
            rcs.append((rc, L.hpfw_gpu_last_error()))
        assert rcs[0][0] == rcs[1][0], rcs
        return rcs[0]

    for kw in (dict(h=None), dict(q_off=None), dict(out=None), dict(n_q=-1), dict(q=None)):
        assert both(**kw)[0] == E_INVALID, kw
    for k in (0, -1, 65):
        rc, msg = both(k=k)
        assert rc == E_INVALID and b"k must be in 1..64" in msg
    for rate in (0, -3, 32, 64):
        rc, msg = both(rate=rate)
        assert rc == E_INVALID and b"max_rate must be in 1..31" in msg
    rc, msg = both(q_off=np.array([0, 8, 4], np.int64))
    assert rc == E_INVALID and b"non-decreasing" in msg
    rc, msg = both(q_off=np.array([0, 4, 16005], np.int64))
    assert rc == E_UNSUPPORTED and b"16000" in msg
    rc, msg = both(q_off=np.array([0, 16005, 10], np.int64))  # both faults: the order is reported
    assert rc == E_INVALID and b"non-decreasing" in msg


def test_query_group_plan_under_sanitizers(tmp_path):
    """search_plan.h is plain C++: the queries of one pass of the plain, overlap and local searches for a sweep of queries,
    clips, splits and tables against the formulas the searches had before the header, a table switch's properties, and the
    groups' lengths -- in a program of its own under ASan and UBSan"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "search_plan_check"
    src = os.path.join(ROOT, "tests", "emu", "search_plan_check.cpp")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "search_plan_check ok" in r.stdout


def test_restatement_equals_enumeration_of_all_runs():
    rng = np.random.default_rng(2501)
    n_cases = n_hits = 0
    for k in range(1, 7):
        for n in range(0, 9):
            for rep in range(4):
                # few distinct words: equal scores at several lags and ends are common
                q = rng.integers(0, 4, k).astype(np.uint64) * np.uint64(0x8000000000000001)
                r = rng.integers(0, 4, n).astype(np.uint64) * np.uint64(0x8000000000000001)
                if rep == 2:                             # sparse words: every rate of a hashprint from 0 to a few bits
                    q = np.uint64(1) << rng.integers(0, 4, k).astype(np.uint64)
                    r = np.uint64(1) << rng.integers(0, 4, n).astype(np.uint64)
                if rep == 3:
                    q, r = rng.integers(0, 2 ** 64, k, dtype=np.uint64), rng.integers(0, 2 ** 64, n, dtype=np.uint64)
                for T in (1, 2, 16, 31):
                    want = ref.enumerate_candidate(q, r, T)
                    assert ref.clip_candidate(q, r, T) == want, (q, r, T)
                    assert np.array_equal(ref.lag_scores_by_steps(q, r, T), ref.lag_scores(q, r, T)), (q, r, T)   # (its form for long queries)
                    n_cases += 1
                    n_hits += want is not None
    assert n_cases == 6 * 9 * 4 * 4 and n_hits > n_cases // 3


def _search(clips, queries, top_k, T, **kw):
    db_hp, db_off = _lib._ragged([np.asarray(c, np.uint64) for c in clips], np.uint64)
    q_hp, q_off = _lib._ragged([np.asarray(q, np.uint64) for q in queries], np.uint64)
    return ref.search_local(db_hp, db_off, q_hp, q_off, top_k, T, **kw)


def _rows(got):
    return [tuple(int(v) for v in h) for h in got]


def test_tie_order():
    ones = np.uint64(0xFFFFFFFFFFFFFFFF)
    a, b, c = (np.uint64(v) for v in (0x0123456789ABCDEF, 0x0F1E2D3C4B5A6978, 0x13579BDF02468ACE))
    # the passage (a, b) lies at two lags of the clip: the smaller lag wins
    clip = np.array([c, a, b, ~c, a, b, c], np.uint64)
    assert _rows(_search([clip], [[a, b]], 1, 8)[0]) == [(16, 0, 1, 0, 2, 0)]
    # two runs of one diagonal with the same score: the one that ends first; an all-mismatch hashprint (x = 8 - 64) parts them
    d, e = np.uint64(0x2468ACE013579BDF), np.uint64(0x0FEDCBA987654321)
    q = np.array([a, b, c, d, e], np.uint64)
    r = np.array([a, b, ~c, d, e], np.uint64)
    assert _rows(_search([r], [q], 1, 8)[0]) == [(16, 0, 0, 0, 2, 0)]
    # the same end, two starts: a hashprint with exactly T mismatching bits adds 0, and the run without it starts later --
    # the smaller j0 wins, as the prefix minimum moves on strict < only
    r = np.array([a ^ np.uint64(0xFF), b, c], np.uint64)
    assert _rows(_search([r], [np.array([a, b, c], np.uint64)], 1, 8)[0]) == [(16, 0, 0, 0, 3, 8)]
    # ... and at the end of a run the shorter one: smaller j1
    r = np.array([a, b, c ^ np.uint64(0xFF)], np.uint64)
    assert _rows(_search([r], [np.array([a, b, c], np.uint64)], 1, 8)[0]) == [(16, 0, 0, 0, 2, 0)]
    # two clips with equal content: the smaller id wins; a reversed clip scores less; clip_base
    r = np.arange(1, 9, dtype=np.uint64) * a
    got = _search([r[::-1].copy(), r, r], [r[2:6]], 3, 20, clip_base=100)[0]
    assert _rows(got[:2]) == [(80, 101, 2, 0, 4, 0), (80, 102, 2, 0, 4, 0)]
    # an all-mismatch query, an empty query, an empty clip, an empty index: padding
    assert _rows(_search([np.zeros(10)], [np.full(5, ones)], 2, 31)[0]) == [ref.PAD, ref.PAD]
    assert _rows(_search([np.zeros(10)], [np.zeros(0)], 1, 31)[0]) == [ref.PAD]
    assert _rows(_search([np.zeros(0)], [np.zeros(3)], 1, 31)[0]) == [ref.PAD]
    assert _rows(ref.search_local(np.zeros(0, np.uint64), np.zeros(1, np.int64), np.zeros(4, np.uint64), np.array([0, 4]), 1, 1)[0]) == [ref.PAD]
    # a query longer than the clip, the clip inside it
    assert _rows(_search([r[2:5]], [r], 1, 5)[0]) == [(15, 0, -2, 2, 3, 0)]


def test_exact_excerpt():
    """a query that is an exact excerpt gives (T k, clip, offset, 0, k, 0)"""
    full = synth.random_hashprints(5, 400, 31)
    for T in (1, 22, 31):
        for c, o, k in ((0, 0, 64), (3, 96, 304), (4, 399, 1), (2, 17, 100)):
            got = _search(list(full), [full[c, o:o + k]], 2, T)[0]
            assert _rows(got[:1]) == [(T * k, c, o, 0, k, 0)], (T, c, o, k)
            assert int(got[1]["score"]) < T * k          # no other clip holds the excerpt


# The half-shared query of DESIGN.md section 25: an index of 8 synthetic clips of 10 s; a query of 5 s whose first part is an
# indexed clip from second 2 on and whose rest is a clip that is not in the index; gain 0.5 and white noise.
CUT_S, COLS_PER_S, T_HALF = 2.0, 80.6, 22


def _half_shared(oracle, filters, share, snr_db, n_queries):
    sr = synth.SR
    songs = np.stack([synth.gen_clip(i, 10.0) for i in range(8)])
    plan10, plan5 = oracle.Plan(10 * sr), oracle.Plan(5 * sr)
    db_hp, db_off = _lib._ragged(list(plan10.extract_batch(filters, songs, min(8, os.cpu_count() or 1))), np.uint64)
    queries = [plan5.extract(filters, ref.half_shared_query(songs[i], synth.gen_clip(100 + i, 10.0), 5.0, share, CUT_S, snr_db, i))
               for i in range(n_queries)]
    q_hp, q_off = _lib._ragged(queries, np.uint64)
    # hashprint j reads columns j .. j + (c - n_hp): the last clean one ends before the foreign part begins
    clean = int(share * plan5.c) - (plan5.c - plan5.n_hp)
    return db_hp, db_off, q_hp, q_off, clean


def test_half_shared_query(oracle, filters):
    for share, snr_db, n_queries in ((0.6, 10.0, 3), (0.5, 0.0, 2)):
        db_hp, db_off, q_hp, q_off, clean = _half_shared(oracle, filters, share, snr_db, n_queries)
        got = ref.search_local(db_hp, db_off, q_hp, q_off, 2, T_HALF)
        for i, row in enumerate(got):
            score, clip, lag, q_start, length, dist = _rows(row[:1])[0]
            runner_up = int(row[1]["score"])
            print(f"share {share}, {snr_db} dB, query {i}: score {score} (runner-up {runner_up}), clip {clip}, lag {lag}, "
                  f"run {q_start}..{q_start + length} (clean {clean}), dist {dist}")
            assert clip == i                                               # the true clip comes first,
            assert score >= 4 * max(runner_up, 1)                          # by a margin a scan that merely ranks does not have,
            assert abs(lag - round(CUT_S * COLS_PER_S)) <= 1               # on the diagonal of the cut
            if share == 0.6:
                assert 142 <= clean <= 144                                 # (143 hashprints free of the foreign part)
                assert abs(q_start + length - 143) <= 45                   # and the run ends where the shared passage does


FACADE = r"""
#include <hpfw/gpu/gpu_collector.h>
#include <hpfw/gpu/gpu_storage.h>
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    hpfw::db::GpuStorage<hpfw::GpuCollector> storage;
    hpfw::GpuCollector::Hashprint hp(304, 0);
    auto hits = storage.find_local(hp, 3, 22);
    if (hits.empty()) return 0;
    return (int)(hits[0].score + hits[0].lag + (int64_t)(hits[0].q_start + hits[0].length + hits[0].cnt + hits[0].filename.size()));
}
"""


def test_local_facade_compiles_and_links(tmp_path):
    src = tmp_path / "local.cpp"
    src.write_text(FACADE)
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(tmp_path / "local"), "-L", lib_dir, "-lhpfw_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "local")], capture_output=True, text=True)   # no argument: no device touched
    assert r.returncode == 2
