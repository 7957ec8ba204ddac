"""CPU tests of the voting search's device tally: the C surface, the refusals that come before any
device work, the derivation of the parallel form against the oracle's literal loop on the fixture of tests/votes_ref.py, the
shard merge in numpy, and the C++ facades.  The libraries load without a device; nothing here touches one."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

import hpfw_amd
from hpfw_amd import _lib, multi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import votes_ref as vr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
NEW = ("hpfw_gpu_knn_windows_device", "hpfw_gpu_vote_windows_device", "hpfw_gpu_search_votes_device", "hpfw_gpu_merge_knn_device")


def _declared(header, pattern):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(pattern, text))


def test_entry_points_are_declared_and_exported():
    single = _declared("hpfw_gpu.h", r"\b(hpfw_gpu_\w+)\s*\(")
    for sym in NEW:
        assert sym in single and sym in _lib.EXPORTS and hasattr(hpfw_amd.lib(), sym), sym
    assert _declared("hpfw_gpu_multi_votes.h", r"\b(hpfw_gpu_(?:group|shard)_\w+)\s*\(") == set(multi.VOTES_EXPORTS)
    assert multi.VOTES_EXPORTS == ("hpfw_gpu_group_search_votes",)
    assert not set(multi.VOTES_EXPORTS) & (set(multi.EXPORTS) | set(multi.RESAMPLE_EXPORTS) | set(multi.SEARCH_EXPORTS))
    assert all(hasattr(multi.lib(), s) for s in multi.VOTES_EXPORTS)
    for name in ("knn_windows_dev", "vote_windows_dev", "search_votes_dev", "merge_knn_dev"):
        assert callable(getattr(hpfw_amd.Gpu, name))
    assert callable(multi.GpuGroup.search_votes) and callable(hpfw_amd.LiveSongIdentification.top_votes)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _message():
    return hpfw_amd.lib().hpfw_gpu_last_error().decode()


def test_bad_arguments_are_refused_without_a_device():
    """the handle here is a buffer of zeros: a call that got as far as using it would not return a status"""
    L = hpfw_amd.lib()
    buf = np.zeros(64, np.int64)
    one = _p(buf)
    off = np.array([0, 70, 140], np.int64)                 # two queries of 70 hashprints: 7 windows each
    down = np.array([0, 70, 10], np.int64)
    wf = np.array([0, 7, 14], np.int64)

    def knn(h=one, q=one, q_off=off, n_q=2, keys=one, cap=70):
        return L.hpfw_gpu_knn_windows_device(h, q, None if q_off is None else _p(q_off), n_q, keys, cap, None)

    def tally(h=one, keys=one, w_first=wf, n_q=2, db_off=one, n_clips=3, out=one):
        return L.hpfw_gpu_vote_windows_device(h, keys, None if w_first is None else _p(w_first), n_q, db_off, n_clips, 0, out, None)

    def search(h=one, q=one, q_off=off, n_q=2, out=one):
        return L.hpfw_gpu_search_votes_device(h, q, None if q_off is None else _p(q_off), n_q, out, None)

    def merge(h=one, d_in=one, base=np.array([0, 5], np.int64), n_shards=2, n_win=4, out=one):
        return L.hpfw_gpu_merge_knn_device(h, d_in, None if base is None else _p(base), n_shards, n_win, out, None)

    # the host functions: round trips over the device calls, every refusal before the first of them
    def knn_host(h=one, q=one, q_off=off, n_q=2, keys=one, cap=70):
        return L.hpfw_gpu_knn_windows(h, q, None if q_off is None else _p(q_off), n_q, keys, cap)

    def search_host(h=one, q=one, q_off=off, n_q=2, out=one):
        return L.hpfw_gpu_search_votes(h, q, None if q_off is None else _p(q_off), n_q, out)

    bad = "bad argument"
    for call, want in ((lambda: knn_host(h=None), bad), (lambda: knn_host(q=None), bad), (lambda: knn_host(q_off=None), bad),
                     (lambda: knn_host(keys=None), bad), (lambda: knn_host(n_q=-1), bad),
                     (lambda: knn_host(q_off=down), "q_off must be non-decreasing"), (lambda: knn_host(cap=69), "keys buffer too small"),
                     (lambda: search_host(h=None), bad), (lambda: search_host(q=None), bad), (lambda: search_host(q_off=None), bad),
                     (lambda: search_host(out=None), bad), (lambda: search_host(n_q=-1), bad),
                     (lambda: search_host(q_off=down), "q_off must be non-decreasing"),
                     (lambda: knn(h=None), bad), (lambda: knn(q=None), bad), (lambda: knn(q_off=None), bad), (lambda: knn(keys=None), bad), (lambda: knn(n_q=-1), bad),
                     (lambda: knn(cap=-1), bad), (lambda: knn(q_off=down), "q_off must be non-decreasing"), (lambda: knn(cap=69), "keys buffer too small"),
                     (lambda: tally(h=None), bad), (lambda: tally(keys=None), bad), (lambda: tally(w_first=None), bad), (lambda: tally(db_off=None), bad),
                     (lambda: tally(out=None), bad), (lambda: tally(n_q=-1), bad), (lambda: tally(n_clips=-1), bad),
                     (lambda: tally(w_first=down), "w_first must be non-decreasing"),
                     (lambda: search(h=None), bad), (lambda: search(q=None), "null queries"), (lambda: search(q_off=None), bad), (lambda: search(out=None), bad),
                     (lambda: search(n_q=-2), bad), (lambda: search(q_off=down), "q_off must be non-decreasing"),
                     (lambda: merge(h=None), bad), (lambda: merge(d_in=None), bad), (lambda: merge(base=None), bad), (lambda: merge(out=None), bad),
                     (lambda: merge(n_shards=0), bad), (lambda: merge(n_shards=-1), bad), (lambda: merge(n_shards=65), bad), (lambda: merge(n_win=-1), bad)):
        rc = call()
        assert rc == E_INVALID and _message() == want, (rc, _message(), want)
    for base in ([-1, 5], [7, 5], [0, 1 << 40]):
        assert merge(base=np.array(base, np.int64)) == E_INVALID and _message().startswith("pos_base must be"), base
    M = multi.lib()
    q = np.zeros(140, np.uint64)
    out = np.zeros(2, _lib.VOTE_DTYPE)
    for rc in (M.hpfw_gpu_group_search_votes(None, _p(q), _p(off), 2, _p(out)), M.hpfw_gpu_group_search_votes(one, _p(q), None, 2, _p(out)),
               M.hpfw_gpu_group_search_votes(one, _p(q), _p(off), 2, None), M.hpfw_gpu_group_search_votes(one, _p(q), _p(off), -1, _p(out))):
        assert rc == E_INVALID and _message() == bad


def _same(a, b):
    return (int(a[0]), int(a[1])) == (int(b[0]), int(b[1])) and np.float32(a[2]).tobytes() == np.float32(b[2]).tobytes()


def _oracle_vote(oracle, keys, db_off):
    v = oracle.vote_windows(np.ascontiguousarray(keys).reshape(-1, 5), db_off)
    return (int(v["clip"]), int(v["offset"]), np.float32(v["cnt"]))


def test_parallel_form_equals_the_literal_loop(oracle):
    """grouping by bucket, one chain per bucket, the earliest event at the maximum: the oracle's literal loop on every query of
    the fixture, and the fixture holds the cases that tell the rule from its near misses"""
    keys, w_first, db_off = vr.fixture(33)
    assert w_first.size == 34 and keys.shape == (w_first[-1], 5) and np.any(np.diff(db_off) == 0)
    for q in range(33):
        k = keys[w_first[q]:w_first[q + 1]]
        want = _oracle_vote(oracle, k, db_off) if k.size else vr.NONE
        assert _same(vr.parallel_votes(k, db_off), want), q
        for row in k:                                       # ascending, padding behind the real keys
            real = row[row != vr.PAD]
            assert np.all(np.diff(real.astype(object)) > 0) and np.all(row[real.size:] == vr.PAD)
    q_tie, q_over, q_chain, q_one, q_none = (keys[w_first[i]:w_first[i + 1]] for i in range(5))
    # 1. two buckets with the same final value; the first to reach it has the larger clip id
    final = {}
    post = vr.post_values(q_tie, db_off)
    for idx in sorted(post):
        final[post[idx][0]] = post[idx][1]
    want = vr.query_tie()[1]
    assert sorted(final.values()) == [np.float32(2), np.float32(2)] and _same(vr.parallel_votes(q_tie, db_off), want)
    assert want[0] == max(b[0] for b in final)
    assert not _same(vr.wrong_final_argmax(q_tie, db_off), want) and not _same(vr.wrong_last_at_max(q_tie, db_off), want)
    # 2. a bucket leads for most of the query and is passed by another bucket's last event
    want = vr.query_overtaken()[1]
    assert _same(vr.parallel_votes(q_over, db_off), want)
    post = vr.post_values(q_over, db_off)
    leader = [_oracle_vote(oracle, q_over[:n], db_off)[:2] for n in range(1, 10)]      # the literal winner after n windows
    assert leader[:7] == [(2, 0)] * 7 and leader[7:] == [(4, -300)] * 2
    last_of_winner = max(i for i, (b, _) in post.items() if b == (4, -300))
    assert last_of_winner // 5 == 7 and post[last_of_winner][1] == np.float32(3.5)
    assert not _same(vr.wrong_final_argmax(q_over, db_off), want) and not _same(vr.wrong_last_at_max(q_over, db_off), want)
    # 3. votes with different d in an order where float accumulation is not the float64 sum rounded once
    chain = np.float32(0)
    for d in vr.CHAIN_D:
        chain = vr.vote_step(chain, d)
    once = np.float32(sum(np.float64(1.0) / np.float64(np.float32(d + 1)) for d in vr.CHAIN_D))
    assert chain != once
    assert _same(vr.parallel_votes(q_chain, db_off), (4, -40, chain))
    # 4. d = 0 votes
    assert any((int(k) >> 40) == 0 for k in q_tie.ravel() if k != vr.PAD)
    # 5. windows with 0, 1 and 4 real keys
    assert {int((row != vr.PAD).sum()) for row in q_chain} >= {0, 1, 4}
    # 6. a query of one window and a query of none
    assert q_one.shape[0] == 1 and q_none.shape[0] == 0 and _same(vr.parallel_votes(q_one, db_off), vr.query_one_window()[1])
    assert _same(vr.parallel_votes(q_none, db_off), vr.NONE)
    # 7. positions in the first and last hashprint of a clip, and in the clip after an empty clip
    pos = {int(k) & vr.POS_MASK for k in keys[:w_first[5]].ravel() if k != vr.PAD}
    assert {int(db_off[2]), int(db_off[3]), int(db_off[1]) - 1, int(db_off[3]) - 1, int(db_off[5]) - 1} <= pos
    assert db_off[1] == db_off[2] and any(e[1] == 0 and e[3] == 2 and e[4] == 0 for e in vr.events(q_over, db_off))   # position 100 is clip 2's


def test_shard_merge_equals_the_unsharded_order():
    """per-shard lists with positions inside the shard, merged with every shard's first position added: the unsharded list,
    with equal distances on both sides of the shard boundaries"""
    rng = np.random.default_rng(5)
    for n_shards in (1, 2, 3, 8):
        lists, base, whole = vr.shard_lists(rng, n_shards, 60)
        assert np.array_equal(vr.merge_knn(lists, base), whole)
        if n_shards > 1:
            ties = 0
            for w in range(60):
                real = whole[w][whole[w] != vr.PAD]
                for a, b in zip(real[:-1], real[1:]):
                    cut = [int(x) for x in base[1:]]
                    ties += (int(a) >> 40) == (int(b) >> 40) and (int(b) & vr.POS_MASK) in cut and (int(a) & vr.POS_MASK) + 1 in cut
            assert ties > 0
    lists, base, whole = vr.shard_lists(rng, 3, 20, spans=np.array([50, 0, 70]))          # a shard without an item
    assert np.all(lists[1] == vr.PAD) and np.array_equal(vr.merge_knn(lists, base), whole)


FACADE = r"""
#include <hpfw/gpu/gpu_collector.h>
#include <hpfw/gpu/gpu_storage.h>
#include <hpfw/gpu/sharded_storage.h>
int main(int argc, char **argv)
{
    if (argc < 2) // no argument: no device touched
        return hpfw_gpu_group_search_votes(nullptr, nullptr, nullptr, 1, nullptr) == HPFW_E_INVALID ? 2 : 1;
    using One = hpfw::db::GpuStorage<hpfw::GpuCollector>;
    using Sharded = hpfw::db::ShardedGpuStorage<hpfw::GpuCollector>;
    One one;
    Sharded sharded(std::vector<int>{0, 0});
    hpfw::GpuCollector::Hashprint hp(100, 0);
    const One::VoteResult a = one.find_votes(hp);
    const Sharded::VoteResult b = sharded.find_votes(hp);
    return a.filename == b.filename && a.cnt == b.cnt && a.offset == b.offset ? 0 : 1;
}
"""


def test_facades_with_find_votes_compile_and_link(tmp_path):
    src = tmp_path / "facade.cpp"
    src.write_text(FACADE)
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(tmp_path / "facade"), "-L", lib_dir, "-lhpfw_gpu_multi", "-lhpfw_gpu", "-Wl,-rpath," + lib_dir,
           "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "facade")], capture_output=True, text=True)   # no argument: no device touched
    assert r.returncode == 2
