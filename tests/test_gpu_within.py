"""The search within sets of clips on the GPU.  Every case is compared field for field with two things:
the restatement of tests/within_ref.py (the sub-index of the set handed to the CPU oracle) and the device's second opinion, a
second handle whose index holds only the set.  Every case runs under each scan selection (conftest's scan_path)."""
import math
import os
import subprocess

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, synth

import group_case
import overlap_score_ref
import timeline_ref
import within_ref as ref

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
_REF = {}                                                # references computed once, shared by the scan selections


@pytest.fixture(scope="module")
def wg(torch_cuda):
    """a handle of this file's own: the searches need no filters, and the session's handle keeps its index"""
    g = hpfw_amd.Gpu(0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def twin(torch_cuda):
    """the handle of the second opinion"""
    g = hpfw_amd.Gpu(0)
    yield g
    g.close()


def _rand(n, seed):
    return np.random.default_rng([0x77697468, seed]).integers(0, 2 ** 64, n, dtype=np.uint64)


def _index(g, db_hp, db_off, base=0):
    g.index_clear()
    g.index_set_clip_base(base)
    if db_off.size > 1:
        g.index_add(db_hp, db_off)


def _csr(sets):
    return (np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64),
            np.array([c for s in sets for c in s], np.int32))


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in ("dist", "clip", "offset"):
        if not np.array_equal(got[f], want[f]):
            bad = np.argwhere(got[f] != want[f])[0]
            raise AssertionError(f"{what}: {f} differs first at {tuple(bad)}: got {got[tuple(bad)]}, want {want[tuple(bad)]}")


def _twin_search(twin, db_hp, db_off, clips, q_hp, q_off, k, base=0, scored=False):
    """the second opinion: search_topk on a handle that holds only `clips`, the ids mapped back"""
    hp, off = ref.sub_index(db_hp, db_off, clips)
    _index(twin, hp if hp.size else np.zeros(1, np.uint64), off)
    out = twin.search_topk_scored(q_hp, q_off, k) if scored else (twin.search_topk(q_hp, q_off, k), None)
    return ref._map_back(out[0], clips, base), out[1]


def _moments(stats):
    return [(int(r["n"]), int(r["sum"]), int(r["sum_sq"])) for r in stats]


# ---- 1. a ragged index and the sets of the issue -------------------------------------------------------------------------------
N_CLIPS, LONGEST = 40, 20
SETS = [[], [5], list(range(0, 40, 2)), list(range(40)), [39], [7, 10, 11, 12, 13, 14], [3, 7, 20, 25]]
Q_LENGTHS = [200, 1, 304, 1000, 64, 5, 304, 700]


def _ragged_case():
    if "ragged" not in _REF:
        rng = np.random.default_rng(2403)
        lengths = [int(n) for n in rng.integers(150, 1200, N_CLIPS)]
        lengths[3], lengths[7], lengths[LONGEST] = 0, 5, 3000
        lengths[5], lengths[38], lengths[39] = 900, 700, 400
        for i, c in enumerate((10, 11, 12, 13, 14)):          # a set whose longest clip is far shorter than the index's
            lengths[c] = 30 + 17 * i
        clips = [_rand(n, 100 + i) for i, n in enumerate(lengths)]
        clips[39][:100] = clips[5][20:120]                    # (a stretch two clips share)
        queries = [_rand(k, 300 + i) for i, k in enumerate(Q_LENGTHS)]
        queries[0][:] = clips[LONGEST][2700:2900] ^ np.uint64(0x0000100000400001)   # in the last chunk of 1 024 offsets of the longest clip
        queries[2][:] = clips[5][10:314] ^ np.uint64(0x8000000000000000)
        queries[4][:] = clips[12][0:64]
        queries[6][:] = clips[38][50:354] ^ np.uint64(3)
        db_hp, db_off = _lib._ragged(clips, np.uint64)
        q_hp, q_off = _lib._ragged(queries, np.uint64)
        _REF["ragged"] = (db_hp, db_off, q_hp, q_off)
    return _REF["ragged"]


def _restated(oracle, key, db_hp, db_off, q_hp, q_off, set_off, set_clips, q_set, base=0):
    """the restatement for k = 64 (the lists for a smaller k are its first k records: the order is total)"""
    if key not in _REF:
        _REF[key] = ref.search_within(oracle, db_hp, db_off, q_hp, q_off, 64, set_off, set_clips, q_set, base)
    return _REF[key]


@pytest.mark.parametrize("k", [1, 3, 10, 64])
def test_the_sets_of_a_ragged_index(wg, twin, oracle, scan_path, k):
    db_hp, db_off, q_hp, q_off = _ragged_case()
    assert 2700 // 1024 == (3000 - 200) // 1024 == 2          # the planted match lies in the clip's last chunk
    _index(wg, db_hp, db_off)
    set_off, set_clips = _csr(SETS)
    n_q = q_off.size - 1
    plain = wg.search_topk(q_hp, q_off, k)
    for s, clips in enumerate(SETS):
        q_set = np.full(n_q, s, np.int32)
        got = wg.search_topk_within(q_hp, q_off, k, set_off, set_clips, q_set)
        want = _restated(oracle, ("ragged", s), db_hp, db_off, q_hp, q_off, set_off, set_clips, q_set)[:, :k]
        _same(got, want, f"set {s} against the restatement")
        assert (got["pad"] == 0).all()
        second, _ = _twin_search(twin, db_hp, db_off, clips, q_hp, q_off, k)
        assert got.tobytes() == second.tobytes(), s
        real = (got["clip"] != NONE).sum(axis=1)
        live = sum(1 for c in clips if db_off[c + 1] > db_off[c])
        assert (real == min(k, live)).all(), (s, real)         # padding records past the set's size
        assert np.isin(got["clip"][got["clip"] != NONE], clips).all()
    all_clips = wg.search_topk_within(q_hp, q_off, k, set_off, set_clips, np.full(n_q, 3, np.int32))
    assert all_clips.tobytes() == plain.tobytes()             # the set of all clips: the bytes of the unrestricted call
    assert wg.search_topk_within(q_hp, q_off, k, set_off, set_clips, np.full(n_q, -1, np.int32)).tobytes() == plain.tobytes()
    assert wg.search_topk_within(q_hp, q_off, k, [0], [], np.full(n_q, -1, np.int32)).tobytes() == plain.tobytes()   # no sets at all
    with_longest = wg.search_topk_within(q_hp, q_off, k, set_off, set_clips, np.full(n_q, 6, np.int32))
    found = {int(h["clip"]): (int(h["dist"]), int(h["offset"])) for h in with_longest[0]}    # (the 5-hashprint clip 7 is compared
    assert found.get(LONGEST, (3 * 200, 2700)) == (3 * 200, 2700) and (k < 3 or LONGEST in found)  # over 5 hashprints and comes first)
    assert k < 3 or (304, 5, 10) in [tuple(int(v) for v in h)[:3] for h in plain[2]]
    assert 5 not in wg.search_topk_within(q_hp, q_off, k, set_off, set_clips, np.full(n_q, 2, np.int32))["clip"]   # 5 is odd


# ---- 2. queries of several sets in one call ----------------------------------------------------------------------------------
MIX_SETS = [[17], [2, 5, 12, 20, 39], list(range(40))]


def _mixed_queries(n_q):
    key = ("mixq", n_q)
    if key not in _REF:
        db_hp, db_off = _ragged_case()[:2]
        lens = [(1, 40, 304, 130, 7, 1000, 64)[i % 7] for i in range(n_q)]
        queries = [_rand(k, 500 + i) for i, k in enumerate(lens)]
        for i in range(0, n_q, 3):                            # a third of the queries belong somewhere
            c = (5, 17, 20, 39, 2)[(i // 3) % 5]
            n = int(db_off[c + 1] - db_off[c])
            k = min(lens[i], n)
            queries[i][:k] = db_hp[db_off[c] + (n - k) // 2:db_off[c] + (n - k) // 2 + k] ^ np.uint64(1 << (i % 64))
        _REF[key] = _lib._ragged(queries, np.uint64)
    return _REF[key]


@pytest.mark.parametrize("n_q", [1, 7, 8, 33, 70])
def test_interleaved_sets(wg, twin, oracle, scan_path, n_q):
    """q_set cycles through three sets of 1, 5 and 40 clips and -1: no 32-row group of the caller's order is of one set"""
    db_hp, db_off = _ragged_case()[:2]
    q_hp, q_off = _mixed_queries(n_q)
    _index(wg, db_hp, db_off)
    set_off, set_clips = _csr(MIX_SETS)
    q_set = np.array([(1, -1, 0, 2)[i % 4] for i in range(n_q)], np.int32)
    k = 3
    got, stats = wg.search_topk_within(q_hp, q_off, k, set_off, set_clips, q_set, scored=True)
    want = _restated(oracle, ("mixed", n_q), db_hp, db_off, q_hp, q_off, set_off, set_clips, q_set)[:, :k]
    _same(got, want, "against the restatement")
    assert got.tobytes() == wg.search_topk_within(q_hp, q_off, k, set_off, set_clips, q_set).tobytes()
    plain, plain_stats = wg.search_topk_scored(q_hp, q_off, k)
    for s in sorted(set(q_set.tolist())):
        rows = np.flatnonzero(q_set == s)
        if s < 0:                                             # -1: the bytes of the existing call
            assert got[rows].tobytes() == plain[rows].tobytes() and stats[rows].tobytes() == plain_stats[rows].tobytes()
            continue
        sub_hp, sub_off = _lib._ragged([q_hp[q_off[i]:q_off[i + 1]] for i in rows], np.uint64)
        second, second_stats = _twin_search(twin, db_hp, db_off, MIX_SETS[s], sub_hp, sub_off, k, scored=True)
        assert got[rows].tobytes() == second.tobytes(), s
        assert stats[rows].tobytes() == second_stats.tobytes(), s


def test_twenty_sets_of_few_queries(wg, twin, oracle, scan_path):
    """70 queries over 20 sets: every set has fewer than 8 queries, the shifted-rows scan's side of the threshold"""
    db_hp, db_off = _ragged_case()[:2]
    q_hp, q_off = _mixed_queries(70)
    _index(wg, db_hp, db_off)
    rng = np.random.default_rng(2404)
    sets = [sorted(rng.choice(N_CLIPS, int(rng.integers(1, 12)), replace=False).tolist()) for _ in range(20)]
    set_off, set_clips = _csr(sets)
    q_set = np.array([(7 * i) % 20 for i in range(70)], np.int32)
    assert np.bincount(q_set, minlength=20).max() < 8
    got = wg.search_topk_within(q_hp, q_off, 10, set_off, set_clips, q_set)
    want = _restated(oracle, "twenty", db_hp, db_off, q_hp, q_off, set_off, set_clips, q_set)[:, :10]
    _same(got, want, "against the restatement")
    for s in (0, 13):
        rows = np.flatnonzero(q_set == s)
        sub_hp, sub_off = _lib._ragged([q_hp[q_off[i]:q_off[i + 1]] for i in rows], np.uint64)
        assert got[rows].tobytes() == _twin_search(twin, db_hp, db_off, sets[s], sub_hp, sub_off, 10)[0].tobytes()


# ---- 3. a query too long for the matrix-core scan, clip_base, device pointers, removal ------------------------------------------
def test_a_query_of_4000_hashprints(wg, twin, oracle):
    """without any switch: the window of a 4 000-hashprint query does not fit the LDS and the scan is the popcount kernel"""
    clips = [_rand(n, 700 + i) for i, n in enumerate((4500, 300, 5000, 4000, 0, 4100))]
    q = clips[2][600:4600] ^ np.uint64(0x10)
    db_hp, db_off = _lib._ragged(clips, np.uint64)
    _index(wg, db_hp, db_off)
    q_off = np.array([0, 4000], np.int64)
    for clips_of in ([1, 2, 5], [0, 3, 4], [2]):
        set_off, set_clips = _csr([clips_of])
        got, stats = wg.search_topk_within(q, q_off, 3, set_off, set_clips, [0], scored=True)
        want = ref.search_within(oracle, db_hp, db_off, q, q_off, 3, set_off, set_clips, [0])
        _same(got, want, clips_of)
        second, second_stats = _twin_search(twin, db_hp, db_off, clips_of, q, q_off, 3, scored=True)
        assert got.tobytes() == second.tobytes() and stats.tobytes() == second_stats.tobytes()
        assert _moments(stats) == ref.moments_within(oracle, db_hp, db_off, q, q_off, set_off, set_clips, [0])
    assert tuple(int(v) for v in wg.search_topk_within(q, q_off, 1, *_csr([[1, 2, 5]]), [0])[0, 0])[:3] == (4000, 2, 600)


def test_clip_base(wg, twin, oracle, scan_path):
    db_hp, db_off, q_hp, q_off = _ragged_case()
    _index(wg, db_hp, db_off, base=1000)
    try:
        set_off, set_clips = _csr(SETS)
        for s in (2, 6):
            q_set = np.full(q_off.size - 1, s, np.int32)
            got = wg.search_topk_within(q_hp, q_off, 10, set_off, set_clips, q_set)
            want = _restated(oracle, ("ragged", s), db_hp, db_off, q_hp, q_off, set_off, set_clips, q_set)[:, :10].copy()
            want["clip"][want["clip"] != NONE] += 1000
            _same(got, want, s)
            assert got.tobytes() == _twin_search(twin, db_hp, db_off, SETS[s], q_hp, q_off, 10, base=1000)[0].tobytes()
    finally:
        wg.index_set_clip_base(0)


def test_device_pointers_on_a_side_stream(wg, scan_path, torch_cuda):
    torch = torch_cuda
    db_hp, db_off = _ragged_case()[:2]
    q_hp, q_off = _mixed_queries(33)
    _index(wg, db_hp, db_off)
    set_off, set_clips = _csr(MIX_SETS)
    q_set = np.array([(1, -1, 0, 2)[i % 4] for i in range(33)], np.int32)
    want_hits, want_stats = wg.search_topk_within(q_hp, q_off, 4, set_off, set_clips, q_set, scored=True)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_q = torch.from_numpy(q_hp.view(np.int64)).cuda()
        d_out = torch.zeros(33 * 4 * 16, dtype=torch.uint8, device="cuda")
        d_stats = torch.full((33 * 24,), 0xAB, dtype=torch.uint8, device="cuda")     # (the call zeroes the rows itself)
        d_plain = torch.zeros(33 * 4 * 16, dtype=torch.uint8, device="cuda")
        wg.search_topk_within_dev(d_q.data_ptr(), q_off, 4, set_off, set_clips, q_set, d_out.data_ptr(), d_stats.data_ptr(),
                                  stream=side.cuda_stream)
        wg.search_topk_within_dev(d_q.data_ptr(), q_off, 4, set_off, set_clips, q_set, d_plain.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    assert d_out.cpu().numpy().tobytes() == want_hits.tobytes() == d_plain.cpu().numpy().tobytes()
    assert d_stats.cpu().numpy().tobytes() == want_stats.tobytes()


def test_after_index_remove(wg, twin, oracle, scan_path):
    """two clips that sets name are removed: their slots are empty clips of the sub-index"""
    db_hp, db_off, q_hp, q_off = _ragged_case()
    _index(wg, db_hp, db_off)
    wg.index_remove([5, 20])
    try:
        now_hp, now_off = wg.index_get()
        assert now_off[6] == now_off[5] and now_off[21] == now_off[20] and now_off.size == N_CLIPS + 1
        set_off, set_clips = _csr(SETS)
        for s in (1, 3, 6):
            q_set = np.full(q_off.size - 1, s, np.int32)
            got, stats = wg.search_topk_within(q_hp, q_off, 10, set_off, set_clips, q_set, scored=True)
            want = _restated(oracle, ("removed", s), now_hp, now_off, q_hp, q_off, set_off, set_clips, q_set)[:, :10]
            _same(got, want, s)
            second, second_stats = _twin_search(twin, now_hp, now_off, SETS[s], q_hp, q_off, 10, scored=True)
            assert got.tobytes() == second.tobytes() and stats.tobytes() == second_stats.tobytes()
            assert not np.isin(got["clip"], [5, 20]).any()
        assert (wg.search_topk_within(q_hp, q_off, 3, set_off, set_clips, np.full(q_off.size - 1, 1, np.int32))["clip"] == NONE).all()
    finally:
        wg.index_clear()


# ---- 4. scored and transposed --------------------------------------------------------------------------------------------------
def test_scored(wg, twin, oracle, scan_path):
    db_hp, db_off, q_hp, q_off = _ragged_case()
    _index(wg, db_hp, db_off)
    set_off, set_clips = _csr(SETS)
    lens = np.diff(db_off)
    for s, clips in enumerate(SETS):
        q_set = np.full(q_off.size - 1, s, np.int32)
        hits, stats = wg.search_topk_within(q_hp, q_off, 3, set_off, set_clips, q_set, scored=True)
        assert hits.tobytes() == wg.search_topk_within(q_hp, q_off, 3, set_off, set_clips, q_set).tobytes()
        if ("moments", s) not in _REF:
            _REF["moments", s] = ref.moments_within(oracle, db_hp, db_off, q_hp, q_off, set_off, set_clips, q_set)
        want = _REF["moments", s]
        assert _moments(stats) == want and (stats["pad"] == 0).all(), s
        assert [m[0] for m in want] == [sum(lens[c] >= kq for c in clips) for kq in Q_LENGTHS]
        _, second_stats = _twin_search(twin, db_hp, db_off, clips, q_hp, q_off, 3, scored=True)
        assert stats.tobytes() == second_stats.tobytes()
        for qi, h in enumerate(hits[:, 0]):
            if h["clip"] == NONE:
                continue
            counted = lens[int(h["clip"])] >= Q_LENGTHS[qi]
            sc, got = timeline_ref.hit_score(int(h["dist"]), counted, *want[qi]), _lib.hit_score(int(h["dist"]), counted, stats[qi])
            assert (math.isnan(sc) and math.isnan(got)) or abs(got - sc) <= 1e-12 * abs(sc), (s, qi, got, sc)
            if want[qi][0] < 3:
                assert math.isnan(got)                        # fewer than 3 counted clips: as an index of 2 clips


def test_query_groups(wg, oracle, scan_path):
    """HPFW_SEARCH_TABLE_KB=1: a table of 32 queries' rows (-1: 5 clips, 1 280 bytes; the set of 2 clips: 512 bytes, so 32 rows
    are the floor).  q_set mixes -1, a set of 2 clips and an empty set, so the 70 queries of group_case are regrouped into
    ranges of 33, 33 and 4: the range of -1 and the range of the set each run in passes of 32 and 1 -- the set's second pass
    meets the ClipView with offsets into the regrouped q_off, hits and moments -- where the call without the switch takes one
    pass each; scored"""
    clips, queries = group_case.case()
    db_hp, db_off = _lib._ragged(clips, np.uint64)
    q_hp, q_off = _lib._ragged(queries, np.uint64)
    _index(wg, db_hp, db_off)
    sets = [[1, 3], []]
    set_off, set_clips = _csr(sets)
    q_set = np.array([-1, 0] * (group_case.N_Q // 2), np.int32)
    q_set[[5, 25, 44, 64]] = 1                                # (two of the set's and two of -1's go to the empty set)
    assert [int((q_set == s).sum()) for s in (-1, 0, 1)] == [33, 33, 4]
    k = 3
    with group_case.env(HPFW_SEARCH_TABLE_KB=1):
        got, stats = wg.search_topk_within(q_hp, q_off, k, set_off, set_clips, q_set, scored=True)
    assert "HPFW_SEARCH_TABLE_KB" not in os.environ
    one_pass = wg.search_topk_within(q_hp, q_off, k, set_off, set_clips, q_set, scored=True)
    assert got.tobytes() == one_pass[0].tobytes() and stats.tobytes() == one_pass[1].tobytes()
    want = _restated(oracle, "query groups", db_hp, db_off, q_hp, q_off, set_off, set_clips, q_set)[:, :k]
    _same(got, want, "against the restatement")
    if "query groups, moments" not in _REF:
        _REF["query groups, moments"] = ref.moments_within(oracle, db_hp, db_off, q_hp, q_off, set_off, set_clips, q_set)
    assert _moments(stats) == _REF["query groups, moments"]
    for i in range(group_case.N_Q):                           # every clip of the query's set that holds hashprints, no other
        live = 0 if i == group_case.EMPTY else {-1: 4, 0: 2, 1: 0}[int(q_set[i])]
        assert (got[i]["clip"] != NONE).sum() == min(k, live), i
        assert q_set[i] != 0 or i == group_case.EMPTY or np.isin(got[i]["clip"][:2], [1, 3]).all(), i


def test_transposed(wg, twin, oracle, scan_path):
    """n_shifts = 3: variant i of query q is q_off entry 3 q + i, q_set has one entry per query"""
    db_hp, db_off = _ragged_case()[:2]
    _index(wg, db_hp, db_off)
    n_q, n_shifts, k = 9, 3, 5
    if "transposed" not in _REF:
        variants = [_rand((304, 64, 130)[q % 3], 800 + 3 * q + i) for q in range(n_q) for i in range(n_shifts)]
        for q in range(n_q):                                  # one variant of every query belongs somewhere; two tie on clip 5
            c, i = (5, 17, 20, 39, 2, 12, 5, 25, 38)[q], q % 3
            v = variants[3 * q + i]
            v[:min(v.size, 30)] = db_hp[db_off[c] + 3:db_off[c] + 3 + min(v.size, 30)]
        variants[3 * 6 + 1][:] = variants[3 * 6 + 0]           # (equal distances under two shifts: the smaller shift index wins)
        _REF["transposed"] = _lib._ragged(variants, np.uint64)
    q_hp, q_off = _REF["transposed"]
    set_off, set_clips = _csr(MIX_SETS)
    q_set = np.array([(1, -1, 0, 2)[q % 4] for q in range(n_q)], np.int32)
    got, stats = wg.search_topk_transposed_within(q_hp, q_off, n_shifts, k, set_off, set_clips, q_set, scored=True)
    assert got.tobytes() == wg.search_topk_transposed_within(q_hp, q_off, n_shifts, k, set_off, set_clips, q_set).tobytes()
    if "transposed_want" not in _REF:
        _REF["transposed_want"] = (ref.transposed_within(oracle, db_hp, db_off, q_hp, q_off, n_shifts, k, set_off, set_clips, q_set),
                                   ref.moments_within(oracle, db_hp, db_off, q_hp, q_off, set_off, set_clips, np.repeat(q_set, n_shifts)))
    want, want_moments = _REF["transposed_want"]
    assert [[tuple(int(v) for v in h) for h in row] for row in got] == want
    assert _moments(stats.ravel()) == want_moments and stats.shape == (n_q, n_shifts)
    plain, plain_stats = wg.search_topk_transposed_scored(q_hp, q_off, n_shifts, k)
    for s in sorted(set(q_set.tolist())):
        rows = np.flatnonzero(q_set == s)
        if s < 0:
            assert got[rows].tobytes() == plain[rows].tobytes() and stats[rows].tobytes() == plain_stats[rows].tobytes()
            continue
        sub_hp, sub_off = _lib._ragged([q_hp[q_off[3 * q + i]:q_off[3 * q + i + 1]] for q in rows for i in range(n_shifts)], np.uint64)
        hp, off = ref.sub_index(db_hp, db_off, MIX_SETS[s])
        _index(twin, hp, off)
        second, second_stats = twin.search_topk_transposed_scored(sub_hp, sub_off, n_shifts, k)
        mapped = second.copy()
        real = mapped["clip"] != NONE
        mapped["clip"][real] = np.array(MIX_SETS[s], np.uint32)[mapped["clip"][real]]
        assert got[rows].tobytes() == mapped.tobytes() and stats[rows].tobytes() == second_stats.tobytes(), s


# ---- 5. a large index: the two-step top-k and two slices of the moments ------------------------------------------------------------
N_BIG, BIG_SETS = 20000, (16500, 9000)


def _popcount(x):
    return np.unpackbits(np.ascontiguousarray(x).view(np.uint8).reshape(x.shape + (8,)), axis=-1).sum(axis=-1, dtype=np.int64)


def _big_case():
    """20 000 clips of 8 hashprints, 40 queries of 8 and 4 of 5; per query and set the distances by numpy"""
    if "big" not in _REF:
        rng = np.random.default_rng(2405)
        db = _rand(N_BIG * 8, 900).reshape(N_BIG, 8)
        sets = [np.sort(rng.choice(N_BIG, n, replace=False)).astype(np.int32) for n in BIG_SETS]
        queries = [_rand(8, 1000 + i) for i in range(40)] + [_rand(5, 1100 + i) for i in range(4)]
        for i in range(0, 40, 2):                             # half of the queries are a clip of their set or of the other one
            queries[i][:] = db[sets[(i // 2) % 2][(i * 397) % 9000]] ^ np.uint64(1 << i)
        for i in range(4):
            queries[40 + i][:] = db[sets[i % 2][100 + i], 2:7]
        q_set = np.array([i % 2 for i in range(44)], np.int32)
        want = []
        for q, s in zip(queries, q_set):
            sub = db[sets[s]]
            d = np.stack([_popcount(sub[:, o:o + q.size] ^ q).sum(axis=1) for o in range(8 - q.size + 1)])      # [offset][clip]
            off = d.argmin(axis=0)                            # the first minimum: the smallest offset
            dist = d.min(axis=0)
            order = np.lexsort((sets[s], dist))[:10]
            want.append(([(int(dist[c]), int(sets[s][c]), int(off[c])) for c in order],
                         (sub.shape[0], int(dist.sum()), int((dist * dist).sum()))))
        _REF["big"] = (db, sets, queries, q_set, want)
    return _REF["big"]


def test_large_index(wg, twin, scan_path):
    db, sets, queries, q_set, want = _big_case()
    assert min(BIG_SETS) < 16384 <= max(BIG_SETS) and max(BIG_SETS) // 4096 >= 2      # both top-k kernels, four and two slices
    _index(wg, db.ravel(), np.arange(N_BIG + 1, dtype=np.int64) * 8)
    try:
        q_hp, q_off = _lib._ragged(queries, np.uint64)
        set_off, set_clips = _csr(sets)
        hits, stats = wg.search_topk_within(q_hp, q_off, 10, set_off, set_clips, q_set, scored=True)
        assert [[tuple(int(v) for v in h)[:3] for h in row] for row in hits] == [w[0] for w in want]
        assert _moments(stats) == [w[1] for w in want]
        for s in (0, 1):
            rows = np.flatnonzero(q_set == s)
            sub_hp, sub_off = _lib._ragged([queries[i] for i in rows], np.uint64)
            _index(twin, db[sets[s]].ravel(), np.arange(sets[s].size + 1, dtype=np.int64) * 8)
            second, second_stats = twin.search_topk_scored(sub_hp, sub_off, 10)
            second["clip"] = sets[s].astype(np.uint32)[second["clip"]]
            assert hits[rows].tobytes() == second.tobytes() and stats[rows].tobytes() == second_stats.tobytes(), s
    finally:
        wg.index_clear()
        twin.index_clear()


def test_a_clip_outside_the_index_is_refused(wg):
    db_hp, db_off, q_hp, q_off = _ragged_case()
    _index(wg, db_hp, db_off)
    for clips in ([N_CLIPS], [0, 5, N_CLIPS + 3]):
        with pytest.raises(hpfw_amd.HpfwError) as e:
            wg.search_topk_within(q_hp, q_off, 1, *_csr([clips]), np.zeros(q_off.size - 1, np.int32))
        assert e.value.status == _lib.E_INVALID
    wg.search_topk_within(q_hp, q_off, 1, *_csr([[N_CLIPS - 1]]), np.zeros(q_off.size - 1, np.int32))


# ---- 6. end to end: concert (C) of tests/overlap_score_ref.py within a subset of its index -----------------------------------------
WITHIN = ["song00", "song02", "song03", "song04", "song05"]          # song 1, which the concert plays last, is outside the set


def _identifiers(filters, tmp_path):
    """(an identifier over songs 0-5 and the item, its twin build()-ed from the subset's hashprints, hashprints, names)"""
    songs, item, names = overlap_score_ref.concert_c_index()
    cache = str(tmp_path / "cache") + "/"                # the collectors read the filter fixture as they read learned filters
    os.makedirs(cache)
    with open(os.path.join(cache, "filters.cereal"), "wb") as f:
        f.write(np.array([64, 2420], np.int32).tobytes() + np.ascontiguousarray(filters, np.float32).tobytes())
    lsi, sub = hpfw_amd.LiveSongIdentification(cache=cache), hpfw_amd.LiveSongIdentification(cache=cache)
    ext = lsi.collector.gpu()
    hp = list(ext.extract(songs)) + [ext.extract(item[None])[0]]
    lsi.build(list(zip(hp, names)))
    sub.build([(h, n) for h, n in zip(hp, names) if n in WITHIN])
    return lsi, sub, hp, names


def _eq(a, b):
    """tuples equal with NaN equal to NaN"""
    return len(a) == len(b) and all(x == y or (isinstance(x, float) and isinstance(y, float) and math.isnan(x) and math.isnan(y))
                                    for x, y in zip(a, b))


def test_identifier_within(tmp_path, filters, torch_cuda, scan_path):
    """top(), timeline() and streams() with within= equal the same calls on the twin identifier that holds only the subset:
    names, times, offsets and scores are the same floats"""
    x = overlap_score_ref.concert_c()
    path = str(tmp_path / "concert_c.wav")
    synth.write_wav(path, x)
    cuts = []
    for i, (a, b) in enumerate(((30.0, 35.0), (3.0, 8.0), (20.0, 25.0))):      # from song 1 (outside the set), song 2, song 4
        cuts.append(str(tmp_path / f"cut{i}.wav"))
        synth.write_wav(cuts[-1], x[int(a * synth.SR):int(b * synth.SR)])
    lsi, sub, hp, names = _identifiers(filters, tmp_path)
    try:
        assert lsi.top(cuts, 1)[0][1][0][1] == "song01"
        for kw in (dict(), dict(tempos=[1.0, 1.04]), dict(shifts=[0, 2])):
            got, want = lsi.top(cuts, 4, within=WITHIN, **kw), sub.top(cuts, 4, **kw)
            assert got == want, kw
            assert all(name in WITHIN for _, rows in got for _, name, *_ in rows)       # song 1 is never named
            assert [rows[0][1] for _, rows in got[1:]] == ["song02", "song04"]
        assert lsi.top(cuts, 4, within=[]) == [(c, []) for c in cuts]
        for kw in (dict(), dict(tempos=[1.0, 1.04])):
            segs, wins = lsi.timeline(path, 5.0, windows=True, within=WITHIN, **kw)
            want_segs, want_wins = sub.timeline(path, 5.0, windows=True, **kw)
            assert len(wins) == len(want_wins) == 17
            for a, b in zip(wins, want_wins):                 # (the clip index differs: the twin's ids are the subset's)
                assert _eq(a[1:], b[1:]) and (a[0] is None) == (b[0] is None), (a, b)
                assert a[0] is None or names[a[0]] == a[1]
            assert len(segs) == len(want_segs) and all(_eq(a, b) for a, b in zip(segs, want_segs)), (segs, want_segs)
            assert {"song02", "song04"} <= {s[2] for s in segs} and "song01" not in {s[2] for s in segs}
            assert "song01" in {s[2] for s in lsi.timeline(path, 5.0, **kw)}
        assert all(math.isnan(w[4]) for w in lsi.timeline(path, 5.0, windows=True, within=["song02", "song04"])[1])   # 2 counted clips
        for bad in (["song09"], ["song02", "nope"]):
            with pytest.raises(KeyError):
                lsi.timeline(path, 5.0, within=bad)
        # two feeds pushed the same recording in uneven chunks, one restricted and one not: each equals its timeline()
        want = {0: lsi.timeline(path, 5.0, windows=True, within=WITHIN), 1: lsi.timeline(path, 5.0, windows=True)}
        segs, wins = {0: [], 1: []}, {0: [], 1: []}
        with lsi.streams(2, 5.0, windows=True, within=[WITHIN, None]) as live:
            at, sizes = [0, 0], [100003, 35797]
            while min(at) < x.size:
                chunks = {f: x[at[f]:at[f] + sizes[f]] for f in (0, 1) if at[f] < x.size}
                at = [min(at[f] + sizes[f], x.size) for f in (0, 1)]
                new, rows = live.push(chunks)
                for f, w, row in rows:
                    assert w == len(wins[f])
                    wins[f].append(row)
                for f, sg in new:
                    segs[f].append(sg)
            for f, sg in live.finish():
                segs[f].append(sg)
        for f in (0, 1):
            assert len(wins[f]) == 17 and all(_eq(a, b) for a, b in zip(wins[f], want[f][1])), f
            assert len(segs[f]) == len(want[f][0]) and all(_eq(a, b) for a, b in zip(segs[f], want[f][0])), (f, segs[f], want[f][0])
        assert want[0][0] != want[1][0]
        lsi.remove(["song03"])                                # a name that has been removed is a KeyError, as in remove()
        with pytest.raises(KeyError):
            lsi.top(cuts, 1, within=WITHIN)
    finally:
        lsi._gpu.close()
        sub._gpu.close()


FACADE = r"""
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <hpfw/gpu/gpu_collector.h>
#include <hpfw/gpu/gpu_storage.h>
#include <hpfw/gpu/live_streams.h>
using Storage = hpfw::db::GpuStorage<hpfw::GpuCollector>;
static void print(const char *tag, int feed, const hpfw::TimelineSegment &s)
{
    std::printf("%s %d %s %.17g %.17g %.17g %.17g\n", tag, feed, s.filename.c_str(), s.start_s, s.end_s, s.score, s.offset_s);
}
template <typename F>
static int refused(F f)
{
    try {
        f();
    } catch (const std::runtime_error &) {
        return 1;
    }
    return 0;
}
int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    Storage storage;
    storage.load(argv[1]);
    std::vector<float> filters((size_t)HPFW_FILTERS * HPFW_FRAME_SIZE);
    std::ifstream(argv[2], std::ios::binary).read(reinterpret_cast<char *>(filters.data()), (std::streamsize)(filters.size() * 4));
    if (hpfw_gpu_set_filters(storage.handle(), filters.data()) != 0) return 3;
    const std::vector<int32_t> set{0, 2, 3, 4, 5};
    hpfw::LiveStreamsOptions opt;
    opt.min_score = std::atof(argv[4]);
    opt.keep_windows = true;
    opt.within = {set};
    const hpfw::Timeline t = hpfw::timeline(storage, storage.handle(), argv[3], opt);
    for (size_t w = 0; w < t.windows.size(); ++w) std::printf("W 0 %zu %u %d %.17g\n", w, t.windows[w].clip, t.windows[w].offset, t.windows[w].score);
    for (const auto &s : t.segments) print("S", 0, s);
    int64_t n = 0;
    if (hpfw_gpu_wav_read_pcm16(argv[3], nullptr, 0, &n) != 0) return 4;
    std::vector<int16_t> pcm((size_t)n);
    if (hpfw_gpu_wav_read_pcm16(argv[3], pcm.data(), n, &n) != 0) return 4;
    // the hashprints of the window at 30 s (song 1, outside the set) through find_within and find_within_scored
    hpfw_geometry g;
    if (hpfw_gpu_geometry(storage.handle(), 220500, &g) != 0) return 5;
    hpfw::GpuCollector::Hashprint hp((size_t)g.n_hp);
    if (hpfw_gpu_extract_pcm16_host(storage.handle(), pcm.data() + 30 * 44100, 220500, 1, hp.data()) != 0) return 5;
    for (const auto &r : storage.find_within(hp, 3, set)) std::printf("F %s %zu %lld\n", r.filename.c_str(), r.cnt, (long long)r.offset);
    for (const auto &r : storage.find_within_scored(hp, 3, set)) std::printf("G %s %zu %lld %.17g\n", r.filename.c_str(), r.cnt, (long long)r.offset, r.score);
    for (const auto &r : storage.find_topk(hp, 1)) std::printf("T %s\n", r.filename.c_str());
    opt.within = {set, std::nullopt};
    hpfw::LiveStreams<Storage> live(storage, storage.handle(), 2, opt);
    const int64_t sizes[2] = {100003, 35797};
    int64_t at[2] = {0, 0};
    while (at[0] < n || at[1] < n) {
        std::vector<hpfw::LiveChunk> chunks;
        for (int f = 0; f < 2; ++f) {
            const int64_t m = std::min(sizes[f], n - at[f]);
            if (m > 0) chunks.push_back({f, pcm.data() + at[f], m});
            at[f] += m;
        }
        for (const auto &s : live.push(chunks)) print("L", s.feed, s.segment);
        for (const auto &w : live.windows()) std::printf("V %d %lld %u %d %.17g\n", w.feed, (long long)w.window, w.hit.clip, w.hit.offset, w.hit.score);
    }
    for (const auto &s : live.finish()) print("L", s.feed, s.segment);
    hpfw::TimelineOptions bad = opt;
    int r = 0;
    bad.within = {set};
    bad.min_overlap = 100;
    r += refused([&] { hpfw::timeline(storage, storage.handle(), argv[3], bad); });
    hpfw::LiveStreamsOptions bad_live = opt;
    bad_live.within = {set, set, set};
    r += refused([&] { hpfw::LiveStreams<Storage> x(storage, storage.handle(), 2, bad_live); });
    bad.min_overlap = 0;
    bad.within = {std::vector<int32_t>{2, 0}};
    r += refused([&] { hpfw::timeline(storage, storage.handle(), argv[3], bad); });
    std::printf("R %d\n", r);
    return 0;
}
"""


def test_cpp_facades_within(tmp_path, filters, torch_cuda):
    """GpuStorage::find_within, hpfw::timeline and hpfw::LiveStreams under TimelineOptions::within print the numbers of the
    Python calls; the program is what this test is about"""
    x = overlap_score_ref.concert_c()
    path = str(tmp_path / "concert_c.wav")
    synth.write_wav(path, x)
    cut = str(tmp_path / "cut.wav")
    synth.write_wav(cut, x[30 * synth.SR:30 * synth.SR + 220500])
    lsi, sub, hp, names = _identifiers(filters, tmp_path)
    try:
        want = {0: lsi.timeline(path, 5.0, windows=True, within=WITHIN), 1: lsi.timeline(path, 5.0, windows=True)}
        want_top = lsi.top([cut], 3, within=WITHIN)[0][1]
        assert lsi.top([cut], 1)[0][1][0][1] == "song01"
    finally:
        lsi._gpu.close()
        sub._gpu.close()
    with open(tmp_path / "dump.cereal", "wb") as f:       # GpuStorage::load: count, then per clip the name and the hashprints
        f.write(np.uint64(len(names)).tobytes())
        for name, h in zip(names, hp):
            f.write(np.uint64(len(name)).tobytes() + name.encode() + np.uint64(h.size).tobytes() + np.ascontiguousarray(h, np.uint64).tobytes())
    np.ascontiguousarray(filters, np.float32).tofile(tmp_path / "filters.f32")
    src = tmp_path / "facade.cpp"
    src.write_text(FACADE)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(src), "-o", str(tmp_path / "facade"),
           "-L", lib_dir, "-lhpfw_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "facade"), str(tmp_path / "dump.cereal"), str(tmp_path / "filters.f32"), path, "5.0"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = [ln.split() for ln in r.stdout.splitlines()]

    def same(a, b):
        return a == b or (math.isnan(a) and math.isnan(b))

    wins = [ln for ln in lines if ln[0] == "W"]
    assert len(wins) == 17
    for ln, row in zip(wins, want[0][1]):
        assert (None if int(ln[3]) == NONE else int(ln[3])) == row[0] and (row[0] is None or int(ln[4]) == row[3]) and same(float(ln[5]), row[4]), (ln, row)
    for tag, feed in (("S", 0), ("L", 0), ("L", 1)):
        got = [(float(ln[3]), float(ln[4]), ln[2], float(ln[5]), float(ln[6])) for ln in lines if ln[0] == tag and int(ln[1]) == feed]
        assert got == [s[:5] for s in want[feed][0]], (tag, feed, got, want[feed][0])
    for feed in (0, 1):
        live = [ln for ln in lines if ln[0] == "V" and int(ln[1]) == feed]
        assert len(live) == 17
        for w, (ln, row) in enumerate(zip(live, want[feed][1])):
            assert int(ln[2]) == w and (None if int(ln[3]) == NONE else int(ln[3])) == row[0] and same(float(ln[5]), row[4]), (feed, ln, row)
    found = [(int(ln[2]), ln[1], int(ln[3])) for ln in lines if ln[0] == "F"]
    assert found == want_top and all(name in WITHIN for _, name, _ in found)
    assert [(int(ln[2]), ln[1], int(ln[3])) for ln in lines if ln[0] == "G"] == want_top
    assert all(not math.isnan(float(ln[4])) for ln in lines if ln[0] == "G")
    assert ["T", "song01"] in lines and ["R", "3"] in lines
