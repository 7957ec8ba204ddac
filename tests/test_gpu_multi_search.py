"""The key, tempo and scored searches and the windows of one recording over a sharded index (DESIGN.md section 6.1,
include/hpfw_gpu_multi_search.h) on the one GPU this box has: the merge and sum kernels alone against the host merge and
Python integers, every group function against its one-handle namesake on every field and against the restatement over
oracle.match_clip, the sharded windows bit for bit, a concert end to end, and the group-level scored bound."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hpfw_amd  # noqa: E402
from hpfw_amd import _lib, multi, synth  # noqa: E402

import timeline_ref as ref  # noqa: E402

NONE = 0xFFFFFFFF
V = 3                                                              # variant sets per query


def _n_devices():
    """visible GPUs, counted without initialising the runtime (as tests/test_gpu_multi.py counts them)"""
    try:
        import torch
        return int(torch.cuda.device_count())
    except Exception:
        return 0


def _placements():
    """one GPU carries every shard; two devices are listed as skipped, not silently absent, where one GPU is visible"""
    n = _n_devices()
    marks = [] if n >= 2 else [pytest.mark.skip(reason=f"needs 2 GPUs, {n} visible")]
    return [[0], [0, 0], [0] * 8, pytest.param([0, 1], marks=marks, id="devices-0-1")]


# ---- the kernels alone (no RCCL) --------------------------------------------------------------------------------------------
DISTS = np.array([0, 0, 5, 5, 17, 17, 1000, 4096, 65535, 65536, 1023999, 1024000], np.uint32)   # ties, 0, the largest distance


def _shard_lists(n_shards, n_q, k, seed):
    """[n_shards][n_q][k] records of four 32-bit words: every list ascending by (dist, clip), clips distinct over the shards
    of a query (clip mod n_shards names the shard; ids up to 2^32 - 2^28), few distinct distances so that the clip decides
    across shards, dist = 0, lists of fewer than k hits and lists that are all padding (dist = clip = 0xffffffff), any third
    word on hits and padding alike, and a fourth word as a shift hit has it (-1 on some padding, not on all: padding comes out
    in input order and the test sees it)"""
    rng = np.random.default_rng(seed)
    shape = (n_shards, n_q, k)
    dist = np.sort(DISTS[rng.integers(0, DISTS.size, shape)], axis=-1)
    serial = np.cumsum(rng.integers(1, 1000, shape), axis=-1) + rng.integers(0, 1 << 20, (n_shards, n_q, 1))
    clip = serial * n_shards + np.arange(n_shards)[:, None, None]
    clip[:, ::5] += 0xF0000000                                     # a fifth of the queries: ids that need all 32 bits
    n_real = rng.integers(0, k + 1, (n_shards, n_q))
    n_real[rng.random((n_shards, n_q)) < 0.25] = k                 # full lists
    n_real[rng.random((n_shards, n_q)) < 0.2] = 0                  # all padding
    if n_shards > 2:
        n_real[1, ::2] = 0                                         # a shard with nothing for every other query
    pad = np.arange(k)[None, None, :] >= n_real[:, :, None]
    rec = np.zeros(shape + (4,), np.uint32)
    rec[..., 0] = np.where(pad, NONE, dist)
    rec[..., 1] = np.where(pad, NONE, clip).astype(np.uint32)
    rec[..., 2] = rng.integers(-2 ** 31, 2 ** 31, shape).astype(np.int32).view(np.uint32)
    fourth = rng.integers(0, 64, shape).astype(np.int32)
    fourth[pad & (rng.random(shape) < 0.5)] = -1
    rec[..., 3] = fourth.view(np.uint32)
    return rec


@pytest.mark.parametrize("n_q", [1, 45, 1000])
@pytest.mark.parametrize("n_shards,k", [(1, 1), (2, 10), (3, 10), (8, 1), (8, 64), (64, 64)])
def test_merge_kernel_equals_the_host_merge(gpu, torch_cuda, n_shards, k, n_q):
    """hpfw_gpu_merge_topk_device against hpfw_gpu_merge_topk on the same bytes, byte for byte: (3, 10) -> 30 candidates is
    the size that is no power of two, (64, 64) -> 4096 fills the LDS"""
    torch = torch_cuda
    rec = _shard_lists(n_shards, n_q, k, 1000 * n_shards + 10 * k + n_q)
    hits = rec.reshape(n_shards, n_q, k * 4).view(_lib.HIT_DTYPE).reshape(n_shards, n_q, k)
    key = (hits["dist"].astype(np.uint64) << np.uint64(32)) | hits["clip"].astype(np.uint64)   # what the generator promises
    assert (key[..., 1:] >= key[..., :-1]).all() and ((hits["dist"] == 0).any() or n_shards * n_q * k <= 40)
    real = hits["clip"] != NONE
    for q in range(min(n_q, 45)):
        c = hits["clip"][:, q][real[:, q]]
        assert np.unique(c).size == c.size
    want = _lib.merge_topk(hits, k)
    d_in = torch.from_numpy(rec.view(np.int32).copy()).cuda()
    d_out = torch.full((n_q, k, 4), 0x55555555, dtype=torch.int32, device="cuda")
    gpu.merge_topk_dev(d_in.data_ptr(), n_shards, n_q, k, d_out.data_ptr())
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert got.tobytes() == want.tobytes(), (n_shards, k, n_q, np.argwhere(got.reshape(n_q, k, 4) != want.view(np.int32).reshape(n_q, k, 4))[:4])
    assert np.array_equal(d_in.cpu().numpy(), rec.view(np.int32))  # the input is only read


@pytest.mark.parametrize("rows", [1, 5000])
@pytest.mark.parametrize("n_shards", [1, 3, 64])
def test_sum_kernel_equals_python_integers(gpu, torch_cuda, n_shards, rows):
    """hpfw_gpu_sum_stats_device: sum and sum_sq modulo 2^64 and n modulo 2^32 with moments near 2^63 (two of them already
    wrap), pad = 0 whatever the input's pad holds"""
    torch = torch_cuda
    rng = np.random.default_rng(7000 + 100 * n_shards + rows)
    st = np.zeros((n_shards, rows), _lib.STATS_DTYPE)
    st["sum"] = rng.integers(2 ** 62, 2 ** 63, (n_shards, rows), dtype=np.uint64) + rng.integers(0, 2 ** 62, (n_shards, rows), dtype=np.uint64)
    st["sum_sq"] = rng.integers(0, 2 ** 64, (n_shards, rows), dtype=np.uint64)
    st["sum_sq"][:, 0] = 2 ** 63 - 1                               # row 0: exactly n_shards (2^63 - 1)
    st["n"] = rng.integers(0, 2 ** 32, (n_shards, rows), dtype=np.uint32)
    st["pad"] = 0xDEADBEEF
    want = np.zeros(rows, _lib.STATS_DTYPE)
    want["sum"] = (st["sum"].astype(object).sum(axis=0) % 2 ** 64).astype(np.uint64)
    want["sum_sq"] = (st["sum_sq"].astype(object).sum(axis=0) % 2 ** 64).astype(np.uint64)
    want["n"] = (st["n"].astype(object).sum(axis=0) % 2 ** 32).astype(np.uint32)
    assert int(want["sum_sq"][0]) == n_shards * (2 ** 63 - 1) % 2 ** 64
    d_in = torch.from_numpy(st.view(np.int64).reshape(n_shards, rows, 3).copy()).cuda()
    d_out = torch.full((rows, 3), 0x5555555555555555, dtype=torch.int64, device="cuda")
    gpu.sum_stats_dev(d_in.data_ptr(), n_shards, rows, d_out.data_ptr())
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == want.tobytes()


# ---- the group against one handle and the oracle ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _workload():
    """the ragged 206-clip index and the 45 queries of test_gpu_multi.py's test_group_search_equals_unsharded_and_oracle, as
    V = 3 variant sets per query: set 0 is the query, sets 1 and 2 are seeded bit flips of it (about one and two bits per
    hashprint), so the variants compete for every clip"""
    rng = np.random.default_rng(31)
    lens = [int(x) for x in rng.integers(1, 900, 203)] + [2320, 0, 5]
    hp = [rng.integers(0, 2 ** 64, size=n, dtype=np.uint64) for n in lens]
    db, db_off = np.concatenate(hp), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    db[db_off[200]:db_off[200] + min(lens[200], lens[3])] = db[db_off[3]:db_off[3] + min(lens[200], lens[3])]
    qs = []
    for i in range(45):
        c = (i * 17) % len(lens)
        k = min(lens[c], int(rng.integers(1, 400)))
        if k and i % 4:
            o = int(rng.integers(0, lens[c] - k + 1))
            seg = db[db_off[c] + o: db_off[c] + o + k].copy()
            seg ^= np.uint64(1) << rng.integers(0, 64, size=k, dtype=np.uint64)
        else:
            seg = rng.integers(0, 2 ** 64, size=max(k, 1), dtype=np.uint64)
        qs.append(seg)
    flip = np.random.default_rng(32)
    sets = []
    for seg in qs:
        sets.append(seg)
        for v in range(1, V):
            x = seg.copy()
            for _ in range(v):
                x ^= np.uint64(1) << flip.integers(0, 64, size=x.size, dtype=np.uint64)
            sets.append(x)
    q_hp, q_off = _lib._ragged(sets, np.uint64)
    return db, db_off, sets, q_hp, q_off


_table_cache = {}


def _table(oracle):
    """per (set, clip) the clip's (distance, offset) by oracle.match_clip, None for an empty clip: computed once"""
    if "t" not in _table_cache:
        db, db_off, sets, _, _ = _workload()
        _table_cache["t"] = [ref.best_per_clip(oracle, s, db, db_off) for s in sets]
    return _table_cache["t"]


def _restated(oracle, n_clips, k):
    """the restatement over oracle.match_clip of both searches on the first n_clips clips: plain hits [sets][k] and stats
    [sets] as (dist, clip, offset) / (n, sum, sum_sq), transposed hits [queries][k] as (dist, clip, offset, set)"""
    _, db_off, sets, _, _ = _workload()
    lens = np.diff(db_off)[:n_clips]
    plain, stats, merged = [], [], []
    for s, per in zip(sets, _table(oracle)):
        per = per[:n_clips]
        live = sorted((p[0], c, p[1]) for c, p in enumerate(per) if p)
        plain.append(live[:k])
        stats.append(ref.row_moments([p[0] if p else 0 for p in per], [lens[c] >= s.size >= 1 for c in range(n_clips)]))
    for q in range(len(sets) // V):
        best = {}
        for v in range(V):
            for c, p in enumerate(_table(oracle)[q * V + v][:n_clips]):
                if p and (c not in best or (p[0], v) < (best[c][0], best[c][3])):
                    best[c] = (p[0], c, p[1], v)
        merged.append(sorted(best.values())[:k])
    return plain, stats, merged


def _rows(hits, fourth=None):
    return [[(int(h["dist"]), int(h["clip"]), int(h["offset"])) + ((int(h[fourth]),) if fourth else ()) for h in row if h["clip"] != NONE]
            for row in hits]


_one_cache = {}


def _one_handle(gpu, n_clips, k):
    """what the one handle gives on the first n_clips clips: computed once per (n_clips, k)"""
    if (n_clips, k) not in _one_cache:
        db, db_off, _, q_hp, q_off = _workload()
        gpu.index_clear()
        gpu.index_set_clip_base(0)
        gpu.index_add(db[:db_off[n_clips]], db_off[:n_clips + 1])
        try:
            _one_cache[(n_clips, k)] = (gpu.search_topk_scored(q_hp, q_off, k), gpu.search_topk_transposed(q_hp, q_off, V, k),
                                        gpu.search_topk_transposed_scored(q_hp, q_off, V, k))
        finally:
            gpu.index_clear()
    return _one_cache[(n_clips, k)]


def _compare(g, gpu, oracle, n_clips, ks):
    db, db_off, sets, q_hp, q_off = _workload()
    for k in ks:
        (one_hits, one_stats), one_t, (one_ts, one_tstats) = _one_handle(gpu, n_clips, k)
        hits, stats = g.search_topk_scored(q_hp, q_off, k)
        assert hits.tobytes() == one_hits.tobytes() and stats.tobytes() == one_stats.tobytes(), (n_clips, k)
        t = g.search_topk_transposed(q_hp, q_off, V, k)
        assert t.dtype == _lib.SHIFT_HIT_DTYPE and t.tobytes() == one_t.tobytes(), (n_clips, k)
        ts, tstats = g.search_topk_transposed_scored(q_hp, q_off, V, k)
        assert ts.tobytes() == one_ts.tobytes() == one_t.tobytes() and tstats.tobytes() == one_tstats.tobytes(), (n_clips, k)
        assert tstats.shape == (len(sets) // V, V) and tstats.tobytes() == stats.tobytes()       # a variant's row is its plain row
        assert g.search_topk(q_hp, q_off, k).tobytes() == hits.tobytes()                         # the unscored search, the same body
        plain, moments, merged = _restated(oracle, n_clips, k)
        assert _rows(hits) == plain and _rows(ts, "shift_index") == merged, (n_clips, k)
        assert [(int(s["n"]), int(s["sum"]), int(s["sum_sq"])) for s in stats] == moments
        assert (hits["pad"] == 0).all() and (ts["shift_index"][ts["clip"] == NONE] == -1).all()
        assert (stats["pad"] == 0).all()


@pytest.mark.parametrize("devices", _placements())
def test_group_searches_equal_one_handle_and_oracle(torch_cuda, gpu, oracle, devices):
    """every group search equals its one-handle namesake on every field, hits and moments, and the restatement over
    oracle.match_clip, at 1, 2 and 8 shards; then with 3 clips on the same shards, so that with 8 of them some are empty"""
    db, db_off, sets, q_hp, q_off = _workload()
    assert len(db_off) - 1 == 206 and len(sets) == 45 * V
    g = multi.GpuGroup(devices)
    try:
        g.index_build(db, db_off)
        assert np.array_equal(g.index_offsets(), db_off)
        _compare(g, gpu, oracle, 206, (1, 10))
        g.index_build(db[:db_off[3]], db_off[:4])
        assert np.array_equal(g.index_offsets(), db_off[:4])
        # 8 shards at k = 64: 512 candidates per query, almost all padding, whose order is what a merge can get wrong
        _compare(g, gpu, oracle, 3, (1, 10, 64) if len(devices) == 8 else (1, 10))
        # one query alone, and no query at all
        one = g.search_topk_transposed_scored(q_hp[q_off[V]:q_off[2 * V]], q_off[V:2 * V + 1] - q_off[V], V, 4)
        assert np.array_equal(one[0], _one_handle(gpu, 3, 10)[2][0][1:2, :4])
        none_hits, none_stats = g.search_topk_scored(np.zeros(1, np.uint64), np.zeros(1, np.int64), 3)
        assert none_hits.shape == (0, 3) and none_stats.shape == (0,)
    finally:
        g.close()


def test_group_lifecycle(torch_cuda):
    """what the group owns comes and goes with it: (a) eight shards created and closed with nothing in between, every owner
    destroyed empty; (b) three rounds of create, build, a plain and a transposed scored search, close, with equal results;
    (c) a placement naming an ordinal that does not exist is refused after part of the group was built, and the next group
    works"""
    db, db_off, _, q_hp, q_off = _workload()
    multi.GpuGroup([0] * 8).close()
    rounds = []
    for _ in range(3):
        g = multi.GpuGroup([0, 0])
        try:
            g.index_build(db[:db_off[3]], db_off[:4])
            ts, tstats = g.search_topk_transposed_scored(q_hp, q_off, V, 10)
            rounds.append((g.search_topk(q_hp, q_off, 10).tobytes(), ts.tobytes(), tstats.tobytes()))
        finally:
            g.close()
    assert rounds[0] == rounds[1] == rounds[2] and (np.frombuffer(rounds[0][0], _lib.HIT_DTYPE)["clip"] != NONE).any()
    with pytest.raises(hpfw_amd.HpfwError, match="no device") as e:
        multi.GpuGroup([0, _n_devices()])
    assert e.value.status == _lib.E_INVALID
    g = multi.GpuGroup([0, 0])
    try:
        g.index_build(db[:db_off[3]], db_off[:4])
        assert g.search_topk(q_hp, q_off, 10).tobytes() == rounds[0][0]
    finally:
        g.close()


def test_group_checks_match_the_one_handle(torch_cuda, gpu):
    """with a group in hand, the refusals carry the one-handle call's status and message"""
    db, db_off, sets, q_hp, q_off = _workload()
    g = multi.GpuGroup([0, 0])
    try:
        g.index_build(db[:db_off[3]], db_off[:4])
        gpu.index_clear()
        gpu.index_add(db[:db_off[3]], db_off[:4])
        for call in (lambda x: x.search_topk_scored(q_hp, q_off, 65), lambda x: x.search_topk_transposed(q_hp, q_off, V, 0),
                     lambda x: x.search_topk_transposed_scored(q_hp, q_off[:66 * 2 + 1], 66, 3),
                     lambda x: x.search_topk_scored(np.zeros(16001, np.uint64), [0, 16001], 1)):
            msgs = []
            for x in (g, gpu):
                with pytest.raises(hpfw_amd.HpfwError) as e:
                    call(x)
                msgs.append((e.value.status, str(e.value)))
            assert msgs[0] == msgs[1], msgs
    finally:
        gpu.index_clear()
        g.close()


def test_group_scored_bound_is_the_groups(torch_cuda):
    """n_clips * k_max^2 * 4096 >= 2^64 is reachable within the 16 000-hashprint limit once clips may be empty: 17 592 187
    clips and a query of 16 000 hashprints.  On two shards each block (8 796 094 and 8 796 093 clips) passes the bound alone
    (tests/test_multi_search_host.py checks the arithmetic), so only the group's own check can refuse the call: it does, with
    the one-handle call's status and message, before any shard is searched.  The plain search has no such bound."""
    n_clips = 17_592_187
    g = multi.GpuGroup([0, 0])
    try:
        g.index_build(np.zeros(1, np.uint64), np.zeros(n_clips + 1, np.int64))
        sizes = [hpfw_amd.Gpu.from_handle(g.handle(s)).index_size() for s in range(2)]
        assert sizes == [8_796_094, 8_796_093] and all(n * 16000 * 16000 * 4096 < 2 ** 64 for n in sizes)
        q = np.zeros(16000, np.uint64)
        for call in (lambda: g.search_topk_scored(q, [0, 16000], 1), lambda: g.search_topk_transposed_scored(q, [0, 0, 16000], 2, 1)):
            with pytest.raises(hpfw_amd.HpfwError) as e:
                call()
            assert e.value.status == _lib.E_UNSUPPORTED
            assert "scored search: n_clips * k_max^2 * 4096 must stay below 2^64" in str(e.value) and "shard" not in str(e.value)
    finally:
        g.close()


# ---- windows ----------------------------------------------------------------------------------------------------------------
WIN = 220500
SHIFTS, TEMPOS = [-2, 0, 2], [0.96, 1.0, 1.04]


def test_group_windows_are_the_one_handles(gpu, filters):
    """a 20 s recording at an even and an odd hop, plain, shifted, at other tempos and both, on 1, 2 and 8 shards (7 windows at
    the even hop: more shards than windows): bit for bit what Gpu.extract_windows gives"""
    x = np.concatenate([synth.gen_clip(520, 10.0), synth.gen_clip(521, 10.0)])
    assert x.size == 20 * synth.SR
    groups = [multi.GpuGroup([0] * n) for n in (1, 2, 8)]
    try:
        for g in groups:
            g.set_filters(filters)
        for hop, n_w in ((110250, 7), (44101, 15)):
            for tempos, shifts in ((None, None), (None, SHIFTS), (TEMPOS, None), (TEMPOS, SHIFTS)):
                want = gpu.extract_windows(x, WIN, hop, tempos, shifts)
                assert want.shape[0] == n_w and want.any()
                for g in groups:
                    got = g.extract_windows(x, WIN, hop, tempos, shifts)
                    assert got.shape == want.shape and np.array_equal(got, want), (g.shards, hop, tempos, shifts)
        g = groups[1]
        assert g.extract_windows(x[:WIN - 1], WIN, 110250).shape == (0, gpu.geometry(WIN).n_hp)     # shorter than a window
        assert np.array_equal(g.extract_windows(x[:WIN], WIN, 110250), gpu.extract_windows(x[:WIN], WIN, 110250))   # one window
        # the one-handle call's checks, made once up front
        for bad in (dict(shifts=[1, 1]), dict(tempos=[3.0]), dict(hop=WIN + 1), dict(win=4410)):
            kw = dict(win=WIN, hop=110250)
            kw.update(bad)
            msgs = []
            for who in (g, gpu):
                with pytest.raises(hpfw_amd.HpfwError) as e:
                    who.extract_windows(x, **kw)
                msgs.append((e.value.status, str(e.value)))
            assert msgs[0] == msgs[1], msgs
        hpfw_amd.Gpu.from_handle(g.handle(0)).set_projection(0)
        with pytest.raises(hpfw_amd.HpfwError, match="projection mode 1"):
            g.extract_windows(x, WIN, 110250, shifts=SHIFTS)
    finally:
        for g in groups:
            g.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------
N_SONGS = 20


def _same(a, b):
    """equality of nested tuples / lists in which NaN equals NaN"""
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a):
        return math.isnan(b)
    return a == b


def test_timeline_of_a_concert_on_a_sharded_index(tmp_path, filters, torch_cuda):
    """concert (A) of tests/test_gpu_timeline.py through LiveSongIdentification(devices=[0, 0, 0]): the same segments and the
    same per-window tuples as devices=None, plain and with variants"""
    x = ref.concert_a()
    path = str(tmp_path / "concert_a.wav")
    synth.write_wav(path, x)
    songs = np.stack([synth.gen_clip(i, 30.0) for i in range(N_SONGS)])
    got = []
    for devices in (None, [0, 0, 0]):
        lsi = hpfw_amd.LiveSongIdentification(devices=devices)
        try:
            ext = lsi.collector.gpu()
            ext.set_filters(filters)
            hp = ext.extract(songs)
            lsi.build([(hp[i], f"song{i:02d}") for i in range(N_SONGS)])
            segs, wins = lsi.timeline(path, min_score=10, windows=True)
            segs_v, wins_v = lsi.timeline(path, min_score=10, shifts=[-2, 0, 2], tempos=[1.0, 1.04], windows=True)
            got.append((segs, wins, segs_v, wins_v))
        finally:
            lsi._gpu.close()
    assert len(got[0][1]) == 41 and [s[2] for s in got[0][0]] == ["song03", "song11", "song07"]
    assert _same(got[0], got[1])
