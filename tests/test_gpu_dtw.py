"""The warped search on the GPU against the restatement of tests/dtw_ref.py: equality of integers,
field for field, at the widths where the kernel changes lane, block or path."""
import ctypes
import os

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, synth

import dtw_ref as ref

pytestmark = pytest.mark.gpu


STRIP, BLOCK = _lib.DTW_STRIP, _lib.DTW_BLOCK             # columns per lane, columns per pass of the wave
# every width within 2 of: one lane's strip, two strips, the last lane's strip, one block, two blocks (so 2 BLOCK + 1 and
# 2 BLOCK + 2 span three blocks)
EDGES = sorted({e + d for e in (STRIP, 2 * STRIP, BLOCK - STRIP, BLOCK, 2 * BLOCK) for d in range(-2, 3)})
_REF = {}


@pytest.fixture(scope="module")
def dt(torch_cuda):
    """a handle of this file's own: the searches need no filters, and the session's handle keeps its index"""
    g = hpfw_amd.Gpu(0)
    yield g
    g.close()


def _rand(n, seed):
    return np.random.default_rng([0x64747721, seed]).integers(0, 2 ** 64, n, dtype=np.uint64)


def _few(n, seed):
    """hashprints of four values a few bits apart: ties everywhere"""
    return np.array([0, 1, 3, 0xFF], np.uint64)[np.random.default_rng([0x74696573, seed]).integers(0, 4, n)]


def _flip(hp, fraction, seed):
    rng = np.random.default_rng([0x666C6970, seed])
    mask = np.zeros(hp.size, np.uint64)
    for b in range(64):
        mask |= (rng.random(hp.size) < fraction).astype(np.uint64) << np.uint64(b)
    return hp ^ mask


def _warp(r, start, k, seed, odd=None):
    """k hashprints read off r from column `start` along a random admissible path (as many as fit); odd: the share of
    steps other than 1 (None: every admissible step is as likely as another)"""
    rng = np.random.default_rng([0x77617270, seed])
    path, prev = [start], -1
    while len(path) < k:
        steps = (1, 2, 0) if prev == 1 and len(path) >= 2 else (1, 2)
        prev = int(rng.choice(steps)) if odd is None or rng.random() < odd else 1
        if path[-1] + prev >= r.size:
            break
        path.append(path[-1] + prev)
    return r[np.array(path)].copy()


def _index(g, clips, base=0):
    db_hp, db_off = _lib._ragged(clips, np.uint64)
    g.index_clear()
    g.index_set_clip_base(base)
    g.index_add(db_hp, db_off)
    return db_hp, db_off


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)[0]
        raise AssertionError(f"{what}: first difference at {tuple(bad)}: got {got[tuple(bad)]}, want {want[tuple(bad)]}")


def test_widths_are_the_kernels(dt):
    strip, block = ctypes.c_int32(0), ctypes.c_int32(0)
    _lib.check(hpfw_amd.lib().hpfw_gpu_dtw_geometry(ctypes.byref(strip), ctypes.byref(block)))
    assert (strip.value, block.value) == (STRIP, BLOCK)


def _widths(k):
    return sorted({1, 2, max(k // 2, 1), k // 2 + 1, k} | set(EDGES))


@pytest.mark.parametrize("content", ["random", "ties"])
@pytest.mark.parametrize("k", [1, 2, 3, 64, 305])
def test_pairs_at_every_width(dt, k, content):
    widths = _widths(k)
    assert 2 * BLOCK + 2 in widths and BLOCK + 1 in widths and STRIP - 1 in widths
    make = _rand if content == "random" else _few
    clips = [make(n, 10 + i) for i, n in enumerate(widths)]
    db = _index(dt, clips)
    big = clips[-1]                                       # 2 BLOCK + 2 columns: three blocks
    q = _warp(big, BLOCK - k // 2 if k > 3 else BLOCK - 1, k, k) if content == "random" else make(k, 99)
    if content == "random" and k > 3:
        q = _flip(q, 0.05, k)
    assert q.size == k
    pairs = [(0, ci) for ci in range(len(clips))]
    want = ref.dtw_pairs(db[0], db[1], q, np.array([0, k]), pairs)
    got = dt.dtw_pairs(q, np.array([0, k]), pairs)
    _same(got, want, (k, content))
    has = np.array([n >= k // 2 + 1 for n in widths])
    assert ((got["clip"] != _lib.NO_CLIP) == has).all()
    if content == "random" and k > 3:                     # the planted path crosses the first block boundary
        assert got[-1]["start"] < BLOCK <= got[-1]["end"] and got[-1]["dist"] < 8 * k


def test_pairs_all_equal_hashprints(dt):
    """every cell ties: the tie order and the propagation of S decide every field"""
    lengths = [1, 2, 3, 5, STRIP, STRIP + 1, 100, BLOCK, BLOCK + 1, BLOCK + 90]
    clips = [np.full(n, 0x0123456789ABCDEF, np.uint64) for n in lengths]
    db = _index(dt, clips)
    ks = [1, 2, 5, 64, 200]
    q_hp, q_off = _lib._ragged([np.full(k, 0x0123456789ABCDEF, np.uint64) for k in ks], np.uint64)
    pairs = [(qi, ci) for qi in range(len(ks)) for ci in range(len(lengths))]
    got = dt.dtw_pairs(q_hp, q_off, pairs)
    _same(got, ref.dtw_pairs(db[0], db[1], q_hp, q_off, pairs), "all equal")
    for (qi, ci), h in zip(pairs, got):
        if lengths[ci] >= ks[qi] // 2 + 1:                # the slowest path from column 0 ends first
            assert (int(h["dist"]), int(h["start"]), int(h["end"])) == (0, 0, ks[qi] // 2)


def test_pairs_matches_at_the_clip_ends(dt):
    n = BLOCK + 88
    r = _rand(n, 500)
    db = _index(dt, [r])
    queries = [r[0:100], r[1:101], r[n - 100:], r[BLOCK - 40:BLOCK + 40], r[n - 200::2], _warp(r, 1, 150, 7), _flip(_warp(r, 0, 90, 8), 0.03, 9)]
    q_hp, q_off = _lib._ragged(queries, np.uint64)
    pairs = [(qi, 0) for qi in range(len(queries))]
    got = dt.dtw_pairs(q_hp, q_off, pairs)
    _same(got, ref.dtw_pairs(db[0], db[1], q_hp, q_off, pairs), "ends")
    assert [(int(h["dist"]), int(h["start"]), int(h["end"])) for h in got[:5]] == \
        [(0, 0, 99), (0, 1, 100), (0, n - 100, n - 1), (0, BLOCK - 40, BLOCK + 39), (0, n - 200, n - 2)]
    assert (int(got[5]["dist"]), int(got[5]["start"])) == (0, 1) and int(got[6]["start"]) == 0


def test_pairs_long_query(dt):
    """K = 2000 against n = 2500: 32 chunks of rows, five blocks"""
    r = _rand(2500, 600)
    q = _flip(_warp(r, 3, 2000, 11, odd=0.3), 0.02, 12)
    assert q.size == 2000
    db = _index(dt, [r])
    got = dt.dtw_pairs(q, np.array([0, 2000]), [(0, 0)])
    _same(got, ref.dtw_pairs(db[0], db[1], q, np.array([0, 2000]), [(0, 0)]), "long")
    assert int(got[0]["start"]) == 3 and int(got[0]["dist"]) < 2000 * 64 * 0.04


RAGGED = [0, 1, 5, 31, 32, 33, 36, 63, 64, 71, 72, 73, 100, 143, 152, 153, 154, 200, 250, 304, 305, 306, 320, 400, 64, 143, 305, 72,
          BLOCK - 1, BLOCK, BLOCK + 1, 600, 2 * BLOCK + 3, 10, 20, 153, 80, 90, 8, 16]
Q_LENGTHS = [64, 143, 305]


def _ragged_case():
    clips = [_rand(n, 700 + i) for i, n in enumerate(RAGGED)]
    queries = [_flip(_warp(clips[31], 100, 64, 1), 0.1, 2), _flip(_warp(clips[32], 500, 143, 3), 0.1, 4), _flip(_warp(clips[31], 2, 305, 5), 0.1, 6)]
    clips[36][:] = clips[31][90:170]                      # part of another clip: a second good candidate for query 0
    return clips, queries


def test_search_every_clip(dt):
    """candidates = 0 on a ragged index: clips below the reachability bound, an empty clip, k below and above the number
    of candidates, a clip base"""
    clips, queries = _ragged_case()
    assert len(clips) == 40
    q_hp, q_off = _lib._ragged(queries, np.uint64)
    cache = _REF.setdefault("ragged", {})
    for base in (0, 1000):
        db = _index(dt, clips, base)
        full = ref.search_dtw(db[0], db[1], q_hp, q_off, 64, clip_base=base, cache=cache)
        n_cand = [sum(n >= k // 2 + 1 for n in RAGGED) for k in Q_LENGTHS]
        assert [int(v) for v in (full["clip"] != _lib.NO_CLIP).sum(1)] == n_cand and max(n_cand) < 40 and min(n_cand) > 5
        for k in (1, 5, 64):
            got = dt.search_dtw(q_hp, q_off, k, 0)
            _same(got, full[:, :k], ("every clip", base, k))
        assert [int(c) - base for c in full["clip"][:, 0]] == [31, 32, 31]
        assert tuple(int(v) for v in full[0, -1]) == ref.PAD   # fewer than 64 candidates: padding behind them
    dt.index_set_clip_base(0)


@pytest.mark.parametrize("base", [0, 77])
def test_search_reranks_the_plain_candidates(dt, oracle, base):
    clips, queries = _ragged_case()
    q_hp, q_off = _lib._ragged(queries, np.uint64)
    db = _index(dt, clips, base)
    cache = _REF.setdefault("ragged", {})
    for k, cand in ((1, 1), (3, 3), (3, 64), (5, 8), (64, 64)):
        plain = oracle.search_topk(db[0], db[1], q_hp, q_off, cand)
        cand_clips = [[int(c) for c in row["clip"] if c != _lib.NO_CLIP] for row in plain]
        want = ref.search_dtw(db[0], db[1], q_hp, q_off, k, cand_clips=cand_clips, clip_base=base, cache=cache)
        got = dt.search_dtw(q_hp, q_off, k, cand)
        _same(got, want, ("re-rank", k, cand, base))
    # 64 candidates of 39 non-empty clips: the plain search names clips too short for the warped rule; they give no hit
    assert (got["clip"] != _lib.NO_CLIP).sum(1).max() < 39
    dt.index_set_clip_base(0)


def test_search_empty_index_and_empty_query(dt):
    dt.index_clear()
    q = _rand(64, 1)
    for cand in (0, 2):
        got = dt.search_dtw(q, np.array([0, 64]), 2, cand)
        assert [tuple(int(v) for v in h) for h in got[0]] == [ref.PAD] * 2
    _index(dt, [_rand(100, 2), _rand(50, 3)])
    got = dt.search_dtw(q, np.array([0, 0, 64]), 2, 0)   # the first query is empty
    assert [tuple(int(v) for v in h) for h in got[0]] == [ref.PAD] * 2 and (got[1]["clip"] != _lib.NO_CLIP).all()
    got = dt.dtw_pairs(q, np.array([0, 0, 64]), [(0, 0), (1, 1)])
    assert tuple(int(v) for v in got[0]) == ref.PAD and int(got[1]["clip"]) == 1


def test_host_and_device_forms_return_the_same_bytes(dt, torch_cuda):
    torch = torch_cuda
    clips, queries = _ragged_case()
    q_hp, q_off = _lib._ragged(queries, np.uint64)
    _index(dt, clips, 5)
    d_q = torch.from_numpy(q_hp.view(np.int64)).cuda()
    pairs = [(0, 31), (1, 32), (2, 31), (2, 0), (1, 5), (0, 36)]

    def dev(n_hits, call):
        d_out = torch.zeros(n_hits * 16, dtype=torch.uint8, device="cuda")
        call(d_out.data_ptr())
        torch.cuda.synchronize()
        return d_out.cpu().numpy().tobytes()

    assert dev(len(pairs), lambda p: dt.dtw_pairs_dev(d_q.data_ptr(), q_off, pairs, p)) == dt.dtw_pairs(q_hp, q_off, pairs).tobytes()
    for k, cand in ((3, 0), (3, 8)):
        assert dev(3 * k, lambda p: dt.search_dtw_dev(d_q.data_ptr(), q_off, k, cand, p)) == dt.search_dtw(q_hp, q_off, k, cand).tobytes()
    hit, path = dt.dtw_path(queries[1], 32)
    d_path = torch.zeros(143, dtype=torch.int32, device="cuda")
    d_hit = torch.zeros(16, dtype=torch.uint8, device="cuda")
    dt.dtw_path_dev(d_q.data_ptr() + 8 * int(q_off[1]), 143, 32, d_path.data_ptr(), d_hit.data_ptr())
    torch.cuda.synchronize()
    assert d_path.cpu().numpy().tobytes() == path.tobytes() and d_hit.cpu().numpy().tobytes() == hit.tobytes()
    dt.index_set_clip_base(0)


def test_refusals_that_need_an_index(dt):
    _index(dt, [_rand(100, 1), np.zeros(134218, np.uint64)])
    q = _rand(64, 2)
    for bad in ([(1, 0)], [(0, 2)]):                      # one query, two clips
        with pytest.raises(hpfw_amd.HpfwError) as e:
            dt.dtw_pairs(q, np.array([0, 64]), bad)
        assert e.value.status == _lib.E_INVALID
    with pytest.raises(hpfw_amd.HpfwError) as e:
        dt.dtw_path(q, 2)
    assert e.value.status == _lib.E_INVALID
    long = np.zeros(16001, np.uint64)
    for call in (lambda: dt.search_dtw(long, np.array([0, 16001]), 1, 0), lambda: dt.search_dtw(long, np.array([0, 16001]), 1, 1),
                 lambda: dt.dtw_pairs(long, np.array([0, 16001]), [(0, 0)]), lambda: dt.dtw_path(long, 0)):
        with pytest.raises(hpfw_amd.HpfwError) as e:
            call()
        assert e.value.status == _lib.E_UNSUPPORTED and "16000" in str(e.value)
    # the cell cap by arithmetic alone: 16000 x 134218 = 2^31 + 4352 cells; nothing is allocated for a refused call
    assert 16000 * 134218 > _lib.DTW_MAX_PATH_CELLS >= 16000 * 134217
    with pytest.raises(hpfw_amd.HpfwError) as e:
        dt.dtw_path(long[:16000], 1)
    assert e.value.status == _lib.E_UNSUPPORTED and "2^31" in str(e.value)


def test_paths(dt):
    r, q, planted = ref.planted()
    few_r, few_q = _few(BLOCK + 70, 1), _few(120, 2)
    short = _rand(40, 3)
    clips = [r, few_r, short, _rand(30, 4)]
    _index(dt, clips)
    cases = [(q, 0), (few_q, 1), (_rand(70, 5), 2), (short[:1], 2), (few_q[:2], 1), (_rand(64, 6), 3)]
    for qq, ci in cases:
        hit, path = dt.dtw_path(qq, ci)
        want = ref.pair(qq, clips[ci], want_path=True)
        if want is None:
            assert tuple(int(v) for v in hit) == ref.PAD and (path == -1).all() and path.size == qq.size
            continue
        dist, start, end, wpath = want
        assert (int(hit["dist"]), int(hit["clip"]), int(hit["start"]), int(hit["end"])) == (dist, ci, start, end)
        assert path.dtype == np.int32 and np.array_equal(path, wpath), (ci, qq.size)
        assert ref.path_identities(qq, clips[ci], dist, start, end, path) == []
    assert ref.pair(cases[2][0], short) is not None and ref.pair(cases[5][0], clips[3]) is None   # 70 rows on 40 columns; 64 on 30
    hit, path = dt.dtw_path(q, 0)
    assert np.array_equal(path, planted) and int(hit["dist"]) <= 200


def test_planted_case_is_rank_one(dt):
    r, q, planted = ref.planted()
    clips = [_rand(2320, 900 + i) for i in range(5)]
    clips.insert(3, r)
    _index(dt, clips)
    got = dt.search_dtw(q, np.array([0, q.size]), 3, 0)
    assert (int(got[0, 0]["clip"]), int(got[0, 0]["start"]), int(got[0, 0]["end"])) == (3, int(planted[0]), int(planted[-1]))
    assert int(got[0, 0]["dist"]) <= 200 and int(got[0, 1]["dist"]) > 20 * 200
    # ... and by re-ranking the plain search's three best it may be missed or found, but what is returned is the rule's
    rr = dt.search_dtw(q, np.array([0, q.size]), 1, 3)
    assert int(rr[0, 0]["clip"]) != 3 or tuple(rr[0, 0]) == tuple(got[0, 0])


def test_top_warped_and_warp_path_end_to_end(tmp_path, filters, torch_cuda):
    """top_warped and warp_path on WAV files give what the Gpu calls give on the hashprints of the same files"""
    songs = np.stack([synth.gen_clip(i, 10.0) for i in range(4)])
    sr = synth.SR
    files = []
    for name, seg in (("a", songs[2][2 * sr:7 * sr]), ("b", songs[0][4 * sr:9 * sr]), ("c", synth.gen_clip(40, 5.0))):
        files.append(str(tmp_path / f"{name}.wav"))
        synth.write_wav(files[-1], np.ascontiguousarray(seg))
    cache = str(tmp_path / "cache") + "/"
    os.makedirs(cache)
    with open(os.path.join(cache, "filters.cereal"), "wb") as f:
        f.write(np.array([64, 2420], np.int32).tobytes() + np.ascontiguousarray(filters, np.float32).tobytes())
    lsi = hpfw_amd.LiveSongIdentification(cache=cache)
    try:
        ext = lsi.collector.gpu()
        names = [f"song{i:02d}" for i in range(4)]
        lsi.build(list(zip(list(ext.extract(songs)), names)))
        hps = [hp for hp, _ in lsi.collector.calc_hashprints(files)]
        q_hp, q_off = _lib._ragged(hps, np.uint64)
        for k, cand in ((3, 0), (2, 3)):
            got = lsi.top_warped(files, k, cand)
            want = lsi._gpu.search_dtw(q_hp, q_off, k, cand)
            assert [label for label, _ in got] == files
            for (label, hits), row in zip(got, want):
                assert hits == [(int(h["dist"]), names[int(h["clip"])], int(h["start"]), int(h["end"])) for h in row if h["clip"] != _lib.NO_CLIP]
        got = lsi.top_warped(files, 3, 0)
        assert got[0][1][0][1] == "song02" and got[1][1][0][1] == "song00"
        plain = lsi.top(files, 1)
        for i in (0, 1):                                  # the rigid alignment is one of the paths
            assert got[i][1][0][0] <= plain[i][1][0][0] and abs(got[i][1][0][2] - plain[i][1][0][2]) <= 8
        dist, cols = lsi.warp_path(files[0], "song02")
        hit, path = lsi._gpu.dtw_path(hps[0], 2)
        assert dist == int(hit["dist"]) == got[0][1][0][0] and cols.dtype == np.int32 and np.array_equal(cols, path)
        assert (cols[0], cols[-1]) == got[0][1][0][2:]
        sec = lsi.columns_to_seconds(cols)
        col_s = float(lsi.columns_to_seconds([1])[0])     # the excerpt begins 2 s into the song
        assert 0.005 < col_s < 0.03 and np.array_equal(sec, cols * col_s) and abs(sec[0] - 2.0) < 0.1
        with pytest.raises(KeyError):
            lsi.warp_path(files[0], "nobody")
        sharded = hpfw_amd.LiveSongIdentification.__new__(hpfw_amd.LiveSongIdentification)
        sharded._gpu = object.__new__(hpfw_amd.liveid._ShardedIndex)
        for call in (lambda: sharded.top_warped(files, 3, 0), lambda: sharded.warp_path(files[0], "song02")):
            with pytest.raises(hpfw_amd.HpfwError) as e:
                call()
            assert e.value.status == _lib.E_UNSUPPORTED
    finally:
        lsi._gpu.close()
