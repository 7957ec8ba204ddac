"""The overlap search on the GPU: every case runs under both kernel selections -- the fp4 matrix-core
scan and the xor/popcount kernel -- and is compared with the restatement of tests/overlap_ref.py field for field."""
import os

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, synth

import group_case
import overlap_ref as ref
import overlap_score_ref

pytestmark = pytest.mark.gpu
CHUNK = _lib.OVERLAP_CHUNK
_REF = {}                                                # references computed once, shared by both kernel selections


@pytest.fixture(params=["mfma", "popcount"])
def kernel(request):
    """the default selection (matrix cores where the window fits the LDS) and the xor/popcount kernel for everything"""
    if request.param == "popcount":
        os.environ["HPFW_OVERLAP_POPC"] = "1"
    yield request.param
    os.environ.pop("HPFW_OVERLAP_POPC", None)


@pytest.fixture(scope="module")
def ov(torch_cuda):
    """a handle of this file's own: the searches need no filters, and the session's handle keeps its index"""
    g = hpfw_amd.Gpu(0)
    yield g
    g.close()


def _rand(n, seed):
    return np.random.default_rng([0x6F766C70, seed]).integers(0, 2 ** 64, n, dtype=np.uint64)


def _flip(hp, fraction, seed):
    """hp with that fraction of its bits flipped"""
    rng = np.random.default_rng([0x666C6970, seed])
    mask = np.zeros(hp.size, np.uint64)
    for b in range(64):
        mask |= (rng.random(hp.size) < fraction).astype(np.uint64) << np.uint64(b)
    return hp ^ mask


def _index(g, clips):
    db_hp, db_off = _lib._ragged(clips, np.uint64)
    g.index_clear()
    g.index_set_clip_base(0)
    g.index_add(db_hp, db_off)
    return db_hp, db_off


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)[0]
        raise AssertionError(f"{what}: first difference at {tuple(bad)}: got {got[tuple(bad)]}, want {want[tuple(bad)]}")


def _check(g, db, queries, k, mo, key, exclude=None):
    """search_overlap of the queries equals the restatement's first k columns (computed once per key for k = 64)"""
    q_hp, q_off = _lib._ragged(queries, np.uint64)
    if key not in _REF:
        cache = _REF.setdefault(key[0], {})
        _REF[key] = ref.search_overlap(db[0], db[1], q_hp, q_off, 64, mo, exclude=exclude, cache=cache)
    got = g.search_overlap(q_hp, q_off, k, mo, exclude=exclude)
    _same(got, _REF[key][:, :k], (key, k, mo))
    return got


LENGTHS = [0, 1, 5, 63, 64, 143, 304, 305, 1023, 1024, 1025, 2320, 3000]
Q_LENGTHS = [1, 64, 143, 304, 305, 1000]


def _ragged_clips():
    return [_rand(n, 100 + i) for i, n in enumerate(LENGTHS)]


def test_ragged_index(ov, kernel):
    clips = _ragged_clips()
    db = _index(ov, clips)
    queries = [_rand(k, 200 + i) for i, k in enumerate(Q_LENGTHS)]
    queries[3][:] = _flip(clips[11][1000:1304], 0.2, 1)   # (one query that belongs somewhere)
    n_cand = {mo: sum(n >= mo for n in LENGTHS) for mo in (1, 64, 100)}
    assert n_cand == {1: 12, 64: 9, 100: 8}               # more than k = 1, 3, 10 at 1; fewer than 10 at 100; fewer than 64 always
    for mo in (1, 64, 100):
        for k in (1, 3, 10, 64):
            got = _check(ov, db, queries, k, mo, ("ragged", mo))
            n_hit = (got["clip"] != 0xFFFFFFFF).sum(1)
            assert [int(v) for v in n_hit] == [min(k, n_cand[mo]) if kq >= mo else 0 for kq in Q_LENGTHS]
    for i, kq in enumerate(Q_LENGTHS):                    # min_overlap = the query's length: one query per call
        for k in (1, 3, 10, 64):
            _check(ov, db, queries[i:i + 1], k, kq, (f"ragged, query {i} alone", kq))


def test_planted_matches(ov, kernel):
    clips = _ragged_clips()
    db = _index(ov, clips)
    want_lag, queries = [], []
    for noise in (0.0, 0.1):
        a = _rand(304, 300)                               # the query's last 100 are clip 11's first 100
        a[204:] = _flip(clips[11][:100], noise, 2)
        b = _rand(304, 301)                               # the query's first 120 are clip 12's last 120
        b[:120] = _flip(clips[12][-120:], noise, 3)
        c = _rand(304, 302)                               # the 143-hashprint clip sits inside the query from position 80
        c[80:223] = _flip(clips[5], noise, 4)
        queries += [a, b, c]
        want_lag += [(11, -204, 100), (12, 3000 - 120, 120), (5, -80, 143)]
    got = _check(ov, db, queries, 3, 100, ("planted", 100))
    for row, (clip, lag, L) in zip(got, want_lag):
        assert (int(row[0]["clip"]), int(row[0]["lag"]), int(row[0]["overlap"])) == (clip, lag, L), row
    assert (got["dist"][:3, 0] == 0).all() and (got["dist"][3:, 0] > 0).all()
    # random hashprints disagree in 32 bits of 64 (sigma 4 / sqrt(L) per hashprint); a tenth flipped is 6.4
    assert (got["dist"][3:, 0] < 10 * got["overlap"][3:, 0]).all() and (got["dist"][:, 1] > 28 * got["overlap"][:, 1]).all()


def test_chunk_boundaries(ov, kernel):
    """k = 304 for every query and min_overlap = 100: the chunks of either kernel begin at lag -204 + 1024 i.  A query is a
    copy of the clip at its lag (random outside the clip), so that lag has rate 0"""
    n, k, mo = 3000, 304, 100
    clips = [_rand(700, 400), _rand(n, 401), _rand(1500, 402)]
    db = _index(ov, clips)
    seams = [mo - k + CHUNK * i + e for i in (1, 2, 3) for e in (-1, 0)]
    assert seams == [819, 820, 1843, 1844, 2867, 2868]
    lags = seams + [mo - k, -1, 0, n - k, n - k + 1, n - mo]
    queries = []
    for i, d in enumerate(lags):
        q = _rand(k, 410 + i)
        j0, j1 = max(0, -d), min(k, n - d)
        q[j0:j1] = clips[1][d + j0:d + j1]
        queries.append(q)
    for splits in (None, "1", "3"):                      # the default deals the chunks to workgroups; 1: one walks them all
        if splits:
            os.environ["HPFW_OVERLAP_SPLITS"] = splits
        try:
            got = _check(ov, db, queries, 2, mo, ("seams", mo))
        finally:
            os.environ.pop("HPFW_OVERLAP_SPLITS", None)
        assert [int(v) for v in got["lag"][:, 0]] == lags and (got["clip"][:, 0] == 1).all() and (got["dist"][:, 0] == 0).all()
        assert [int(v) for v in got["overlap"][:, 0]] == [ref.overlap(k, n, d) for d in lags]


def test_query_counts(ov, kernel):
    """1, 7, 32, 33 and 70 queries of mixed lengths in one call: padded rows, more than one group, groups whose longest
    query differs"""
    clips = [_rand(n, 500 + i) for i, n in enumerate([700, 90, 1100, 304, 40, 257])]
    db = _index(ov, clips)
    rng = np.random.default_rng(501)
    queries = []
    for i in range(70):
        kq = int(rng.choice([0, 20, 39, 40, 41, 100, 257, 304, 305, 420]))
        q = _rand(kq, 510 + i)
        if i % 3 == 0 and kq >= 40:                       # part of the query is part of a clip
            c = clips[(0, 2, 5)[i % 9 // 3]]
            o = int(rng.integers(0, c.size - 40))
            m = min(kq, c.size - o)
            q[kq - m:] = _flip(c[o:o + m], 0.05, i)
        queries.append(q)
    for n_q in (1, 7, 32, 33, 70):
        q_hp, q_off = _lib._ragged(queries[:n_q], np.uint64)
        if "counts" not in _REF:
            all_hp, all_off = _lib._ragged(queries, np.uint64)
            _REF["counts"] = ref.search_overlap(db[0], db[1], all_hp, all_off, 5, 40)
        _same(ov.search_overlap(q_hp, q_off, 5, 40), _REF["counts"][:n_q], n_q)


def test_long_queries(ov, kernel):
    """queries whose window does not fit the LDS go through the xor/popcount kernel without the switch"""
    clips = [_rand(20000, 600), _rand(7000, 601), _rand(300, 602)]
    db = _index(ov, clips)
    q4, q16 = _rand(4000, 610), _rand(16000, 611)
    q4[1000:] = _flip(clips[1][:3000], 0.1, 5)            # lag -1000, overlap 3000
    q16[:9000] = _flip(clips[0][11000:], 0.1, 6)          # lag 11000, overlap 9000
    got = _check(ov, db, [q4, q16], 3, 250, ("long", 250))
    assert [(int(r[0]["clip"]), int(r[0]["lag"]), int(r[0]["overlap"])) for r in got] == [(1, -1000, 3000), (0, 11000, 9000)]


def test_device_pointers_on_a_side_stream(ov, kernel, torch_cuda):
    torch = torch_cuda
    clips = _ragged_clips()
    _index(ov, clips)
    queries = [_rand(k, 700 + i) for i, k in enumerate([304, 64, 0, 305, 143] * 8)]
    q_hp, q_off = _lib._ragged(queries, np.uint64)
    exclude = np.array([(i % 14) - 1 for i in range(len(queries))], np.int32)
    want = ov.search_overlap(q_hp, q_off, 4, 64, exclude=exclude)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_q = torch.from_numpy(q_hp.view(np.int64)).cuda()
        d_out = torch.zeros(len(queries) * 4 * 16, dtype=torch.uint8, device="cuda")
        ov.search_overlap_dev(d_q.data_ptr(), q_off, 4, 64, d_out.data_ptr(), exclude=exclude, stream=side.cuda_stream)
    side.synchronize()
    assert d_out.cpu().numpy().tobytes() == want.tobytes()
    assert (want["clip"] != 0xFFFFFFFF).any()


def test_exclude_all_against_all(ov, kernel):
    clips = [_rand(n, 800 + i) for i, n in enumerate([400, 350, 500, 304, 450, 600, 380, 420])]
    clips[6] = clips[2].copy()                            # duplicates find each other at lag 0
    clips[1][:200] = _flip(clips[5][400:], 0.1, 7)        # the start of clip 1 continues clip 5
    db = _index(ov, clips)
    me = np.arange(8, dtype=np.int32)
    got = _check(ov, db, clips, 3, 100, ("all", "but itself"), exclude=me)
    assert not (got["clip"] == me[:, None]).any()
    assert tuple(int(v) for v in got[2, 0]) == (0, 6, 0, 500) and tuple(int(v) for v in got[6, 0]) == (0, 2, 0, 500)
    assert (int(got[1, 0]["clip"]), int(got[1, 0]["lag"]), int(got[1, 0]["overlap"])) == (5, 400, 200)
    assert (int(got[5, 0]["clip"]), int(got[5, 0]["lag"]), int(got[5, 0]["overlap"])) == (1, -400, 200)
    none = _check(ov, db, clips, 3, 100, ("all", "none left out"), exclude=np.full(8, -1, np.int32))
    # without it everything finds itself, the second of the duplicates the first
    assert [int(c) for c in none["clip"][:, 0]] == [0, 1, 2, 3, 4, 5, 2, 7] and (none["dist"][:, 0] == 0).all()
    for bad in (8, 100):
        with pytest.raises(hpfw_amd.HpfwError) as e:
            ov.search_overlap(db[0], db[1], 3, 100, exclude=np.array([0, 1, 2, 3, 4, 5, 6, bad], np.int32))
        assert e.value.status == _lib.E_INVALID and "exclude" in str(e.value)
    ov.index_set_clip_base(1000)                          # hits carry clip_base, exclude does not
    try:
        based = ov.search_overlap(db[0], db[1], 3, 100, exclude=me)
    finally:
        ov.index_set_clip_base(0)
    want = got.copy()
    want["clip"][got["clip"] != 0xFFFFFFFF] += 1000
    _same(based, want, "clip_base")


def test_query_groups(ov, kernel):
    """HPFW_OVERLAP_TABLE_KB=4 with two splits a clip: the table holds 32 queries' rows (5 clips x 2 splits x 16 bytes each,
    5 KiB -- the floor), so the 70 queries of group_case run in passes of 32, 32 and 6.  `exclude` names another clip for
    every query, so a later pass must read its own part of it; plain and scored."""
    clips, queries = group_case.case()
    db = _index(ov, clips)
    q_hp, q_off = _lib._ragged(queries, np.uint64)
    mo, k = 8, 3
    exclude = [(-1, 0, 1, 3, 4)[i % 5] for i in range(group_case.N_Q)]
    with group_case.env(HPFW_OVERLAP_TABLE_KB=4, HPFW_OVERLAP_SPLITS=2):
        got = _check(ov, db, queries, k, mo, ("query groups", mo), exclude=exclude)
        hits, stats = ov.search_overlap_scored(q_hp, q_off, k, mo, exclude=exclude)
    assert "HPFW_OVERLAP_TABLE_KB" not in os.environ and "HPFW_OVERLAP_SPLITS" not in os.environ
    assert got.tobytes() == hits.tobytes() == ov.search_overlap(q_hp, q_off, k, mo, exclude=exclude).tobytes()
    one_pass = ov.search_overlap_scored(q_hp, q_off, k, mo, exclude=exclude)
    assert hits.tobytes() == one_pass[0].tobytes() and stats.tobytes() == one_pass[1].tobytes()
    if "query groups, moments" not in _REF:
        _REF["query groups, moments"] = [overlap_score_ref.row_moments(overlap_score_ref.candidates(db[0], db[1], q, mo), ex)
                                         for q, ex in zip(queries, exclude)]
    assert [(int(r["n"]), int(r["sum"]), int(r["sum_sq"])) for r in stats] == _REF["query groups, moments"]
    for i, (q, ex) in enumerate(zip(queries, exclude)):  # every clip of 8 hashprints or more but the excluded one, if the query has 8
        live = [c for c, n in enumerate(group_case.CLIP_LENGTHS) if n >= mo and c != ex] if len(q) >= mo else []
        assert (got[i]["clip"] != 0xFFFFFFFF).sum() == min(k, len(live)) and ex not in got[i]["clip"], i
    assert (got[group_case.EMPTY]["clip"] == 0xFFFFFFFF).all()
    assert int(got[group_case.LONG, 0]["clip"]) == 0 and int(got[group_case.LONG, 0]["overlap"]) == 40   # it overhangs clip 0 on both sides


def test_min_overlap_k_is_search_topk(ov, kernel):
    clips = [_rand(n, 900 + i) for i, n in enumerate([304, 305, 400, 1024, 1330, 2320, 304, 777, 3000])]
    db = _index(ov, clips)
    queries = [_flip(clips[c][o:o + 304], 0.1, 10 + c) for c, o in ((1, 1), (3, 720), (5, 2016), (6, 0), (8, 2696), (4, 1026))]
    queries += [_rand(304, 950 + i) for i in range(34)]
    q_hp, q_off = _lib._ragged(queries, np.uint64)
    for k in (1, 10):
        plain = ov.search_topk(q_hp, q_off, k)
        got = ov.search_overlap(q_hp, q_off, k, 304)
        assert np.array_equal(got["dist"], plain["dist"]) and np.array_equal(got["clip"], plain["clip"])
        assert np.array_equal(got["lag"], plain["offset"])
        assert np.array_equal(got["overlap"], np.where(plain["clip"] != 0xFFFFFFFF, 304, 0))     # (nine clips: k = 10 pads)
    assert [int(c) for c in got["clip"][:6, 0]] == [1, 3, 5, 6, 8, 4]


def test_empty_inputs(ov, kernel):
    pad = np.zeros(1, _lib.OVERLAP_HIT_DTYPE)
    pad[0] = ref.PAD
    ov.index_clear()
    q_hp, q_off = _lib._ragged([_rand(304, 1), _rand(5, 2)], np.uint64)
    got = ov.search_overlap(q_hp, q_off, 3, 4)
    assert got.shape == (2, 3) and (got == pad[0]).all()                      # an empty index
    db = _index(ov, [_rand(400, 3), _rand(0, 4), _rand(3, 5)])
    got = ov.search_overlap(q_hp, q_off, 3, 6)
    assert int(got[0, 0]["clip"]) == 0 and (got[0, 1:] == pad[0]).all() and (got[1] == pad[0]).all()   # a query below min_overlap
    _same(got, ref.search_overlap(db[0], db[1], q_hp, q_off, 3, 6), "short query")
    got = ov.search_overlap(np.zeros(1, np.uint64), np.zeros(3, np.int64), 2, 1)
    assert (got == pad[0]).all()                                               # empty queries
    assert ov.search_overlap(np.zeros(1, np.uint64), np.zeros(1, np.int64), 2, 1).shape == (0, 2)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _noisy(x, seed):
    """gain 0.5 and white noise at 10 dB SNR, as synth.gen_query makes its queries"""
    seg = 0.5 * x.astype(np.float64)
    rng = np.random.default_rng([0x6E6F6973, seed])
    p = float(np.mean(seg ** 2)) + 1e-12
    seg = seg + np.sqrt(p / 10 ** (10.0 / 10)) * rng.standard_normal(seg.size)
    return np.clip(np.round(seg), -32768, 32767).astype(np.int16)


def test_top_overlap_end_to_end(tmp_path, filters, oracle, torch_cuda, kernel):
    """six songs of 10 s and a 3 s item; five 5 s queries: A begins 2 s before song 2 does, B runs 2 s past the end of song 1,
    C holds the whole item, D lies inside song 4, E is not in the index"""
    sr = synth.SR
    songs = np.stack([synth.gen_clip(i, 10.0) for i in range(6)])
    item = synth.gen_clip(50, 3.0)
    other = [synth.gen_clip(100 + i, 5.0) for i in range(4)]
    pcm = {"A": np.concatenate([other[0][:2 * sr], songs[2][:3 * sr]]),
           "B": np.concatenate([songs[1][-3 * sr:], other[1][:2 * sr]]),
           "C": np.concatenate([other[2][:sr], item, other[2][sr:2 * sr]]),
           "D": songs[4][2 * sr:7 * sr],
           "E": other[3]}
    files = []
    for i, (name, x) in enumerate(pcm.items()):
        assert x.size == 5 * sr
        pcm[name] = _noisy(x, i)
        files.append(str(tmp_path / f"{name}.wav"))
        synth.write_wav(files[-1], pcm[name])
    cache = str(tmp_path / "cache") + "/"                # the collector reads the filter fixture as it reads learned filters
    os.makedirs(cache)
    with open(os.path.join(cache, "filters.cereal"), "wb") as f:
        f.write(np.array([64, 2420], np.int32).tobytes() + np.ascontiguousarray(filters, np.float32).tobytes())
    lsi = hpfw_amd.LiveSongIdentification(cache=cache)
    try:
        ext = lsi.collector.gpu()
        hp = list(ext.extract(songs)) + [ext.extract(item[None])[0]]
        names = [f"song{i:02d}" for i in range(6)] + ["item"]
        lsi.build(list(zip(hp, names)))
        got = lsi.top_overlap(files, 3, 100)
        plain = lsi.top(files, 1)
        mode = oracle.get_projection()
        oracle.set_projection(ext.get_projection())
        try:
            if "e2e" not in _REF:
                idx = list(oracle.Plan(10 * sr).extract_batch(filters, songs, 16)) + [oracle.Plan(3 * sr).extract(filters, item)]
                q = oracle.Plan(5 * sr).extract_batch(filters, np.stack(list(pcm.values())), 16)
                db_hp, db_off = _lib._ragged(idx, np.uint64)
                q_hp, q_off = _lib._ragged(list(q), np.uint64)
                _REF["e2e"] = ([h.size for h in idx], q.shape, ref.search_overlap(db_hp, db_off, q_hp, q_off, 3, 100))
        finally:
            oracle.set_projection(mode)
        sizes, q_shape, want = _REF["e2e"]
        assert sizes == [707] * 6 + [143] and q_shape == (5, 304) and [h.size for h in hp] == sizes
        col_s = 5.0 / 403.0                                 # 5 s are 403 columns of the spectrogram: 80.6 a second
        for (label, hits), f, row in zip(got, files, want):
            print(os.path.basename(f), [(d, nm, lag, L, round(d / L, 2)) for d, nm, lag, L in hits])
            assert label == f and len(hits) == 3
            assert [(d, names.index(nm), lag, L) for d, nm, lag, L in hits] == [tuple(int(v) for v in h) for h in row]
        for (label, hits), clip, seconds in zip(got[:4], (2, 1, 6, 4), (-2.0, 7.0, -1.0, 2.0)):
            assert names.index(hits[0][1]) == clip and abs(hits[0][2] - seconds / col_s) <= 2, (label, hits[0])
        # the plain rule compares the item over its own 143 hashprints at offset 0, on another scale: it names the item for
        # everything that is not a full window of a song
        assert [plain[i][1][0][1] for i in (0, 1, 2, 4)] == ["item"] * 4
        # a sharded identifier has no overlap search
        sharded = hpfw_amd.LiveSongIdentification.__new__(hpfw_amd.LiveSongIdentification)
        sharded._gpu = object.__new__(hpfw_amd.liveid._ShardedIndex)
        with pytest.raises(hpfw_amd.HpfwError) as e:
            sharded.top_overlap(files, 3, 100)
        assert e.value.status == _lib.E_UNSUPPORTED
    finally:
        lsi._gpu.close()
