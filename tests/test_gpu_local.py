"""The local search on the GPU: every case runs under both kernel selections -- the fp4 matrix-core
scan and the xor/popcount kernel -- and is compared with the restatement of tests/local_ref.py field for field."""
import os

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, synth

import group_case
import local_ref as ref

pytestmark = pytest.mark.gpu
CHUNK = _lib.LOCAL_CHUNK
NONE = 0xFFFFFFFF
_REF = {}                                                # references computed once, shared by both kernel selections


@pytest.fixture(params=["mfma", "popcount"])
def kernel(request):
    """the default selection (matrix cores where the window fits the LDS) and the xor/popcount kernel for everything"""
    if request.param == "popcount":
        os.environ["HPFW_LOCAL_POPC"] = "1"
    yield request.param
    os.environ.pop("HPFW_LOCAL_POPC", None)


@pytest.fixture(scope="module")
def lc(torch_cuda):
    """a handle of this file's own: the searches need no filters, and the session's handle keeps its index"""
    g = hpfw_amd.Gpu(0)
    yield g
    g.close()


def _rand(n, seed):
    return np.random.default_rng([0x6C6F6361, seed]).integers(0, 2 ** 64, n, dtype=np.uint64)


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


def _check(g, db, queries, k, T, key):
    """search_local of the queries equals the restatement's first k columns (computed once per key for k = 64)"""
    q_hp, q_off = _lib._ragged(queries, np.uint64)
    if key not in _REF:
        _REF[key] = ref.search_local(db[0], db[1], q_hp, q_off, 64, T)
    got = g.search_local(q_hp, q_off, k, T)
    _same(got, _REF[key][:, :k], (key, k, T))
    return got


def _plant(q, j0, clip, p0, length):
    """query positions j0 .. j0 + length - 1 become clip positions p0 ..: a passage at lag p0 - j0"""
    q[j0:j0 + length] = clip[p0:p0 + length]
    return q


# ---- 1. sizes ---------------------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 5, 63, 64, 143, 304, 1023, 1024, 1025, 2320, 3000]
Q_LENGTHS = [1, 64, 143, 304, 305, 1000]


def test_ragged_index(lc, kernel):
    clips = [_rand(n, 100 + i) for i, n in enumerate(LENGTHS)]
    db = _index(lc, clips)
    queries = [_rand(k, 200 + i) for i, k in enumerate(Q_LENGTHS)]
    queries[0][:] = clips[9][700]                        # one hashprint, somewhere
    _plant(queries[3], 40, _flip(clips[11], 0.1, 1), 1000, 200)   # a noisy passage
    _plant(queries[5], 900, clips[10], 0, 100)           # the query's end on the clip's start
    for T in (1, 22, 31):
        for k in (1, 3, 64):
            got = _check(lc, db, queries, k, T, ("ragged", T))
        n_hit = (got["clip"] != NONE).sum(1)             # (k = 64: more slots than clips)
        assert (n_hit < 64).all() and n_hit[0] >= 1
        assert (got["score"][got["clip"] == NONE] == 0).all() and (got["score"][got["clip"] != NONE] >= 1).all()
        assert tuple(int(v) for v in got[0, 0]) == (T, 9, 700, 0, 1, 0)
        assert (int(got[5, 0]["clip"]), int(got[5, 0]["lag"])) == (10, -900) and int(got[5, 0]["score"]) >= T * 100
    want = _REF[("ragged", 1)]
    assert (want["clip"][1] == NONE).all() and (want["clip"][3] == NONE).all()   # at one bit per hashprint random words score nothing
    assert ((_REF[("ragged", 31)]["clip"] != NONE).sum(1) >= 9).all()            # ... and at 31 nearly every clip has a run
    for i in (0, 3):                                     # one query per call: the chunks begin at its own 1 - k
        for k in (1, 64):
            _check(lc, db, queries[i:i + 1], k, 22, (f"ragged, query {i} alone", 22))


# ---- 2. seams ---------------------------------------------------------------------------------------------------------------------
def test_chunk_seams(lc, kernel):
    """k = 304 for every query: the chunks of either kernel begin at lag -303 + 1024 i.  A query is a copy of the clip at its lag
    (random outside the clip), so that lag scores T per shared hashprint"""
    n, k, T = 3000, 304, 22
    clips = [_rand(700, 400), _rand(n, 401), _rand(1500, 402)]
    db = _index(lc, clips)
    seams = [1 - k + CHUNK * i + e for i in (1, 2, 3) for e in (-1, 0)]
    assert seams == [720, 721, 1744, 1745, 2768, 2769]
    lags = seams + [1 - k, 2 - k, -1, 0, n - k, n - k + 1, n - 2, n - 1]
    queries = []
    for i, d in enumerate(lags):
        j0, j1 = max(0, -d), min(k, n - d)
        queries.append(_plant(_rand(k, 410 + i), j0, clips[1], d + j0, j1 - j0))
    got = _check(lc, db, queries, 2, T, ("seams", T))
    for row, d in zip(got, lags):
        j0, j1 = max(0, -d), min(k, n - d)
        if j1 - j0 >= 2:                                 # (a single shared hashprint may be met elsewhere by a random run)
            assert (int(row[0]["clip"]), int(row[0]["lag"])) == (1, d) and int(row[0]["score"]) >= T * (j1 - j0), (d, row)
    # a longer query in the group moves the seams of the matrix-core scan to -999 + 1024 i: the same lags, other registers
    longer = queries + [_plant(_rand(1000, 440), 500, clips[2], 24, 300)]
    got = _check(lc, db, longer, 2, T, ("seams, a longer query in the group", T))
    assert (int(got[-1, 0]["clip"]), int(got[-1, 0]["lag"])) == (2, 24 - 500)
    moved = [1 - 1000 + CHUNK * i + e for i in (1, 2, 3) for e in (-1, 0)]
    queries = [_plant(_rand(1000, 450 + i), 100, clips[1], d + 100, 150) for i, d in enumerate(moved)]
    got = _check(lc, db, queries, 1, T, ("seams of a group of long queries", T))
    assert [int(v) for v in got["lag"][:, 0]] == moved


def test_runs_on_and_off_the_staged_chunks(lc, kernel):
    """the matrix-core scan stages the queries 16 positions at a time: runs that start and end on, and one off, multiples of 16"""
    T = 22
    clips = [_rand(2000, 500), _rand(300, 501)]
    db = _index(lc, clips)
    spans = [(j0 + a, j1 + b) for j0, j1 in ((16, 48), (0, 16), (32, 304), (288, 304), (160, 176)) for a in (-1, 0, 1) for b in (-1, 0, 1)
             if 0 <= j0 + a < j1 + b <= 304]
    queries = [_plant(_rand(304, 510 + i), j0, clips[0], 1000 + 7 * i + j0, j1 - j0) for i, (j0, j1) in enumerate(spans)]
    got = _check(lc, db, queries, 2, T, ("chunks of 16", T))
    for i, (row, (j0, j1)) in enumerate(zip(got, spans)):
        h = row[0]
        assert (int(h["clip"]), int(h["lag"])) == (0, 1000 + 7 * i), (i, h)
        # the planted run, grown at most by neighbours that happen to agree in more than 64 - T bits
        assert int(h["q_start"]) <= j0 and int(h["q_start"] + h["length"]) >= j1 and int(h["length"]) <= j1 - j0 + 4, (i, h)
        assert int(h["score"]) == T * int(h["length"]) - int(h["dist"]) >= T * (j1 - j0)


# ---- 3. batches and ties ------------------------------------------------------------------------------------------------------------
def _batch_queries(clips, n_q):
    queries = []
    for i in range(n_q):
        k = [1, 17, 64, 100, 143, 250, 304, 33, 0, 16][i % 10]
        q = _rand(k, 600 + i)
        if k >= 17 and i % 3:                            # two in three hold a noisy passage of some clip
            c = clips[1 + i % 4]
            length = min(k, c.size) * 2 // 3
            _plant(q, (k - length) // 2, _flip(c, 0.05 * (i % 3), i), (11 * i) % (c.size - length + 1), length)
        queries.append(q)
    return queries


def test_batches(lc, kernel):
    clips = [_rand(n, 550 + i) for i, n in enumerate([40, 1100, 300, 777, 1024, 0, 90])]
    db = _index(lc, clips)
    for n_q in (1, 7, 32, 33, 70):
        queries = _batch_queries(clips, n_q)
        for T in (22, 31):
            got = _check(lc, db, queries, 3, T, ("batch", n_q, T))
        assert (got["clip"][[len(q) == 0 for q in queries]] == NONE).all()
        assert got["clip"][[len(q) > 0 for q in queries], 0].max() < NONE


def test_query_groups(lc, kernel):
    """HPFW_LOCAL_TABLE_KB=1: the table holds 32 queries' rows (5 clips x 8 bytes each), so the 70 queries of group_case run in
    passes of 32, 32 and 6 -- the later passes' offsets into the queries and the hits, and the reuse of the table and the image.
    The call returns, so no winner's walk disagreed with the scan in any pass."""
    clips, queries = group_case.case()
    db = _index(lc, clips)
    T, k = 12, 2
    with group_case.env(HPFW_LOCAL_TABLE_KB=1):
        got = _check(lc, db, queries, k, T, ("query groups", T))
    assert got.tobytes() == lc.search_local(*_lib._ragged(queries, np.uint64), k, T).tobytes()
    assert "HPFW_LOCAL_TABLE_KB" not in os.environ
    for i in range(group_case.N_Q):                      # a planted passage of at least 11 hashprints: some 9 a hashprint
        assert (got[i, 0]["clip"] != NONE and got[i, 0]["score"] >= 60) == group_case.planted(i), i
    assert (got[group_case.EMPTY]["clip"] == NONE).all()
    assert int(got[group_case.LONG, 0]["clip"]) == 0 and int(got[group_case.LONG, 0]["length"]) >= 20   # the clip inside the query
    assert got[group_case.TWINS[0]].tobytes() == got[group_case.TWINS[1]].tobytes()


def test_ties_and_padding(lc, kernel):
    T = 22
    a, b = _rand(2000, 700), _rand(60, 701)
    passage = _rand(48, 702)
    a[100:148] = passage                                 # twice in clip 0: the smaller lag wins
    a[1500:1548] = passage
    c = _rand(500, 703)
    c[200:248] = passage                                 # ... and in clips 2 and 3: the smaller id wins
    clips = [a, b, c, c.copy(), _rand(1, 704)]
    db = _index(lc, clips)
    q1 = _plant(_rand(100, 710), 30, passage, 0, 48)
    q2 = np.concatenate([_rand(100, 711), b, _rand(140, 712)])   # a query longer than the clip, the clip inside it
    got = _check(lc, db, [q1, q2], 4, T, ("ties", T))
    assert [(int(h["clip"]), int(h["lag"])) for h in got[0, :3]] == [(0, 70), (2, 170), (3, 170)]
    assert (got[0, :3]["score"] == got[0, 0]["score"]).all() and int(got[0, 0]["score"]) >= T * 48
    assert tuple(int(v) for v in got[1, 0])[:3] == (T * 60, 1, -100) and int(got[1, 0]["length"]) == 60
    # an all-mismatch query: every hashprint of the index has at most 2 bits set, the query has all 64
    sparse = [np.uint64(1) << (_rand(n, 720 + i) % np.uint64(64)) | np.uint64(1) for i, n in enumerate([300, 1100])]
    db = _index(lc, sparse)
    ones = np.full(200, np.uint64(0xFFFFFFFFFFFFFFFF))
    for T in (1, 31):
        got = _check(lc, db, [ones, ones[:1], _rand(50, 730)], 2, T, ("all mismatch", T))
        assert (got["clip"][:2] == NONE).all() and [tuple(int(v) for v in h) for h in got[0]] == [ref.PAD, ref.PAD]
    # an empty index
    lc.index_clear()
    got = lc.search_local(ones, np.array([0, 100, 100, 200]), 3, 22)
    assert got.shape == (3, 3) and all(tuple(int(v) for v in h) == ref.PAD for h in got.ravel())


# ---- 4. queries whose window does not fit the LDS -------------------------------------------------------------------------------------
def test_large_queries(lc, kernel):
    """4 000 and 16 000 hashprints against a clip of 20 000: the xor/popcount kernel, asked for or not"""
    T = 22
    big = _rand(20000, 800)
    db = _index(lc, [_rand(10, 801), big, _rand(1500, 802)])
    q4 = _plant(_rand(4000, 810), 1000, _flip(big, 0.1, 5), 15000, 2500)
    q16 = _plant(_rand(16000, 811), 9000, _flip(big, 0.1, 6), 2000, 6000)
    for name, q in (("4000", q4), ("16000", q16)):
        got = _check(lc, db, [q], 2, T, ("large", name, T))
        h = got[0, 0]
        assert int(h["clip"]) == 1 and int(h["score"]) > T * 1000
    assert int(_REF[("large", "4000", T)][0, 0]["lag"]) == 14000 and int(_REF[("large", "16000", T)][0, 0]["lag"]) == -7000
    with pytest.raises(hpfw_amd.HpfwError) as e:
        lc.search_local(_rand(16001, 812), np.array([0, 16001]), 1, T)
    assert e.value.status == _lib.E_UNSUPPORTED


# ---- 5. API -----------------------------------------------------------------------------------------------------------------------
def _api_case(lc):
    clips = [_rand(n, 900 + i) for i, n in enumerate([500, 64, 1200, 300, 0, 800, 2100])]
    db = _index(lc, clips)
    queries = []
    for i, k in enumerate([304, 64, 0, 305, 143] * 8):
        q = _rand(k, 920 + i)
        if k >= 64:
            c = clips[[0, 2, 5, 6][i % 4]]
            length = min(k - 20, 200)
            _plant(q, 10, _flip(c, 0.08, i), (13 * i) % (c.size - length), length)
        queries.append(q)
    return clips, db, queries


def test_device_pointers_on_a_side_stream(lc, kernel, torch_cuda):
    torch = torch_cuda
    _, _, queries = _api_case(lc)
    q_hp, q_off = _lib._ragged(queries, np.uint64)
    want = lc.search_local(q_hp, q_off, 4, 22)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_q = torch.from_numpy(q_hp.view(np.int64)).cuda()
        d_out = torch.zeros(len(queries) * 4 * 24, dtype=torch.uint8, device="cuda")
        lc.search_local_dev(d_q.data_ptr(), q_off, 4, 22, d_out.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    assert d_out.cpu().numpy().tobytes() == want.tobytes()
    assert (want["clip"][:, 0] != NONE).sum() == sum(len(q) > 0 for q in queries)


def test_clip_base_and_removed_clips(lc, kernel):
    clips, db, queries = _api_case(lc)
    got = _check(lc, db, queries, 3, 22, ("api", 22))
    lc.index_set_clip_base(1000)
    try:
        based = lc.search_local(*_lib._ragged(queries, np.uint64), 3, 22)
    finally:
        lc.index_set_clip_base(0)
    want = got.copy()
    want["clip"][got["clip"] != NONE] += 1000
    _same(based, want, "clip_base")
    # removed clips are empty clips: ids stay, their hashprints are gone
    lc.index_remove([2, 5])
    left = [c if i not in (2, 5) else c[:0] for i, c in enumerate(clips)]
    got = _check(lc, _lib._ragged(left, np.uint64), queries, 3, 22, ("api, clips 2 and 5 removed", 22))
    assert not np.isin(got["clip"], [2, 5]).any() and np.isin(_REF[("api", 22)]["clip"][:, 0], [2, 5]).any()


def test_bad_arguments_with_an_index(lc):
    _index(lc, [_rand(100, 990)])
    q = _rand(10, 991)
    for kw, status in ((dict(k=0), _lib.E_INVALID), (dict(k=65), _lib.E_INVALID), (dict(max_rate=0), _lib.E_INVALID),
                       (dict(max_rate=32), _lib.E_INVALID)):
        with pytest.raises(hpfw_amd.HpfwError) as e:
            lc.search_local(q, np.array([0, 10]), **{"k": 1, "max_rate": 22, **kw})
        assert e.value.status == status, kw


def test_top_local_end_to_end(tmp_path, filters, torch_cuda, kernel):
    """the half-shared query of DESIGN.md section 25 as a WAV file: eight songs of 10 s in the index; a query of 5 s whose first
    60 % is song 3 from second 2 on and whose rest is a song that is not indexed, at gain 0.5 and 10 dB SNR"""
    sr, T = synth.SR, 22
    songs = np.stack([synth.gen_clip(i, 10.0) for i in range(8)])
    files = [str(tmp_path / "half.wav"), str(tmp_path / "short.wav")]
    synth.write_wav(files[0], ref.half_shared_query(songs[3], synth.gen_clip(103, 10.0), 5.0, 0.6, 2.0, 10.0, 3))
    synth.write_wav(files[1], np.zeros(sr // 2, np.int16))     # too short for a hashprint
    names = [f"song{i:02d}" for i in range(8)]
    cache = str(tmp_path / "cache") + "/"                # the collector reads the filter fixture as it reads learned filters
    os.makedirs(cache)
    with open(os.path.join(cache, "filters.cereal"), "wb") as f:
        f.write(np.array([64, 2420], np.int32).tobytes() + np.ascontiguousarray(filters, np.float32).tobytes())
    lsi = hpfw_amd.LiveSongIdentification(cache=cache)
    try:
        index = list(lsi.collector.gpu().extract(songs))
        lsi.build(list(zip(index, names)))
        got = lsi.top_local(files, 3, T)
        assert got[1] == (files[1], None) and got[0][0] == files[0]
        q = lsi.collector.calc_hashprints(files[:1])[0][0]
        db_hp, db_off = _lib._ragged(index, np.uint64)
        if "e2e" not in _REF:
            _REF["e2e"] = ref.search_local(db_hp, db_off, q, np.array([0, q.size]), 3, T)[0]
        assert got[0][1] == [(int(h["score"]), names[int(h["clip"])], int(h["lag"]), int(h["q_start"]), int(h["length"]), int(h["dist"]))
                             for h in _REF["e2e"] if h["clip"] != NONE]
        score, name, lag, q_start, length, dist = got[0][1][0]
        print(f"top_local: {got[0][1]}")
        assert name == "song03" and score >= 4 * got[0][1][1][0] and abs(lag - 161) <= 1 and abs(q_start + length - 143) <= 45
        assert score == T * length - dist
        sharded = hpfw_amd.LiveSongIdentification.__new__(hpfw_amd.LiveSongIdentification)
        sharded._gpu = object.__new__(hpfw_amd.liveid._ShardedIndex)
        with pytest.raises(hpfw_amd.HpfwError) as e:
            sharded.top_local(files, 3, T)
        assert e.value.status == _lib.E_UNSUPPORTED
    finally:
        lsi._gpu.close()
