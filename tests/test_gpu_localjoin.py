"""The local self-join on the GPU: every case runs under both kernel selections -- the fp4 matrix-core
scan with its slice loop and the xor/popcount kernel -- and is compared with the restatement of tests/localjoin_ref.py field
for field."""
import ctypes
import os

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, synth

import localjoin_ref as ref

pytestmark = pytest.mark.gpu
SEED = 20261021
_REF = {}                                                # candidates computed once per index and T, shared by both kernel selections


@pytest.fixture(params=["mfma", "popcount"])
def kernel(request):
    if request.param == "popcount":
        os.environ["HPFW_LOCALJOIN_POPC"] = "1"
    yield request.param
    os.environ.pop("HPFW_LOCALJOIN_POPC", None)


@pytest.fixture(scope="module")
def lj(torch_cuda):
    """a handle of this file's own: the join needs no filters, and the session's handle keeps its index"""
    g = hpfw_amd.Gpu(0)
    yield g
    g.close()


def _rand(n, seed):
    return np.random.default_rng([SEED, seed]).integers(0, 2 ** 64, n, dtype=np.uint64)


def _flip(hp, fraction, seed):
    """hp with that fraction of its bits flipped"""
    rng = np.random.default_rng([SEED, 0x666C6970, seed])
    mask = np.zeros(hp.size, np.uint64)
    for b in range(64):
        mask |= (rng.random(hp.size) < fraction).astype(np.uint64) << np.uint64(b)
    return hp ^ mask


def _index(g, clips, base=0):
    db_hp, db_off = _lib._ragged(clips, np.uint64)
    g.index_clear()
    g.index_set_clip_base(base)
    g.index_add(db_hp, db_off)
    return db_hp, db_off


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: first difference at {bad}: got {got[bad]}, want {want[bad]}")


def _check(g, db, T, min_score, key, base=0):
    """index_localjoin equals the restatement (the candidates of an index are computed once per key and T)"""
    want = ref.localjoin(db[0], db[1], T, min_score, clip_base=base, cache=_REF.setdefault(key, {}))
    got = g.index_localjoin(T, min_score)
    _same(got, want, (key, T, min_score))
    return got


def _pairs(recs):
    return [(int(p["a"]), int(p["b"])) for p in recs]


# ---- the ragged index: 40 clips, two row groups (the triangle cuts inside the first, the second is partial) ----------------
LENGTHS = [0, 3, 7, 8, 9, 31, 32, 33, 64, 100, 143, 200, 255, 256, 257, 304]
FIXED = {18: 300, 19: 599, 20: 400, 21: 60, 22: 520, 23: 100, 24: 500, 33: 90, 36: 200, 38: 333}


def _ragged_clips():
    rng = np.random.default_rng([SEED, 1])
    lengths = LENGTHS + [int(v) for v in rng.integers(8, 600, 24)]
    for i, n in FIXED.items():
        lengths[i] = n
    clips = [_rand(n, 100 + i) for i, n in enumerate(lengths)]
    p, q, r, s = (_rand(60, 900 + i) for i in range(4))
    clips[18][20:80] = p                                  # a passage of 60 shared by two clips at different positions,
    clips[19][300:360] = p
    clips[20][100:160] = _flip(p, 0.1, 1)                 # and by a third with a tenth of its bits flipped
    clips[21] = q                                         # a clip that lies twice in one b: the smaller lag
    clips[22][50:110] = q
    clips[22][400:460] = q
    clips[16] = clips[11].copy()                          # an exact copy (200)
    clips[24][150:250] = clips[23]                        # a short clip wholly inside a long one
    clips[12][100:160] = r                                # a of the first row group, b in the second
    clips[36][5:65] = r
    clips[33][:60] = s                                    # both in the second row group
    clips[38][-60:] = s
    assert len(clips) == 40 and all(c.size <= 599 for c in clips)
    return clips


NOISY = {(18, 20), (19, 20)}
PLANTED = {(11, 16), (18, 19), (21, 22), (23, 24), (12, 36), (33, 38)} | NOISY
# T: (the planted pairs that score, a min_score between their scores and every other pair's).  The smallest planted score is
# that of 60 hashprints with 6.4 bits flipped on average, 60 (T - 6.4): none at T = 1, some 940 at 22, some 1 480 at 31; an
# exact passage of 60 scores 60 T.  Random hashprints differ in 32 +- 4 bits, a step of T - 32 +- 4: at T = 1 and 22 a run
# of them is a few steps of luck (at most 64 T), at T = 31 the drift is -1 a step and runs of some 200 occur.
MIDDLE = {1: (PLANTED - NOISY, 30), 22: (PLANTED, 300), 31: (PLANTED, 600)}


def test_ragged_index(lj, kernel):
    clips = _ragged_clips()
    db = _index(lj, clips)
    for T, (planted, middle) in MIDDLE.items():
        cand = ref.candidates(db[0], db[1], T, cache=_REF.setdefault("ragged", {}))
        top_other = max([v[0] for pair, v in cand.items() if pair not in planted], default=0)
        low_planted = min(cand[pair][0] for pair in planted)
        print(f"T {T}: smallest planted score {low_planted}, largest other score {top_other}, {len(cand)} pairs score at least 1")
        assert 2 * top_other <= middle <= low_planted // 2
        everything = _check(lj, db, T, 1, "ragged")
        assert everything.size == len(cand) and (everything["a"] < everything["b"]).all() and (everything["pad"] == 0).all()
        assert (everything["score"] == T * everything["length"].astype(np.int64) - everything["dist"]).all()
        got = _check(lj, db, T, middle, "ragged")
        assert _pairs(got) == sorted(planted)
        by_pair = {pair: p for pair, p in zip(_pairs(got), got)}
        assert tuple(int(v) for v in by_pair[(11, 16)])[2:7] == (200 * T, 0, 0, 200, 0)
        assert tuple(int(v) for v in by_pair[(23, 24)])[2:7] == (100 * T, 150, 0, 100, 0)
        for pair, lag in (((18, 19), 280), ((21, 22), 50), ((12, 36), -95), ((33, 38), 273)):
            p = by_pair[pair]
            assert int(p["lag"]) == lag and int(p["score"]) >= 60 * T and int(p["length"]) >= 60, p
        assert _check(lj, db, T, 200 * T + 1, "ragged").size == 0       # above every score
        os.environ["HPFW_LOCALJOIN_TABLE_KB"] = "12"      # one row group of 40 clips is 10 KiB: a pass per group
        try:
            _check(lj, db, T, 1, "ragged")
            _check(lj, db, T, middle, "ragged")
            _same(lj.index_localjoin(T, 1, cap=max(everything.size - 50, 1)), everything, "two passes, growing and repeating")
        finally:
            os.environ.pop("HPFW_LOCALJOIN_TABLE_KB", None)


def test_cross_check_against_search_local(lj, kernel):
    """the same pairs by the local search all-against-all (which computes both orders of every pair), a < b taken"""
    clips = _ragged_clips()
    db = _index(lj, clips)
    for T in (22, 31):
        pairs = lj.index_localjoin(T, 1)
        hits = lj.search_local(db[0], db[1], 64, T)
        by_pair = {(a, int(h["clip"])): tuple(int(h[f]) for f in ("score", "lag", "q_start", "length", "dist"))
                   for a, row in enumerate(hits) for h in row if h["clip"] != 0xFFFFFFFF and a < int(h["clip"])}
        assert pairs.size == len(by_pair) and pairs.size > 100
        for p in pairs:
            assert by_pair[(int(p["a"]), int(p["b"]))] == tuple(int(p[f]) for f in ("score", "lag", "a_start", "length", "dist")), p


# ---- seams: lengths and lags taken from the kernel's geometry -----------------------------------------------------------------
def _with_splits(splits, f):
    if splits:
        os.environ["HPFW_LOCALJOIN_SPLITS"] = splits
    try:
        return f()
    finally:
        os.environ.pop("HPFW_LOCALJOIN_SPLITS", None)


def test_geometry_seams(lj, kernel):
    """every a is a copy of b at its lag (random where it overhangs b), so the pair's run is the whole overlap at that lag.  The
    chunks of a pair begin at min_len - (the longest a of the row group) + chunk i, min_len = ceil(min_score / T): 1 and 8
    here; a is staged in slices of `slice` positions"""
    sl, ch = _lib.localjoin_geometry()
    T, lens = 22, (1, 8)
    for n_b in (ch + sl + 7, 3 * ch + 5):
        b = _rand(n_b, 300 + n_b)
        for n_a in (sl - 1, sl, sl + 1, 2 * sl + 3):
            seams = sorted({ml - n_a + ch * i + e for ml in lens for i in range(1, (n_b - 2 * ml + n_a) // ch + 1) for e in (-1, 0)})
            lags = seams + [sl - 1, sl, 2 * sl - 1, 2 * sl, ch - sl - 1, ch - sl]          # b's window of a slice moves by sl
            lags += [1 - n_a, 8 - n_a, -1, 0, n_b - n_a, n_b - n_a + 1, n_b - 8, n_b - 1]
            # a run that begins in a slice which lies before b for the chunk's first lags and on b for this one
            lags += [-(sl + 8)] if n_a > sl + 8 else []
            lags = list(dict.fromkeys(lags))
            assert len(lags) < 32                                                            # one row group: its longest a is n_a
            clips = []
            for i, d in enumerate(lags):
                a = _rand(n_a, 400 + i)
                j0, j1 = max(0, -d), min(n_a, n_b - d)
                a[j0:j1] = b[d + j0:d + j1]
                clips.append(a)
            db = _index(lj, clips + [b])
            for ml in lens:
                for splits in (None, "1", "3"):
                    got = _with_splits(splits, lambda: _check(lj, db, T, ml * T, ("seams", n_b, n_a)))
                    vs_b = got[got["b"] == len(lags)]
                    want = [(i, d, max(0, -d), min(n_a, n_b - d) - max(0, -d)) for i, d in enumerate(lags)]
                    want = [w for w in want if w[3] >= ml]
                    assert [(int(p["a"]), int(p["lag"]), int(p["a_start"]), int(p["length"])) for p in vs_b] == want, (n_b, n_a, ml, splits)
                    assert (vs_b["dist"] == 0).all() and (vs_b["score"] == T * vs_b["length"].astype(np.int64)).all()


def test_runs_on_and_off_the_slices(lj, kernel):
    """runs of a that start and end on, one before and one after multiples of the slice; a run over several slices with one
    bad hashprint in it, which the rule bridges where what lies before it outweighs it and not where it does not"""
    sl, ch = _lib.localjoin_geometry()
    T, n_a = 22, 4 * sl + 3
    n_b = ch + sl + 7
    b = _rand(n_b, 700)
    ones = np.uint64(0xFFFFFFFFFFFFFFFF)
    clips, want = [], []

    def plant(d, j0, j1, seed):
        a = _rand(n_a, seed)
        a[j0:j1] = b[d + j0:d + j1]
        a[j0 - 1], a[j1] = ~b[d + j0 - 1], ~b[d + j1]      # (no chance hashprint at the run's ends: x = T - 64 there)
        return a

    for d in (100, 10 - n_a + ch - 1, 10 - n_a + ch):     # inside a chunk; the last lag of chunk 0 and the first of chunk 1 at min_len 10
        for j0 in (sl - 1, sl, sl + 1):
            for j1 in (3 * sl - 1, 3 * sl, 3 * sl + 1):
                clips.append(plant(d, j0, j1, 800 + len(clips)))
                want.append((d, j0, j1 - j0, 0))
    # a bad hashprint (64 bits: x = T - 64 = -42) after 40 good ones is bridged (40 T > 42), after one it is not (T < 42);
    # one with 2 T mismatching bits after one good hashprint brings the prefix back to 0: the earlier start wins
    a = plant(200, 2, n_a - 1, 900)
    a[42] ^= ones
    clips.append(a)
    want.append((200, 2, n_a - 3, 64))
    a = plant(200, 2, n_a - 1, 901)
    a[3] ^= ones
    clips.append(a)
    want.append((200, 4, n_a - 5, 0))
    a = plant(200, 2, n_a - 1, 902)
    a[3] ^= np.uint64((1 << 2 * T) - 1)
    clips.append(a)
    want.append((200, 2, n_a - 3, 2 * T))
    assert len(clips) < 32
    db = _index(lj, clips + [b])
    for splits in (None, "1"):
        got = _with_splits(splits, lambda: _check(lj, db, T, 10 * T, "slices"))
        vs_b = got[got["b"] == len(clips)]
        assert [tuple(int(p[f]) for f in ("lag", "a_start", "length", "dist")) for p in vs_b] == want


# ---- long recordings ------------------------------------------------------------------------------------------------------------
def test_one_long_pair(lj, kernel):
    """17 000 against 20 000 hashprints, above the local search's limit, with a shared passage of 5 000 at lag -500"""
    a, b = _rand(17000, 500), _rand(20000, 501)
    a[3000:8000] = b[2500:7500]
    db = _index(lj, [a, b])
    got = _check(lj, db, 22, 1000, "long")
    assert got.size == 1 and int(got[0]["lag"]) == -500 and int(got[0]["a_start"]) <= 3000 and int(got[0]["length"]) >= 5000
    assert int(got[0]["score"]) >= 22 * 5000 and _check(lj, db, 22, 22 * 5000 + 200, "long").size == 0


def test_longest_recordings(lj):
    """two equal recordings of 2^18 - 1 hashprints at T = 31 on the matrix cores: 2 * 31 * (2^18 - 1), the largest value the
    f32 accumulators ever hold.  One hashprint more is refused"""
    n = ref.MAX_LEN
    r = _rand(n, 600)
    _index(lj, [r, r])
    got = lj.index_localjoin(31, 1)
    assert [tuple(int(v) for v in p) for p in got] == [(0, 1, 31 * n, 0, 0, n, 0, 0)]
    with pytest.raises(hpfw_amd.HpfwError) as e:
        _index(lj, [np.zeros(n + 1, np.uint64), _rand(10, 603)])
        lj.index_localjoin(31, 1)
    assert e.value.status == _lib.E_UNSUPPORTED
    lj.index_clear()


# ---- degenerate inputs and call forms -----------------------------------------------------------------------------------------
def test_degenerate_inputs(lj, kernel):
    # all-zero clips: every overlap is a run of x = T; the longest overlap, then the smallest lag
    db = _index(lj, [np.zeros(10, np.uint64), np.zeros(3, np.uint64), np.zeros(7, np.uint64)])
    got = _check(lj, db, 5, 1, "zeros")
    assert [tuple(int(v) for v in p) for p in got] == [(0, 1, 15, -7, 7, 3, 0, 0), (0, 2, 35, -3, 3, 7, 0, 0), (1, 2, 15, 0, 0, 3, 0, 0)]
    assert _pairs(_check(lj, db, 5, 16, "zeros")) == [(0, 2)]
    # two equal clips and a reversed one
    r = np.arange(1, 41, dtype=np.uint64) * np.uint64(0x0123456789ABCDEF)
    db = _index(lj, [r, r[::-1].copy(), r])
    got = _check(lj, db, 16, 100, "equal")
    assert [tuple(int(v) for v in p) for p in got] == [(0, 2, 640, 0, 0, 40, 0, 0)]
    # all-ones against all-zeros at T = 31: nothing is positive
    db = _index(lj, [np.zeros(50, np.uint64), np.full(70, 0xFFFFFFFFFFFFFFFF, np.uint64)])
    assert _check(lj, db, 31, 1, "ones").size == 0
    # an empty index, a single clip, empty clips beside one
    lj.index_clear()
    assert lj.index_localjoin(22, 1).size == 0
    _index(lj, [_rand(100, 600)])
    assert lj.index_localjoin(22, 1).size == 0
    r = _rand(100, 600)
    db = _index(lj, [r, _rand(0, 601), r[40:45].copy(), _rand(0, 602)])
    assert [tuple(int(v) for v in p) for p in _check(lj, db, 22, 1, "empties")] == [(0, 2, 110, -40, 40, 5, 0, 0)]
    assert lj.index_localjoin(22, 111).size == 0          # ceil(111 / 22) = 6 hashprints: one clip reaches that


def test_cap_and_device_pointers(lj, kernel, torch_cuda):
    torch = torch_cuda
    clips = _ragged_clips()
    db = _index(lj, clips)
    want = ref.localjoin(db[0], db[1], 31, 1, cache=_REF.setdefault("ragged", {}))
    assert want.size > 100
    L = hpfw_amd.lib()
    for cap in (0, 1, 37, want.size, want.size + 5):
        out = np.zeros(max(cap, 1), _lib.PASSAGE_PAIR_DTYPE)
        count = ctypes.c_int64(-1)
        _lib.check(L.hpfw_gpu_index_localjoin(lj._h, 31, 1, _lib._hp(out) if cap else None, cap, ctypes.byref(count)))
        assert count.value == want.size
        _same(out[:min(cap, want.size)], want[:cap], ("cap", cap))
    _same(lj.index_localjoin(31, 1, cap=7), want, "growing and repeating")
    # device pointers on a side stream
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_out = torch.zeros(50 * 32, dtype=torch.uint8, device="cuda")
        d_count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        lj.index_localjoin_dev(31, 1, d_out.data_ptr(), 50, d_count.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    assert int(d_count.cpu()[0]) == want.size and d_out.cpu().numpy().tobytes() == want[:50].tobytes()


def test_clip_base_and_index_remove(lj, kernel):
    clips = _ragged_clips()
    db = _index(lj, clips, base=1000)
    try:
        got = _check(lj, db, 22, MIDDLE[22][1], "ragged", base=1000)
        assert _pairs(got) == [(1000 + a, 1000 + b) for a, b in sorted(PLANTED)]
        lj.index_remove([16, 19])                         # one clip of the exact copy, one of the three that share a passage
        emptied = [c if i not in (16, 19) else c[:0] for i, c in enumerate(clips)]
        db = _lib._ragged(emptied, np.uint64)
        got = _check(lj, db, 22, MIDDLE[22][1], "removed", base=1000)
        assert _pairs(got) == [(1000 + a, 1000 + b) for a, b in sorted(PLANTED) if not {a, b} & {16, 19}]
        _check(lj, db, 22, 1, "removed", base=1000)
    finally:
        lj.index_set_clip_base(0)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def _noisy(x, seed):
    """gain 0.5 and white noise at 10 dB SNR, as synth.gen_query makes its queries"""
    seg = 0.5 * x.astype(np.float64)
    rng = np.random.default_rng([0x6E6F6973, seed])
    p = float(np.mean(seg ** 2)) + 1e-12
    seg = seg + np.sqrt(p / 10 ** (10.0 / 10)) * rng.standard_normal(seg.size)
    return np.clip(np.round(seg), -32768, 32767).astype(np.int16)


COLS_PER_S, T_E2E = 80.6, 22


def test_shared_passages_end_to_end(tmp_path, filters, oracle, torch_cuda, kernel):
    """six songs of 10 s and an item of 10 s: two seconds of its own material, seconds 3 to 7 of song 4 at gain 0.5 and 10 dB
    SNR, four seconds of its own.  duplicates() does not see the pair; shared_passages() reports it alone, with its ends.
    min_score is the geometric mean of the true pair's score and the largest other score by the restatement"""
    sr, T = synth.SR, T_E2E
    songs = np.stack([synth.gen_clip(i, 10.0) for i in range(6)])
    own = synth.gen_clip(50, 10.0)
    item = np.concatenate([own[:2 * sr], _noisy(songs[4][3 * sr:7 * sr], 11), own[6 * sr:]])
    names = ["item"] + [f"song{i:02d}" for i in range(6)]
    cache = str(tmp_path / "cache") + "/"                # the collector reads the filter fixture as it reads learned filters
    os.makedirs(cache)
    with open(os.path.join(cache, "filters.cereal"), "wb") as f:
        f.write(np.array([64, 2420], np.int32).tobytes() + np.ascontiguousarray(filters, np.float32).tobytes())
    lsi = hpfw_amd.LiveSongIdentification(cache=cache)
    try:
        ext = lsi.collector.gpu()
        pcm = np.concatenate([item[None], songs])
        hp = list(ext.extract(pcm))
        lsi.build(list(zip(hp, names)))
        mode = oracle.get_projection()
        oracle.set_projection(ext.get_projection())
        try:
            if "e2e" not in _REF:                         # the CPU oracle's hashprints are the device's
                plan = oracle.Plan(10 * sr)
                db_hp, db_off = _lib._ragged(list(plan.extract_batch(filters, pcm, 16)), np.uint64)
                _REF["e2e"] = (db_hp, db_off, ref.candidates(db_hp, db_off, T), plan.c - plan.n_hp)
        finally:
            oracle.set_projection(mode)
        db_hp, db_off, cand, reach = _REF["e2e"]
        assert all(np.array_equal(h, db_hp[db_off[i]:db_off[i + 1]]) for i, h in enumerate(hp))
        true = (0, 5)                                     # (item, song04)
        other = max(v[0] for p, v in cand.items() if p != true)
        print(f"true pair {cand[true]}, largest other score {other}")
        assert cand[true][0] >= 4 * other
        min_score = int(round((cand[true][0] * other) ** 0.5))
        # the overlap rule rates everything the two have in common at the lag: the foreign material hides the pair
        assert ("item", "song04") not in [(a, b) for a, b, *_ in lsi.duplicates(19.38, 100)]
        got = lsi.shared_passages(T, min_score)
        want = ref.localjoin(db_hp, db_off, T, min_score)
        assert [(names.index(a), names.index(b)) + tuple(rest) for a, b, *rest in got] == [tuple(int(v) for v in p)[:7] for p in want]
        assert [(a, b) for a, b, *_ in got] == [("item", "song04")]
        _, _, score, lag, a_start, length, dist = got[0]
        # item second 2 is song second 3; a hashprint reads `reach` columns beyond its own: 4 s less that much are clean
        assert abs(lag - round(1.0 * COLS_PER_S)) <= 1 and score == T * length - dist
        assert abs(a_start - round(2.0 * COLS_PER_S)) <= 45 and abs(a_start + length - (round(6.0 * COLS_PER_S) - reach)) <= 45
        # a sharded identifier has no local self-join
        sharded = hpfw_amd.LiveSongIdentification.__new__(hpfw_amd.LiveSongIdentification)
        sharded._gpu = object.__new__(hpfw_amd.liveid._ShardedIndex)
        with pytest.raises(hpfw_amd.HpfwError) as e:
            sharded.shared_passages(T, min_score)
        assert e.value.status == _lib.E_UNSUPPORTED
    finally:
        lsi._gpu.close()
