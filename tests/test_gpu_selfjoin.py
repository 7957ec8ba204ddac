"""The catalogue self-join on the GPU: every case runs under both kernel selections -- the fp4
matrix-core scan with its slice loop and the xor/popcount kernel -- and is compared with the restatement of
tests/selfjoin_ref.py field for field."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, synth

import overlap_ref
import selfjoin_ref as ref

pytestmark = pytest.mark.gpu
SEED = 20261020
_REF = {}                                                # candidates computed once per index, shared by both kernel selections


@pytest.fixture(params=["mfma", "popcount"])
def kernel(request):
    if request.param == "popcount":
        os.environ["HPFW_SELFJOIN_POPC"] = "1"
    yield request.param
    os.environ.pop("HPFW_SELFJOIN_POPC", None)


@pytest.fixture(scope="module")
def sj(torch_cuda):
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


def _check(g, db, mo, num, den, key, base=0):
    """index_selfjoin equals the restatement (the candidates of an index are computed once per key and min_overlap)"""
    want = ref.selfjoin(db[0], db[1], mo, num, den, clip_base=base, cache=_REF.setdefault(key, {}))
    got = g.index_selfjoin(mo, num, den)
    _same(got, want, (key, mo, num, den))
    return got


# ---- the ragged index: 40 clips, two row groups (the triangle cuts inside the first, the second is partial) ----------------
LENGTHS = [0, 3, 7, 8, 9, 31, 32, 33, 64, 100, 143, 200, 255, 256, 257, 304]


def _ragged_clips():
    rng = np.random.default_rng([SEED, 1])
    lengths = LENGTHS + [int(v) for v in rng.integers(8, 600, 24)]
    lengths[18], lengths[19], lengths[20], lengths[21] = 100, 500, 333, 410
    clips = [_rand(n, 100 + i) for i, n in enumerate(lengths)]
    clips[16] = clips[11].copy()                          # an exact copy (200)
    clips[17] = _flip(clips[15], 0.1, 1)                  # a copy with a tenth of the bits flipped (304)
    clips[19][150:250] = clips[18]                        # a short clip wholly inside a long one
    clips[21][:80] = clips[20][-80:]                      # the tail of one as the head of another
    assert len(clips) == 40 and all(8 <= c.size <= 599 for c in clips[16:])
    return clips


PLANTED = {(11, 16): (0, 200, 0), (15, 17): (None, 304, 0), (18, 19): (0, 100, 150), (20, 21): (0, 80, 80 - 333)}


def test_ragged_index(sj, kernel):
    clips = _ragged_clips()
    db = _index(sj, clips)
    for mo in (8, 64):
        cand = ref.candidates(db[0], db[1], mo, cache=_REF.setdefault("ragged", {}))
        rates = sorted((Fraction(d, L), pair) for pair, (d, L, _) in cand.items())
        print(f"min_overlap {mo}: planted rates", [(p, float(r)) for r, p in rates[:4]], "smallest other rate", float(rates[4][0]))
        want = ref.selfjoin(db[0], db[1], mo, 16, 1, cache=_REF["ragged"])
        # the restatement reports exactly the planted pairs (random pairs lie far above 16, the noisy copy near 6.4)
        assert [(int(p["a"]), int(p["b"])) for p in want] == sorted(PLANTED)
        for p in want:
            dist, L, lag = PLANTED[(int(p["a"]), int(p["b"]))]
            assert (int(p["overlap"]), int(p["lag"])) == (L, lag) and (dist is None or int(p["dist"]) == dist), p
        assert 5 * 304 < int(want[1]["dist"]) < 8 * 304
        _check(sj, db, mo, 16, 1, "ragged")
        # threshold 64: every pair whose two clips reach min_overlap
        m = sum(c.size >= mo for c in clips)
        got = _check(sj, db, mo, 64, 1, "ragged")
        assert got.size == m * (m - 1) // 2
        assert not np.isin(got["a"], [i for i, c in enumerate(clips) if c.size < mo]).any()
        assert (got["a"] < got["b"]).all() and (got["pad"] == 0).all()
        os.environ["HPFW_SELFJOIN_TABLE_KB"] = "24"       # one row group of 40 clips is 20 KiB: a pass per group
        try:
            _check(sj, db, mo, 16, 1, "ragged")
            _check(sj, db, mo, 64, 1, "ragged")
            _same(sj.index_selfjoin(mo, 64, 1, cap=got.size - 50), got, "two passes, growing and repeating")
        finally:
            os.environ.pop("HPFW_SELFJOIN_TABLE_KB", None)


def test_cross_check_against_search_overlap(sj, kernel):
    """the same pairs by the overlap search all-against-all with exclude (which computes both orders of every pair)"""
    clips = _ragged_clips()
    db = _index(sj, clips)
    me = np.arange(len(clips), dtype=np.int32)
    for mo in (8, 64):
        pairs = sj.index_selfjoin(mo, 64, 1)
        hits = sj.search_overlap(db[0], db[1], 64, mo, exclude=me)
        by_pair = {(a, int(h["clip"])): (int(h["dist"]), int(h["overlap"]), int(h["lag"]))
                   for a, row in enumerate(hits) for h in row if h["clip"] != 0xFFFFFFFF}
        m = sum(c.size >= mo for c in clips)
        assert pairs.size == m * (m - 1) // 2 and m > 20
        for p in pairs:
            assert by_pair[(int(p["a"]), int(p["b"]))] == (int(p["dist"]), int(p["overlap"]), int(p["lag"])), p


# ---- seams: lengths and lags taken from the kernel's geometry -----------------------------------------------------------------
def test_geometry_seams(sj, kernel):
    """every a is a copy of b at its lag (random where it overhangs b), so that lag has rate 0.  The chunks of a pair begin at
    min_overlap - (the longest a of the row group) + chunk i; a is staged in slices of `slice` positions"""
    sl, ch = _lib.selfjoin_geometry()
    mo = 8
    for n_b in (ch + sl + 7, 3 * ch + 5):
        b = _rand(n_b, 300 + n_b)
        for n_a in (sl - 1, sl, sl + 1, 2 * sl + 3):
            d_lo = mo - n_a
            seams = [d_lo + ch * i + e for i in range(1, (n_b - mo - d_lo) // ch + 1) for e in (-1, 0)]
            lags = seams + [sl - 1, sl, 2 * sl - 1, 2 * sl, ch - sl - 1, ch - sl]          # b's window of a slice moves by sl
            lags += [mo - n_a, -1, 0, n_b - n_a, n_b - n_a + 1, n_b - mo]
            assert len(lags) < 32                                                            # one row group: its longest a is n_a
            clips = []
            for i, d in enumerate(lags):
                a = _rand(n_a, 400 + i)
                j0, j1 = max(0, -d), min(n_a, n_b - d)
                a[j0:j1] = b[d + j0:d + j1]
                clips.append(a)
            db = _index(sj, clips + [b])
            for splits in (None, "1", "3"):
                if splits:
                    os.environ["HPFW_SELFJOIN_SPLITS"] = splits
                try:
                    got = _check(sj, db, mo, 64, 1, ("seams", n_b, n_a))
                finally:
                    os.environ.pop("HPFW_SELFJOIN_SPLITS", None)
                vs_b = got[got["b"] == len(lags)]
                assert [int(v) for v in vs_b["lag"]] == lags and (vs_b["dist"] == 0).all(), (n_b, n_a, splits)
                assert [int(v) for v in vs_b["overlap"]] == [overlap_ref.overlap(n_a, n_b, d) for d in lags]


def test_one_long_pair(sj, kernel):
    """17 000 against 20 000 hashprints: above the overlap search's limit, and an overlap above its 14-bit field"""
    a, b = _rand(17000, 500), _rand(20000, 501)
    a[3000:] = b[2500:16500]
    db = _index(sj, [a, b])
    got = _check(sj, db, 304, 8, 1, "long")
    assert got.size == 1 and (int(got[0]["lag"]), int(got[0]["overlap"])) == (-500, 16500)
    assert _check(sj, db, 304, 4, 1, "long").size == 0    # (2500 random positions of 16500: 4.85 bits a hashprint)


def test_tied_candidates(sj, kernel):
    # all-zero clips: rate 0 at every lag, so the largest overlap wins, then the smallest lag
    db = _index(sj, [np.zeros(10, np.uint64), np.zeros(3, np.uint64), np.zeros(7, np.uint64)])
    got = _check(sj, db, 2, 0, 1, "zeros")
    assert [tuple(int(v) for v in p) for p in got] == [(0, 1, 0, 3, -7, 0), (0, 2, 0, 7, -3, 0), (1, 2, 0, 3, 0, 0)]
    # two equal clips
    r = np.arange(1, 41, dtype=np.uint64) * np.uint64(0x0123456789ABCDEF)
    db = _index(sj, [r, r[::-1].copy(), r])
    got = _check(sj, db, 4, 0, 1, "equal")
    assert [tuple(int(v) for v in p) for p in got] == [(0, 2, 0, 40, 0, 0)]
    # 32 / 64 against 64 / 128 (the same rate in other terms), then 31 / 64 (section 17's pairs)
    q = np.zeros(128, np.uint64)
    half = np.zeros(64, np.uint64)
    half[::2] = 1
    full = np.zeros(128, np.uint64)
    full[32:96] = 1
    for tag, first in (("32/64", 32), ("31/64", 31)):
        if first == 31:
            half[0] = 0
        db = _index(sj, [q, half, full])
        got = _check(sj, db, 64, 64, 1, tag)
        assert [(int(p["dist"]), int(p["overlap"])) for p in got[:2]] == [(first, 64), (64, 128)]
        # the threshold's edge: dist rate_den == rate_num overlap is reported, one bit more is not
        _check(sj, db, 64, 1, 2, tag)
        exact = sj.index_selfjoin(64, first, 64)
        assert (0, 1) in [(int(p["a"]), int(p["b"])) for p in exact]
        assert (0, 1) not in [(int(p["a"]), int(p["b"])) for p in sj.index_selfjoin(64, first - 1, 64)]


def test_cap_below_the_count(sj, kernel, torch_cuda):
    torch = torch_cuda
    clips = _ragged_clips()
    db = _index(sj, clips)
    want = ref.selfjoin(db[0], db[1], 64, 64, 1, cache=_REF.setdefault("ragged", {}))
    assert want.size > 100
    L = hpfw_amd.lib()
    for cap in (0, 1, 37, want.size, want.size + 5):
        out = np.zeros(max(cap, 1), _lib.DUP_PAIR_DTYPE)
        count = ctypes.c_int64(-1)
        _lib.check(L.hpfw_gpu_index_selfjoin(sj._h, 64, 64, 1, _lib._hp(out) if cap else None, cap, ctypes.byref(count)))
        assert count.value == want.size
        _same(out[:min(cap, want.size)], want[:cap], ("cap", cap))
    _same(sj.index_selfjoin(64, 64, 1, cap=7), want, "growing and repeating")
    # device pointers on a side stream
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_out = torch.zeros(50 * 24, dtype=torch.uint8, device="cuda")
        d_count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        sj.index_selfjoin_dev(64, 64, 1, d_out.data_ptr(), 50, d_count.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    assert int(d_count.cpu()[0]) == want.size and d_out.cpu().numpy().tobytes() == want[:50].tobytes()


def test_after_index_remove(sj, kernel):
    clips = _ragged_clips()
    _index(sj, clips, base=1000)
    try:
        sj.index_remove([16, 19])                         # one clip of the exact copy, the long clip that holds the short one
        emptied = [c if i not in (16, 19) else c[:0] for i, c in enumerate(clips)]
        db_hp, db_off = _lib._ragged(emptied, np.uint64)
        got = _check(sj, (db_hp, db_off), 8, 16, 1, "removed", base=1000)
        assert [(int(p["a"]), int(p["b"])) for p in got] == [(1015, 1017), (1020, 1021)]
        _check(sj, (db_hp, db_off), 8, 64, 1, "removed", base=1000)
    finally:
        sj.index_set_clip_base(0)


def test_empty_index_and_one_clip(sj, kernel):
    sj.index_clear()
    assert sj.index_selfjoin(1, 64, 1).size == 0
    _index(sj, [_rand(100, 600)])
    assert sj.index_selfjoin(1, 64, 1).size == 0
    _index(sj, [_rand(100, 600), _rand(0, 601), _rand(5, 602)])
    assert sj.index_selfjoin(6, 64, 1).size == 0          # one clip reaches min_overlap
    got = sj.index_selfjoin(5, 64, 1)
    assert got.size == 1 and (int(got[0]["a"]), int(got[0]["b"]), int(got[0]["overlap"])) == (0, 2, 5)
    with pytest.raises(hpfw_amd.HpfwError) as e:          # a recording above 2^18 - 1 hashprints
        _index(sj, [np.zeros(2 ** 18, np.uint64), _rand(10, 603)])
        sj.index_selfjoin(5, 64, 1)
    assert e.value.status == _lib.E_UNSUPPORTED
    sj.index_clear()


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def _noisy(x, seed):
    """gain 0.5 and white noise at 10 dB SNR, as synth.gen_query makes its queries"""
    seg = 0.5 * x.astype(np.float64)
    rng = np.random.default_rng([0x6E6F6973, seed])
    p = float(np.mean(seg ** 2)) + 1e-12
    seg = seg + np.sqrt(p / 10 ** (10.0 / 10)) * rng.standard_normal(seg.size)
    return np.clip(np.round(seg), -32768, 32767).astype(np.int16)


def test_duplicates_end_to_end(tmp_path, filters, oracle, torch_cuda, kernel):
    """an item that is seconds 2 to 5 of song 4, a noisy copy of song 2 (gain 0.5, 10 dB SNR), and six songs of 10 s.  The
    threshold is the geometric mean of the largest true-pair rate and the smallest other rate by the restatement"""
    sr = synth.SR
    songs = np.stack([synth.gen_clip(i, 10.0) for i in range(6)])
    copy = _noisy(songs[2], 7)
    item = np.ascontiguousarray(songs[4][2 * sr:5 * sr])
    names = ["item", "copy"] + [f"song{i:02d}" for i in range(6)]
    cache = str(tmp_path / "cache") + "/"                # the collector reads the filter fixture as it reads learned filters
    os.makedirs(cache)
    with open(os.path.join(cache, "filters.cereal"), "wb") as f:
        f.write(np.array([64, 2420], np.int32).tobytes() + np.ascontiguousarray(filters, np.float32).tobytes())
    lsi = hpfw_amd.LiveSongIdentification(cache=cache)
    try:
        ext = lsi.collector.gpu()
        hp = [ext.extract(item[None])[0]] + list(ext.extract(np.concatenate([copy[None], songs])))
        lsi.build(list(zip(hp, names)))
        mode = oracle.get_projection()
        oracle.set_projection(ext.get_projection())
        try:
            if "e2e" not in _REF:                         # the CPU oracle's hashprints are the device's
                idx = [oracle.Plan(3 * sr).extract(filters, item)] + list(oracle.Plan(10 * sr).extract_batch(
                    filters, np.concatenate([copy[None], songs]), 16))
                db_hp, db_off = _lib._ragged(idx, np.uint64)
                _REF["e2e"] = (db_hp, db_off, ref.candidates(db_hp, db_off, 100))
        finally:
            oracle.set_projection(mode)
        db_hp, db_off, cand = _REF["e2e"]
        assert all(np.array_equal(h, db_hp[db_off[i]:db_off[i + 1]]) for i, h in enumerate(hp))
        true = {(0, 6), (1, 4)}                           # (item, song04), (copy, song02)
        worst_true = max(Fraction(d, L) for p, (d, L, _) in cand.items() if p in true)
        best_other = min(Fraction(d, L) for p, (d, L, _) in cand.items() if p not in true)
        threshold = (float(worst_true) * float(best_other)) ** 0.5
        print(f"largest true-pair rate {float(worst_true):.2f}, smallest other rate {float(best_other):.2f}, threshold {threshold:.2f}")
        got = lsi.duplicates(threshold, 100)
        num, den = hpfw_amd.liveid.rate_fraction(threshold)
        want = ref.selfjoin(db_hp, db_off, 100, num, den)
        assert [(names.index(a), names.index(b), d, L, lag) for a, b, d, L, lag in got] == \
               [tuple(int(v) for v in p)[:5] for p in want]
        assert [(a, b) for a, b, *_ in got] == [("item", "song04"), ("copy", "song02")]
        assert abs(got[0][4] - 161) <= 1 and abs(got[1][4]) <= 1, got
        assert lsi.duplicate_groups(got) == [["item", "song04"], ["copy", "song02"]]
        # a sharded identifier has no self-join
        sharded = hpfw_amd.LiveSongIdentification.__new__(hpfw_amd.LiveSongIdentification)
        sharded._gpu = object.__new__(hpfw_amd.liveid._ShardedIndex)
        with pytest.raises(hpfw_amd.HpfwError) as e:
            sharded.duplicates(16, 100)
        assert e.value.status == _lib.E_UNSUPPORTED
    finally:
        lsi._gpu.close()
