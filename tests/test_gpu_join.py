"""The ingest check on the GPU: recordings that are not in the index joined against it.  Every case
runs under both kernel selections -- the fp4 matrix-core scan and the xor/popcount kernel -- and is compared field for field
with the restatement of tests/join_ref.py; where it says so also with the device's second opinion: a second handle with the
batch added to the index, its self-join, and of that the pairs whose b is of the batch."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, synth

import join_ref as ref
import overlap_ref
import selfjoin_ref

pytestmark = pytest.mark.gpu
SEED = 2024
_REF = {}                                                # candidates computed once per (index, batch), shared by both kernel selections


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


@pytest.fixture(scope="module")
def twin(torch_cuda):
    """the handle of the second opinion"""
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
    if clips:
        g.index_add(db_hp, db_off)
    return db_hp, db_off


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: first difference at {bad}: got {got[bad]}, want {want[bad]}")


def _want(db, x, mo, num, den, among, key, base=0):
    return ref.join(db[0], db[1], x[0], x[1], mo, num, den, among, clip_base=base, cache=_REF.setdefault(key, {}))


def _check(g, db, x, mo, num, den, among, key, base=0):
    """index_join equals the restatement (the candidates of an index with its batch are computed once per key and min_overlap)"""
    want = _want(db, x, mo, num, den, among, key, base)
    got = g.index_join(x[0], x[1], mo, num, den, among)
    _same(got, want, (key, mo, num, den, among))
    return got


def _second_opinion(g, clips, batch, mo, num, den, among, base=0):
    """on another handle: index_add of the batch, index_selfjoin, the pairs with b of the batch (and a indexed unless among)"""
    _index(g, list(clips) + list(batch), base)
    full = g.index_selfjoin(mo, num, den)
    keep = full["b"] >= base + len(clips)
    if not among:
        keep &= full["a"] < base + len(clips)
    return full[keep]


# ---- 1. a ragged index of 40 clips against a batch of 10 ---------------------------------------------------------------------
def _ragged_case():
    rng = np.random.default_rng([SEED, 1])
    lengths = [0, 5, 599, 64] + [int(v) for v in rng.integers(8, 599, 36)]
    lengths[10], lengths[11], lengths[12] = 304, 333, 410
    clips = [_rand(n, 100 + i) for i, n in enumerate(lengths)]
    assert len(clips) == 40 and max(lengths) == 599 and lengths.count(599) == 1
    fresh = _rand(250, 150)
    batch = [clips[2].copy(),                                                     # 40: an exact copy of the longest clip
             _flip(clips[10], 0.1, 1),                                            # 41: a copy with a tenth of the bits flipped
             clips[2][100:260].copy(),                                            # 42: inside clip 2 -- and inside 40
             np.concatenate([_rand(150, 151), clips[3], _rand(200, 152)]),        # 43: the 64-hashprint clip between random ones
             np.concatenate([clips[11][-120:], _rand(300, 153)]),                 # 44: the tail of clip 11, then random
             fresh,                                                               # 45: a random recording
             _flip(fresh, 0.05, 2),                                               # 46: the same with a twentieth of the bits flipped
             _rand(5, 154),                                                       # 47
             _rand(0, 155),                                                       # 48: empty
             np.concatenate([_rand(40, 156), clips[12][:100]])]                   # 49: random, then the head of clip 12
    planted = {(2, 40): (0, 599, 0), (10, 41): (None, 304, 0), (2, 42): (0, 160, -100), (40, 42): (0, 160, -100),
               (3, 43): (0, 64, 150), (11, 44): (0, 120, 120 - 333), (45, 46): (None, 250, 0), (12, 49): (0, 100, 40)}
    return clips, batch, planted


def test_ragged_index(sj, twin, kernel):
    clips, batch, planted = _ragged_case()
    db, x = _index(sj, clips), _lib._ragged(batch, np.uint64)
    n = len(clips)
    for mo in (8, 64):
        cand = selfjoin_ref.candidates(*ref.appended(*db, *x), mo, cache=_REF.setdefault("ragged", {}))
        rates = sorted((Fraction(d, L), pair) for pair, (d, L, _) in cand.items() if pair[1] >= n)
        print(f"min_overlap {mo}: planted rates", [(p, round(float(r), 2)) for r, p in rates[:len(planted)]],
              "smallest other rate", round(float(rates[len(planted)][0]), 2))
        for among in (0, 1):
            expect = sorted(p for p in planted if among or p[0] < n)
            # the restatement reports exactly the planted pairs at 16 (random pairs lie far above, the noisy copies at 6.4 and 3.2)
            want = _want(db, x, mo, 16, 1, among, "ragged")
            assert [(int(p["a"]), int(p["b"])) for p in want] == expect
            for p in want:
                dist, L, lag = planted[(int(p["a"]), int(p["b"]))]
                assert (int(p["overlap"]), int(p["lag"])) == (L, lag) and (dist is None or int(p["dist"]) == dist), p
            # threshold 64: every pair whose two recordings reach min_overlap
            rows = sum(c.size >= mo for c in clips)
            cols = [j for j, c in enumerate(batch) if c.size >= mo]
            eligible = rows * len(cols) + (len(cols) * (len(cols) - 1) // 2 if among else 0)
            for splits in (None, "1", "3"):
                for table_kb in (None, "15" if splits == "3" else "5"):  # a row group of 10 externals is 5 KiB a split: a pass per group
                    if splits:
                        os.environ["HPFW_SELFJOIN_SPLITS"] = splits
                    if table_kb:
                        os.environ["HPFW_SELFJOIN_TABLE_KB"] = table_kb
                    try:
                        _check(sj, db, x, mo, 16, 1, among, "ragged")
                        got = _check(sj, db, x, mo, 64, 1, among, "ragged")
                    finally:
                        os.environ.pop("HPFW_SELFJOIN_SPLITS", None)
                        os.environ.pop("HPFW_SELFJOIN_TABLE_KB", None)
                    assert got.size == eligible and (got["a"] < got["b"]).all() and (got["pad"] == 0).all() and (got["b"] >= n).all()
                    short = [i for i, c in enumerate(clips + batch) if c.size < mo]
                    assert not np.isin(got["a"], short).any() and not np.isin(got["b"], short).any()
            _same(_second_opinion(twin, clips, batch, mo, 64, 1, among), got, ("second opinion", mo, among))


# ---- 2. row groups that hold indexed and external rows together ----------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 30, 32, 33, 64])
def test_mixed_row_groups(sj, twin, kernel, n):
    lengths = np.random.default_rng([SEED, 2, n]).integers(20, 61, n)
    clips = [_rand(int(k), 1000 * n + i) for i, k in enumerate(lengths)]
    first = clips[0] if n else _rand(48, 700)
    loner = _rand(40, 701)
    batch = [first.copy(),                                                        # n: clip 0 again (n = 0: a new recording)
             _flip(first, 0.05, 3),                                               # n + 1: near n and clip 0
             (clips[-1] if n else first)[5:].copy(),                              # n + 2: the last clip without its head
             loner,                                                               # n + 3
             np.concatenate([_rand(9, 702), loner[:30]])]                         # n + 4: holds the head of n + 3
    db, x = _index(sj, clips), _lib._ragged(batch, np.uint64)
    key = ("mixed", n)
    for among in (0, 1):
        got = _check(sj, db, x, 8, 16, 1, among, key)
        pairs = [(int(p["a"]), int(p["b"])) for p in got]
        # the recordings that hold `first` pair with each other (n <= 1: n + 2 is one of them), n - 1 with n + 2, n + 3 with n + 4
        family = ([0] if n else []) + [n, n + 1] + ([n + 2] if n <= 1 else [])
        planted = {(a, b) for a in family for b in family if a < b} | {(n + 3, n + 4)} | ({(n - 1, n + 2)} if n > 1 else set())
        assert pairs == sorted((a, b) for a, b in planted if b >= n and (among or a < n)), (n, among, pairs)
        full = _check(sj, db, x, 8, 64, 1, among, key)
        assert full.size == n * 5 + (10 if among else 0)
        _same(_second_opinion(twin, clips, batch, 8, 64, 1, among), full, ("second opinion", n, among))


# ---- 3. seams: lengths and lags taken from the kernel's geometry ---------------------------------------------------------------
def test_geometry_seams(sj, kernel):
    """every a is a copy of b at its lag (random where it overhangs b), so that lag has rate 0.  The chunks of a pair begin at
    min_overlap - (the longest a of the row group) + chunk i; a is staged in slices of `slice` positions.  Once with every a
    indexed and b the batch, once with half of them indexed and the others in the batch before b: one row group of both"""
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
            for n_indexed in (len(clips), len(clips) // 2):
                db = _index(sj, clips[:n_indexed])
                x = _lib._ragged(clips[n_indexed:] + [b], np.uint64)
                for splits in (None, "1", "3"):
                    if splits:
                        os.environ["HPFW_SELFJOIN_SPLITS"] = splits
                    try:
                        got = _check(sj, db, x, mo, 64, 1, 1, ("seams", n_b, n_a))     # (the same list either way)
                    finally:
                        os.environ.pop("HPFW_SELFJOIN_SPLITS", None)
                    vs_b = got[got["b"] == len(lags)]
                    assert [int(v) for v in vs_b["lag"]] == lags and (vs_b["dist"] == 0).all(), (n_b, n_a, n_indexed, splits)
                    assert [int(v) for v in vs_b["overlap"]] == [overlap_ref.overlap(n_a, n_b, d) for d in lags]
                    assert [int(v) for v in vs_b["a"]] == list(range(len(lags)))


# ---- 4. other cases ----------------------------------------------------------------------------------------------------------------
def test_one_long_pair(sj, kernel):
    """17 000 indexed against an external recording of 20 000 hashprints: above the overlap search's limits"""
    a, b = _rand(17000, 500), _rand(20000, 501)
    a[3000:] = b[2500:16500]
    db, x = _index(sj, [a]), _lib._ragged([b], np.uint64)
    for among in (0, 1):
        got = _check(sj, db, x, 304, 8, 1, among, "long")
        assert got.size == 1 and tuple(int(v) for v in got[0])[:2] == (0, 1)
        assert (int(got[0]["lag"]), int(got[0]["overlap"])) == (-500, 16500)
    assert _check(sj, db, x, 304, 4, 1, 1, "long").size == 0   # (2500 random positions of 16500: 4.85 bits a hashprint)


def test_thresholds_on_the_edge(sj, kernel):
    # 32 / 64 against 64 / 128 (the same rate in other terms), then 31 / 64 (section 17's pairs)
    q = np.zeros(128, np.uint64)
    half = np.zeros(64, np.uint64)
    half[::2] = 1
    full = np.zeros(128, np.uint64)
    full[32:96] = 1
    for tag, first in (("32/64", 32), ("31/64", 31)):
        if first == 31:
            half[0] = 0
        db, x = _index(sj, [q]), _lib._ragged([half, full], np.uint64)
        got = _check(sj, db, x, 64, 64, 1, 0, tag)
        assert [(int(p["dist"]), int(p["overlap"])) for p in got] == [(first, 64), (64, 128)]
        _check(sj, db, x, 64, 64, 1, 1, tag)
        # the threshold's edge: dist rate_den == rate_num overlap is reported, one bit more is not
        _check(sj, db, x, 64, 1, 2, 1, tag)
        exact = sj.index_join(x[0], x[1], 64, first, 64, 0)
        assert (0, 1) in [(int(p["a"]), int(p["b"])) for p in exact]
        assert (0, 1) not in [(int(p["a"]), int(p["b"])) for p in sj.index_join(x[0], x[1], 64, first - 1, 64, 0)]


def test_cap_streams_and_an_untouched_index(sj, kernel, torch_cuda):
    torch = torch_cuda
    clips, batch, _ = _ragged_case()
    db, x = _index(sj, clips), _lib._ragged(batch, np.uint64)
    before, self_before = sj.index_get(), sj.index_selfjoin(64, 16, 1)
    want = _want(db, x, 64, 64, 1, 1, "ragged")
    assert want.size > 100
    L = hpfw_amd.lib()
    for cap in (0, 1, 37, want.size, want.size + 5):
        out = np.zeros(max(cap, 1), _lib.DUP_PAIR_DTYPE)
        count = ctypes.c_int64(-1)
        _lib.check(L.hpfw_gpu_index_join(sj._h, _lib._hp(x[0]), _lib._hp(x[1]), len(batch), 1, 64, 64, 1, _lib._hp(out) if cap else None,
                                         cap, ctypes.byref(count)))
        assert count.value == want.size
        _same(out[:min(cap, want.size)], want[:cap], ("cap", cap))
    first = sj.index_join(x[0], x[1], 64, 64, 1, 1, cap=7)
    _same(first, want, "growing and repeating")
    assert sj.index_join(x[0], x[1], 64, 64, 1, 1).tobytes() == first.tobytes()          # a repeated call: the same bytes
    # offsets that do not begin at 0
    shifted = (np.concatenate([_rand(11, 800), x[0]]), x[1] + 11)
    _same(sj.index_join(shifted[0], shifted[1], 64, 64, 1, 1), want, "offsets from 11 on")
    # device pointers on a side stream
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_x = torch.from_numpy(x[0].view(np.int64)).to("cuda", non_blocking=False)
        d_out = torch.zeros(50 * 24, dtype=torch.uint8, device="cuda")
        d_count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        sj.index_join_dev(d_x.data_ptr(), x[1], 64, 64, 1, 1, d_out.data_ptr(), 50, d_count.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    assert int(d_count.cpu()[0]) == want.size and d_out.cpu().numpy().tobytes() == want[:50].tobytes()
    # the index is as it was, and so is its self-join
    after = sj.index_get()
    assert before[0].tobytes() == after[0].tobytes() and np.array_equal(before[1], after[1]) and sj.index_size() == len(clips)
    assert sj.index_selfjoin(64, 16, 1).tobytes() == self_before.tobytes()


def test_after_index_remove_and_the_clip_base(sj, kernel):
    clips, batch, planted = _ragged_case()
    x = _lib._ragged(batch, np.uint64)
    db = _index(sj, clips, base=1000)
    try:
        got = _check(sj, db, x, 8, 16, 1, 1, "ragged", base=1000)                        # external ids are 1000 + n + i
        assert [(int(p["a"]), int(p["b"])) for p in got] == sorted((a + 1000, b + 1000) for a, b in planted)
        sj.index_remove([2, 11])                          # the longest clip (partner of 40 and 42) and the partner of 44
        emptied = [c if i not in (2, 11) else c[:0] for i, c in enumerate(clips)]
        db = _lib._ragged(emptied, np.uint64)
        got = _check(sj, db, x, 8, 16, 1, 1, "removed", base=1000)
        assert [(int(p["a"]), int(p["b"])) for p in got] == sorted((a + 1000, b + 1000) for a, b in planted if a not in (2, 11))
        full = _check(sj, db, x, 8, 64, 1, 1, "removed", base=1000)
        assert not np.isin(full["a"], [1002, 1011]).any()
    finally:
        sj.index_set_clip_base(0)


def test_empty_sides_and_refusals(sj, kernel):
    x = _lib._ragged([_rand(100, 600), _rand(0, 601), _rand(5, 602)], np.uint64)
    none = (np.zeros(1, np.uint64), np.zeros(1, np.int64))
    sj.index_clear()
    assert sj.index_join(*none, 1, 64, 1, 1).size == 0                                   # n_x = 0
    assert sj.index_join(*x, 5, 64, 1, 0).size == 0                                      # an empty index, nothing among the batch
    got = sj.index_join(*x, 5, 64, 1, 1)                                                 # the pairs among the batch
    assert got.size == 1 and (int(got[0]["a"]), int(got[0]["b"]), int(got[0]["overlap"])) == (0, 2, 5)
    assert sj.index_join(*x, 6, 64, 1, 1).size == 0                                      # one recording reaches min_overlap
    _index(sj, [_rand(100, 603)])
    assert sj.index_join(*none, 1, 64, 1, 1).size == 0
    got = sj.index_join(*x, 5, 64, 1, 0)
    assert [(int(p["a"]), int(p["b"])) for p in got] == [(0, 1), (0, 3)]
    assert sj.index_join(*x, 101, 64, 1, 1).size == 0                                    # no external reaches min_overlap
    # an external recording of 2^18 hashprints, and an indexed one
    big = _lib._ragged([np.zeros(2 ** 18, np.uint64), _rand(10, 604)], np.uint64)
    with pytest.raises(hpfw_amd.HpfwError) as e:
        sj.index_join(*big, 5, 64, 1, 1)
    assert e.value.status == _lib.E_UNSUPPORTED
    assert sj.index_join(big[0][1:], big[1] - np.array([0, 1, 1]), 5, 64, 1, 1).size == 3   # 2^18 - 1 is taken
    with pytest.raises(hpfw_amd.HpfwError) as e:
        _index(sj, [np.zeros(2 ** 18, np.uint64)])
        sj.index_join(*x, 5, 64, 1, 1)
    assert e.value.status == _lib.E_UNSUPPORTED
    sj.index_clear()


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------
def _noisy(x, seed):
    """gain 0.5 and white noise at 10 dB SNR, as synth.gen_query makes its queries"""
    seg = 0.5 * x.astype(np.float64)
    rng = np.random.default_rng([0x6E6F6973, seed])
    p = float(np.mean(seg ** 2)) + 1e-12
    seg = seg + np.sqrt(p / 10 ** (10.0 / 10)) * rng.standard_normal(seg.size)
    return np.clip(np.round(seg), -32768, 32767).astype(np.int16)


def test_known_and_add_new_end_to_end(tmp_path, filters, oracle, torch_cuda, kernel):
    """six songs of 10 s in the index; the files: song 2 again at gain 0.5 and 10 dB SNR, seconds 2 to 5 of song 4, a new song,
    and the new song in a second file.  The threshold is the geometric mean of the largest planted rate and the smallest other
    rate by the restatement on the oracle's hashprints"""
    sr = synth.SR
    songs = np.stack([synth.gen_clip(i, 10.0) for i in range(6)])
    new_song = synth.gen_clip(77, 10.0)
    pcm = {"copy": _noisy(songs[2], 7), "item": np.ascontiguousarray(songs[4][2 * sr:5 * sr]), "new_a": new_song, "new_b": new_song}
    files = []
    for stem, samples in pcm.items():
        files.append(str(tmp_path / f"{stem}.wav"))
        synth.write_wav(files[-1], samples)
    song_names = [f"song{i:02d}" for i in range(6)]
    cache = str(tmp_path / "cache") + "/"                # the collector reads the filter fixture as it reads learned filters
    os.makedirs(cache)
    with open(os.path.join(cache, "filters.cereal"), "wb") as f:
        f.write(np.array([64, 2420], np.int32).tobytes() + np.ascontiguousarray(filters, np.float32).tobytes())
    lsi, other = hpfw_amd.LiveSongIdentification(cache=cache), hpfw_amd.LiveSongIdentification(cache=cache)
    try:
        ext = lsi.collector.gpu()
        index = list(zip(ext.extract(songs), song_names))
        lsi.build(index)
        other.build(index)
        new = lsi.collector.calc_hashprints(files)
        names = song_names + [name for _, name in new]
        mode = oracle.get_projection()
        oracle.set_projection(ext.get_projection())
        try:
            if "e2e" not in _REF:                         # the CPU oracle's hashprints are the device's
                hps = list(oracle.Plan(10 * sr).extract_batch(filters, songs, 16)) + [oracle.Plan(s.size).extract(filters, s) for s in pcm.values()]
                all_hp, all_off = _lib._ragged(hps, np.uint64)
                _REF["e2e"] = (all_hp, all_off, selfjoin_ref.candidates(all_hp, all_off, 100))
        finally:
            oracle.set_projection(mode)
        all_hp, all_off, cand = _REF["e2e"]
        assert all(np.array_equal(h, all_hp[all_off[i]:all_off[i + 1]]) for i, (h, _) in enumerate(index + new))
        planted = {(2, 6), (4, 7), (8, 9)}               # (song02, copy), (song04, item), (new_a, new_b)
        worst_planted = max(Fraction(d, L) for p, (d, L, _) in cand.items() if p in planted)
        best_other = min(Fraction(d, L) for p, (d, L, _) in cand.items() if p not in planted)
        assert planted <= set(cand) and worst_planted < best_other                         # the two separate
        threshold = (float(worst_planted) * float(best_other)) ** 0.5
        print(f"largest planted rate {float(worst_planted):.2f}, smallest other rate {float(best_other):.2f}, threshold {threshold:.2f}")
        num, den = hpfw_amd.liveid.rate_fraction(threshold)
        assert worst_planted <= Fraction(num, den) < best_other
        # known() is what duplicates() gains by add(files), and changes nothing
        before = other.duplicates(threshold, 100)
        assert before == lsi.duplicates(threshold, 100) == []
        got = lsi.known(files, threshold, 100)
        assert lsi.names == song_names and lsi._gpu.index_size() == 6
        assert other.add(files) == 4
        after = other.duplicates(threshold, 100)
        assert got == [p for p in after if p not in before]
        want = ref.join(all_hp, all_off[:7], all_hp, all_off[6:], 100, num, den, 1)
        assert [(names.index(a), names.index(b), d, L, lag) for a, b, d, L, lag in got] == [tuple(int(v) for v in p)[:5] for p in want]
        assert [(a, b) for a, b, *_ in got] == [("song02", "copy"), ("song04", "item"), ("new_a", "new_b")]
        assert lsi.known(files, threshold, 100, among_new=False) == got[:2]
        # add_new() adds the new song once, and nothing the second time
        added, pairs = lsi.add_new(files, threshold, 100)
        assert added == ["new_a"] and pairs == got and lsi.names == song_names + ["new_a"] and lsi._gpu.index_size() == 7
        assert lsi._added_len[-1] == new[2][0].size
        hp, off = lsi._gpu.index_get()
        assert np.array_equal(hp[off[6]:off[7]], new[2][0])
        added, pairs = lsi.add_new(files, threshold, 100)
        assert added == [] and lsi.names == song_names + ["new_a"] and lsi._gpu.index_size() == 7
        assert [(a, b) for a, b, *_ in pairs] == [("song02", "copy"), ("song04", "item"), ("new_a", "new_a"), ("new_a", "new_b"), ("new_a", "new_b")]
        # a sharded identifier has no join
        sharded = hpfw_amd.LiveSongIdentification.__new__(hpfw_amd.LiveSongIdentification)
        sharded._gpu = object.__new__(hpfw_amd.liveid._ShardedIndex)
        for call in (sharded.known, sharded.add_new):
            with pytest.raises(hpfw_amd.HpfwError) as e:
                call(files, 16, 100)
            assert e.value.status == _lib.E_UNSUPPORTED
    finally:
        lsi._gpu.close()
        other._gpu.close()
