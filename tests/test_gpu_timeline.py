"""The timeline of a long recording on the GPU: the moments of the scored search integer for integer
against the oracle on all three scan kernels, the windows of one recording bit for bit against the extraction of the windows
copied out, and the set lists of two synthetic concerts end to end."""
from math import gcd

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, synth

import timeline_ref as ref

pytestmark = pytest.mark.gpu
WIN, HOP = 220500, 110250
SHIFTS, TEMPOS = [-2, 0, 2], [0.96, 1.0, 1.04]


# ---- stats --------------------------------------------------------------------------------------------------------------------
def _ragged_index(lengths, seed):
    full = synth.random_hashprints(len(lengths), max(max(lengths), 1), seed)
    return _lib._ragged([full[i, :n] for i, n in enumerate(lengths)], np.uint64)


def _planted(db_hp, db_off, specs, seed):
    """queries cut from clip c at offset o, k hashprints long, with a few bits flipped: specs [(c, o, k)]"""
    rng = np.random.default_rng(seed)
    out = []
    for c, o, k in specs:
        q = db_hp[db_off[c] + o:db_off[c] + o + k].copy()
        assert q.size == k
        for i in range(k):
            for b in rng.integers(0, 64, 6):
                q[i] ^= np.uint64(1) << np.uint64(b)
        out.append(q)
    return out


def _want_rows(oracle, queries, db_hp, db_off):
    return [ref.search_scored(oracle, q, db_hp, db_off) for q in queries]


def _close(a, b):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-12 * abs(b)


def _check_stats(stats, want):
    for i, (row, w) in enumerate(zip(stats, want)):
        assert (int(row["n"]), int(row["sum"]), int(row["sum_sq"])) == w[3], (i, row, w[3])


def test_stats_are_exact(gpu, oracle, scan_path):
    """a ragged index (clips shorter than some queries, empty clips), planted queries of mixed length and an empty one: the
    moments equal Python integers over oracle.match_clip, the hits equal search_topk's, and the score of the best hit equals
    the restatement's"""
    lengths = [400, 0, 50, 300, 20, 600, 304, 303, 64, 63, 1, 0, 512, 97, 350, 30, 31, 29, 450, 7, 120, 305, 200]
    db_hp, db_off = _ragged_index(lengths, 11)
    specs = [(0, 10, 304), (5, 250, 304), (3, 0, 64), (12, 100, 30), (14, 46, 304), (18, 3, 120), (21, 1, 304), (6, 0, 304),
             (5, 0, 600), (0, 396, 1), (20, 20, 97)]
    queries = _planted(db_hp, db_off, specs, 12) + [np.zeros(0, np.uint64)]
    q_hp, q_off = _lib._ragged(queries, np.uint64)
    want = _want_rows(oracle, queries, db_hp, db_off)
    gpu.index_clear()
    gpu.index_add(db_hp, db_off)
    try:
        for k in (1, 5):
            hits, stats = gpu.search_topk_scored(q_hp, q_off, k)
            assert np.array_equal(hits, gpu.search_topk(q_hp, q_off, k)), (scan_path, k)
            _check_stats(stats, want)
        assert int(stats[-1]["n"]) == 0 and hits[-1, 0]["clip"] == _lib.NO_CLIP          # the empty query
        assert [int(s["n"]) for s in stats[:3]] == [sum(n >= 304 for n in lengths)] * 2 + [sum(n >= 64 for n in lengths)]
        lens = np.diff(db_off)
        for i, ((c, o, kq), w) in enumerate(zip(specs, want)):
            h = hits[i, 0]
            assert (int(h["clip"]), int(h["dist"]), int(h["offset"])) == (w[0], w[1], w[2]), (i, h, w)
            # (a clip shorter than the query is compared over fewer hashprints and may win: it is not counted, so no score)
            got = _lib.hit_score(h["dist"], lens[w[0]] >= kq, stats[i])
            assert _close(got, w[4]) and np.isnan(got) == (lens[w[0]] < kq or w[3][0] < 3), (i, got, w[4])
            # the clip the query was cut from stands out from the counted clips
            d, at = oracle.match_clip(queries[i], db_hp[db_off[c]:db_off[c + 1]])
            mine = _lib.hit_score(d, True, stats[i])
            assert at == o and _close(mine, ref.hit_score(d, True, *w[3])) and (mine > 3 or w[3][0] < 3), (i, d, at, mine)
        # fewer queries than a tile, and one alone
        for sel in ([0, 3, 8], [9]):
            sub = [queries[i] for i in sel]
            s_hp, s_off = _lib._ragged(sub, np.uint64)
            hits, stats = gpu.search_topk_scored(s_hp, s_off, 3)
            assert np.array_equal(hits, gpu.search_topk(s_hp, s_off, 3))
            _check_stats(stats, [want[i] for i in sel])
    finally:
        gpu.index_clear()
    hits, stats = gpu.search_topk_scored(q_hp, q_off, 2)                                  # an empty index
    assert (stats["n"] == 0).all() and (stats["sum"] == 0).all() and (hits["clip"] == _lib.NO_CLIP).all()


def test_stats_of_a_large_index(gpu, oracle):
    """16 484 clips and 4 queries: the two-step top-k takes over and the stats row is split over workgroups"""
    rng = np.random.default_rng(21)
    lengths = [int(x) for x in rng.choice([40, 40, 40, 33, 24, 10, 0], 16484)]
    db_hp, db_off = _ragged_index(lengths, 22)
    long_clips = [c for c, n in enumerate(lengths) if n == 40]
    queries = _planted(db_hp, db_off, [(long_clips[5], 3, 24), (long_clips[-1], 0, 40), (long_clips[700], 10, 12)], 23)
    queries.append(synth.random_hashprints(1, 33, 24)[0])
    q_hp, q_off = _lib._ragged(queries, np.uint64)
    want = _want_rows(oracle, queries, db_hp, db_off)
    gpu.index_clear()
    gpu.index_add(db_hp, db_off)
    try:
        hits, stats = gpu.search_topk_scored(q_hp, q_off, 10)
        assert np.array_equal(hits, gpu.search_topk(q_hp, q_off, 10))
        _check_stats(stats, want)
        assert [int(h["clip"]) for h in hits[:3, 0]] == [long_clips[5], long_clips[-1], long_clips[700]]
        assert int(stats[1]["n"]) == lengths.count(40) and int(stats[0]["n"]) == sum(n >= 24 for n in lengths)
    finally:
        gpu.index_clear()


def test_variant_stats_are_exact(gpu, oracle):
    """the transposed form: one stats row per variant set, each equal to the plain row of that set; the hits equal
    search_topk_transposed's and are scored against the row of their shift_index"""
    lengths = [400, 0, 50, 300, 20, 600, 304, 303, 64, 310]
    db_hp, db_off = _ragged_index(lengths, 31)
    n_sets = 3
    sets = _planted(db_hp, db_off, [(0, 5, 300), (5, 100, 300), (3, 0, 300),          # query 0: three variants of 300
                                     (9, 2, 64), (6, 7, 64), (8, 0, 64),               # query 1
                                     (5, 9, 304), (5, 200, 304), (0, 50, 304)], 32)    # query 2
    q_hp, q_off = _lib._ragged(sets, np.uint64)
    want = _want_rows(oracle, sets, db_hp, db_off)
    gpu.index_clear()
    gpu.index_add(db_hp, db_off)
    try:
        hits, stats = gpu.search_topk_transposed_scored(q_hp, q_off, n_sets, 4)
        assert np.array_equal(hits, gpu.search_topk_transposed(q_hp, q_off, n_sets, 4))
        assert stats.shape == (3, n_sets)
        _check_stats(stats.ravel(), want)
        for q in range(3):
            h = hits[q, 0]
            v = int(h["shift_index"])
            w = want[q * n_sets + v]
            assert (int(h["clip"]), int(h["dist"]), int(h["offset"])) == (w[0], w[1], w[2]), (q, h, w)
            assert w[1] == min(want[q * n_sets + i][1] for i in range(n_sets))
            counted = lengths[int(h["clip"])] >= sets[q * n_sets + v].size      # (a shorter clip may win: no score then)
            got = _lib.hit_score(h["dist"], counted, stats[q, v])
            assert _close(got, w[4]) and np.isnan(got) == (not counted), (q, got, w[4])
    finally:
        gpu.index_clear()


def test_scored_search_refuses_what_could_wrap(gpu):
    """n_clips k_max^2 4096 >= 2^64 cannot be reached with queries of at most 16 000 hashprints and 2^32 clips; the bound is
    checked all the same, and the plain limit on the query length comes first"""
    db_hp, db_off = _ragged_index([10, 10], 41)
    gpu.index_clear()
    gpu.index_add(db_hp, db_off)
    try:
        with pytest.raises(hpfw_amd.HpfwError) as e:
            gpu.search_topk_scored(np.zeros(16001, np.uint64), [0, 16001], 1)
        assert e.value.status == _lib.E_UNSUPPORTED
    finally:
        gpu.index_clear()


# ---- windows ------------------------------------------------------------------------------------------------------------------
def _recording(seconds, seed=500):
    parts = [synth.gen_clip(seed + i, 30.0) for i in range(int(np.ceil(seconds / 30.0)))]
    return np.concatenate(parts)[:int(round(seconds * synth.SR))]


def _windows_dev(gpu, x, win, hop, tempos=None, shifts=None):
    import torch
    n_w, sets, nhp, _, _ = gpu._windows_shape(x.size, win, hop, tempos, shifts)
    d_pcm = torch.from_numpy(x).cuda()
    d_hp = torch.zeros((n_w, sets, nhp), dtype=torch.int64, device="cuda")
    gpu.extract_windows_dev(d_pcm.data_ptr(), x.size, win, hop, d_hp.data_ptr(), tempos, shifts)
    torch.cuda.synchronize()
    out = d_hp.cpu().numpy().view(np.uint64)
    return out if (tempos is not None or shifts is not None) else out[:, 0, :]


@pytest.mark.parametrize("win", [220500, 220493])
def test_windows_are_exact(gpu, win):
    """windows at an even, an odd and a full-window hop of a 33 s recording, a 7-smooth and a chirp-z window length: from
    host and from device pointers, plain, shifted, at other tempos and both, bit for bit what the extraction of the windows
    copied out gives; also in several passes and (plain) in projection mode 0"""
    x = _recording(33.0)
    for hop in (110250, 44101, win):
        w = ref.windows_of(x, win, hop)
        assert w.shape[0] == _lib.window_count(x.size, win, hop) >= 6
        want = gpu.extract(w)
        assert np.array_equal(gpu.extract_windows(x, win, hop), want), (win, hop)
        assert np.array_equal(_windows_dev(gpu, x, win, hop), want), (win, hop)
        for tempos, shifts, direct in ((None, SHIFTS, lambda: gpu.extract_transposed(w, SHIFTS)),
                                       (TEMPOS, None, lambda: gpu.extract_tempo(w, TEMPOS)),
                                       (TEMPOS, SHIFTS, lambda: gpu.extract_tempo(w, TEMPOS, SHIFTS))):
            want_v = direct()
            assert np.array_equal(gpu.extract_windows(x, win, hop, tempos, shifts), want_v), (win, hop, tempos, shifts)
            assert np.array_equal(_windows_dev(gpu, x, win, hop, tempos, shifts), want_v), (win, hop, tempos, shifts)
    hop = 44101
    w = ref.windows_of(x, win, hop)
    want = gpu.extract(w)
    gpu.set_batch(7)                                                       # 28 windows in four passes
    try:
        assert np.array_equal(gpu.extract_windows(x, win, hop), want)
        assert np.array_equal(gpu.extract_windows(x, win, hop, TEMPOS, SHIFTS), gpu.extract_tempo(w, TEMPOS, SHIFTS))
    finally:
        gpu.set_batch(0)
    gpu.set_projection(0)
    try:
        assert np.array_equal(gpu.extract_windows(x, win, hop), gpu.extract(w))
        with pytest.raises(hpfw_amd.HpfwError, match="projection mode 1"):
            gpu.extract_windows(x, win, hop, shifts=SHIFTS)
        with pytest.raises(hpfw_amd.HpfwError, match="projection mode 1"):
            gpu.extract_windows(x, win, hop, tempos=TEMPOS)
    finally:
        gpu.set_projection(1)


def test_windows_of_a_twenty_minute_recording(gpu):
    """twenty minutes, 106 MB of PCM uploaded once: 479 windows of 5 s every 2.5 s in two passes; nothing of a recording
    shorter than a window"""
    base = _recording(120.0, seed=600)
    rng = np.random.default_rng(7)
    x = np.concatenate([np.roll(base, int(rng.integers(0, base.size))) for _ in range(10)])
    assert x.size == 20 * 60 * synth.SR
    got = gpu.extract_windows(x, WIN, HOP)
    assert got.shape == (479, gpu.geometry(WIN).n_hp)
    w = ref.windows_of(x, WIN, HOP)
    assert np.array_equal(got, gpu.extract(w))
    assert np.array_equal(_windows_dev(gpu, x, WIN, HOP), got)
    short = x[:WIN - 1]
    assert gpu.extract_windows(short, WIN, HOP).shape == (0, gpu.geometry(WIN).n_hp)
    assert gpu.extract_windows(short, WIN, HOP, TEMPOS, SHIFTS).shape[:2] == (0, 9)
    assert gpu.extract_windows(np.zeros(0, np.int16), WIN, HOP).shape[0] == 0


# ---- end to end ---------------------------------------------------------------------------------------------------------------
N_SONGS = 20


def _lsi(filters, resample=False):
    """an identifier whose collector holds the filter fixture and whose index holds the 20 songs hashed under it"""
    lsi = hpfw_amd.LiveSongIdentification(resample=resample)
    ext = lsi.collector.gpu()
    ext.set_filters(filters)
    hp = ext.extract(np.stack([synth.gen_clip(i, 30.0) for i in range(N_SONGS)]))
    lsi.build([(hp[i], f"song{i:02d}") for i in range(N_SONGS)])
    return lsi, hp


def _ranges(segs):
    """(song number, first window, last window) of timeline()'s segments at the 5 s / 2.5 s default"""
    return [(int(name[4:]), int(round(a / 2.5)), int(round((b - 5.0) / 2.5))) for a, b, name, *_ in segs]


def test_timeline_of_a_concert(tmp_path, filters, oracle, torch_cuda):
    """concert (A): three indexed songs, noise and two songs outside the index.  Every window's clip, distance, offset and
    score equal the restatement over oracle hashprints; min_score = 10 gives exactly the three segments"""
    x = ref.concert_a()
    path = str(tmp_path / "concert_a.wav")
    synth.write_wav(path, x)
    lsi, idx_hp = _lsi(filters)
    try:
        segs, wins = lsi.timeline(path, min_score=10, windows=True)
        want_idx = oracle.Plan(30 * synth.SR).extract_batch(filters, np.stack([synth.gen_clip(i, 30.0) for i in range(N_SONGS)]), 16)
        assert np.array_equal(idx_hp, want_idx)
        db_hp, db_off = _lib._ragged(list(want_idx), np.uint64)
        w_hp = oracle.Plan(WIN).extract_batch(filters, ref.windows_of(x, WIN, HOP), 16)
        assert len(wins) == 41 == w_hp.shape[0]
        rows = []
        for w, (clip, name, dist, off, score, shift, tempo) in enumerate(wins):
            c, d, o, mom, s = ref.search_scored(oracle, w_hp[w], db_hp, db_off)
            print(f"window {w:2d}: clip {clip:2d} dist {dist:5d} offset {off:5d} score {score:6.2f}")
            assert (clip, dist, off) == (c, d, o) and name == f"song{c:02d}" and (shift, tempo) == (0, 1.0), (w, wins[w], c, d, o)
            assert abs(score - s) <= 1e-12 * abs(s), (w, score, s)
            rows.append((c, o, 0, 1.0, s))
        assert _ranges(segs) == [(3, 0, 7), (11, 12, 22), (7, 31, 36)], segs
        m = lsi._gpu.geometry(WIN).m
        want_segs = ref.segments(rows, 10.0, HOP * m / (3.0 * WIN), WIN, HOP)
        assert [(s["clip"], s["first"], s["last"]) for s in want_segs] == _ranges(segs)
        for (a, b, name, score, off_s, shift, tempo), s in zip(segs, want_segs):
            assert (a, b, score) == (s["start"] / synth.SR, s["end"] / synth.SR, s["best_score"])
            assert abs(off_s - s["first_offset"] * 3.0 * WIN / m / synth.SR) < 1e-9 and (shift, tempo) == (0, 1.0)
        in_segment = {w for _, a, b in _ranges(segs) for w in range(a, b + 1)}
        assert not in_segment & (set(range(9, 12)) | set(range(23, 31)) | set(range(37, 41)))
        # the songs start where the concert took them from: song 3 from 2 s, song 11 from 0, song 7 from 5 s + 2.5 s
        assert [round(s[4], 1) for s in segs] == [2.0, 0.0, 4.5]
        # short and unreadable files have no timeline; a missing min_score is refused
        synth.write_wav(str(tmp_path / "short.wav"), x[:WIN - 1])
        assert lsi.timeline(str(tmp_path / "short.wav"), 10) == [] and lsi.timeline(str(tmp_path / "missing.wav"), 10) == []
        assert lsi.timeline(str(tmp_path / "short.wav"), 10, windows=True) == ([], [])
        with pytest.raises(hpfw_amd.HpfwError):
            lsi.timeline(path, 0.0)
        with pytest.raises(hpfw_amd.HpfwError):
            lsi.timeline(path, 10, window_s=5.0, hop_s=6.0)
    finally:
        lsi._gpu.close()


def test_timeline_with_variants(tmp_path, filters, torch_cuda):
    """concert (B): song 5 played 4 % faster and a semitone up, a song outside the index, song 9 played 4 % slower.  With
    tempos and shifts both are found at their (tempo, shift); without, song 5 is not (a semitone away it scores below 10)
    and song 9 still is (4 % off it still scores above 20, and its offsets chain under the default tolerance)"""
    x = ref.concert_b()
    path = str(tmp_path / "concert_b.wav")
    synth.write_wav(path, x)
    lsi, _ = _lsi(filters)
    try:
        segs, wins = lsi.timeline(path, min_score=10, tempos=TEMPOS, shifts=SHIFTS, windows=True)
        assert len(wins) == 24
        for w, row in enumerate(wins):
            print(f"variants window {w:2d}: clip {row[0]} dist {row[2]} offset {row[3]} score {row[4]:.2f} shift {row[5]} tempo {row[6]:g}")
        assert _ranges(segs) == [(5, 0, 8), (9, 16, 23)], segs
        assert [(s[5], s[6]) for s in segs] == [(2, float(np.float32(1.04))), (0, float(np.float32(0.96)))]
        assert all(wins[w][0] == 5 and wins[w][5:] == (2, float(np.float32(1.04))) and wins[w][4] >= 10 for w in range(0, 9))
        assert all(wins[w][0] == 9 and wins[w][5:] == (0, float(np.float32(0.96))) and wins[w][4] >= 10 for w in range(16, 24))
        assert all(not wins[w][4] >= 10 for w in range(9, 16))
        plain, pw = lsi.timeline(path, min_score=10, windows=True)
        for w, row in enumerate(pw):
            print(f"plain window {w:2d}: clip {row[0]} dist {row[2]} offset {row[3]} score {row[4]:.2f}")
        assert all(name != "song05" for _, _, name, *_ in plain)
        assert _ranges(plain) == [(9, 16, 23)], plain
        assert all(pw[w][0] == 5 and pw[w][4] < 10 for w in range(0, 9))
        assert all(pw[w][0] == 9 and pw[w][4] > 20 for w in range(16, 24))
    finally:
        lsi._gpu.close()


def test_timeline_of_a_48k_file(tmp_path, filters, torch_cuda):
    """concert (A) converted to 48 kHz on the host and read with resample=True: the same three songs in the same order (the
    resampler changes the samples, so the window ranges may move by one: they are printed, not asserted)"""
    from scipy.signal import resample_poly
    g = gcd(44100, 48000)
    y = resample_poly(ref.concert_a().astype(np.float64), 48000 // g, 44100 // g)
    path = str(tmp_path / "concert_a_48k.wav")
    synth.write_wav(path, np.clip(np.round(y), -32768, 32767).astype(np.int16), rate=48000)
    lsi, _ = _lsi(filters, resample=True)
    try:
        segs = lsi.timeline(path, min_score=10)
        print("48 kHz:", _ranges(segs))
        assert [name for _, _, name, *_ in segs] == ["song03", "song11", "song07"]
        plain = hpfw_amd.LiveSongIdentification()                           # without the switch a 48 kHz file is unreadable
        try:
            assert plain.timeline(path, min_score=10) == []
        finally:
            plain._gpu.close()
    finally:
        lsi._gpu.close()
