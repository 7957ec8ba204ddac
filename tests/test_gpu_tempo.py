"""Queries at another tempo on the GPU: the hashprints of time-scaled (and bin-shifted) dB spectrograms
bit for bit against the oracle on the restated spectrogram, the sub-batches of the scaled-spectrogram workspace, the search
over the tempo x shift variants, and live identification of queries played faster or slower than the indexed recording."""
import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, synth

import tempo_ref as ref
import transpose_ref

pytestmark = pytest.mark.gpu
TEMPOS = [1.0, 0.92, 1.08, 0.5, 2.0, 0.97]
SHIFTS = [0, 2, -2, 24]


def _want(oracle, filters, db, tempos, shifts):
    """[V][n_hp_t] of one clip's dB spectrogram by the restatement and the oracle"""
    ct = ref.tempo_columns(db.shape[1], np.float32(tempos))
    out = []
    for rho in tempos:
        scaled = ref.scale_db(db, rho)[:, :ct]
        for s in (shifts or [0]):
            out.append(oracle.hashprints_from_db(filters, transpose_ref.shift_db(scaled, s)))
    return np.stack(out)


@pytest.mark.parametrize("n", [220500, 220493, 1323000, 2646000])
def test_tempo_extraction_is_exact(gpu, oracle, filters, n):
    """from PCM (host and device) and from dB, every (tempo, shift) variant equals the oracle on the scaled, shifted dB
    spectrogram cut to the common length; 7-smooth and chirp-z lengths, 5 s to 60 s"""
    import torch
    n_clips = 2 if n < 2_000_000 else 1
    clips = np.stack([synth.gen_clip(400 + i, n / synth.SR)[:n] for i in range(n_clips)])
    g = gpu.geometry(n)
    d_pcm = torch.from_numpy(clips).cuda()
    d_db = torch.empty((n_clips, 121, g.c), dtype=torch.float32, device="cuda")
    gpu.stage_spectrogram_dev(d_pcm.data_ptr(), n, n_clips, d_db.data_ptr())
    torch.cuda.synchronize()
    db = d_db.cpu().numpy()
    ct = ref.tempo_columns(g.c, np.float32(TEMPOS))
    assert _lib.tempo_columns(g.c, TEMPOS) == ct
    for shifts in (None, SHIFTS):
        V = len(TEMPOS) * (len(shifts) if shifts else 1)
        hp = gpu.extract_tempo(clips, TEMPOS, shifts)
        assert hp.shape == (n_clips, V, ct - 99)
        d_hp = torch.zeros((n_clips, V, ct - 99), dtype=torch.int64, device="cuda")
        gpu.hashprints_from_db_tempo_dev(d_db.data_ptr(), n_clips, g.c, TEMPOS, d_hp.data_ptr(), shifts)
        d_hp2 = torch.zeros_like(d_hp)
        gpu.extract_tempo_dev(d_pcm.data_ptr(), n, n_clips, TEMPOS, d_hp2.data_ptr(), shifts)
        torch.cuda.synchronize()
        from_db, from_dev = d_hp.cpu().numpy().view(np.uint64), d_hp2.cpu().numpy().view(np.uint64)
        for i in range(n_clips):
            want = _want(oracle, filters, db[i], TEMPOS, shifts)
            for v in range(V):
                assert np.array_equal(hp[i, v], want[v]), (n, i, shifts, v)
                assert np.array_equal(from_db[i, v], want[v]), (n, i, shifts, v)
                assert np.array_equal(from_dev[i, v], want[v]), (n, i, shifts, v)


def test_tempo_one_is_plain_extraction(gpu):
    x = np.stack([synth.gen_clip(7, 5.0), synth.gen_clip(8, 5.0)])
    plain = gpu.extract(x)
    assert np.array_equal(gpu.extract_tempo(x, [1.0])[:, 0], plain)
    both = gpu.extract_tempo(x, [1.0, 1.04])                          # faster: more columns, 1.0 sets the length
    assert both.shape[2] == plain.shape[1] and np.array_equal(both[:, 0], plain)
    slow = gpu.extract_tempo(x, [0.96, 1.0])                          # slower: fewer columns, the plain prefix
    assert slow.shape[2] < plain.shape[1] and np.array_equal(slow[:, 1], plain[:, :slow.shape[2]])
    with_shifts = gpu.extract_tempo(x, [0.96, 1.0], [-2, 0, 2])
    assert np.array_equal(with_shifts[:, 4], slow[:, 1])               # variant (tempo 1.0, shift 0)
    assert np.array_equal(with_shifts[:, 1], slow[:, 0])               # variant (tempo 0.96, shift 0)


def test_tempo_sub_batches(gpu, oracle, filters):
    """200 clips x 16 tempos = 3200 pairs of 179 KB: three sub-batches of the 256 MiB workspace (and from PCM two
    passes of the front end); the result equals one call per clip, and sampled clips equal the oracle"""
    import torch
    n, n_clips = 220500, 200
    tempos = list(np.linspace(0.92, 1.08, 16))
    clips = np.stack([synth.gen_clip(1000 + i, 5.0) for i in range(n_clips)])
    g = gpu.geometry(n)
    ct = ref.tempo_columns(g.c, np.float32(tempos))
    assert n_clips * len(tempos) * 121 * ct * 4 > 2 * (256 << 20)
    gpu.set_batch(128)
    try:
        hp = gpu.extract_tempo(clips, tempos)
    finally:
        gpu.set_batch(0)
    d_pcm = torch.from_numpy(clips).cuda()
    d_db = torch.empty((n_clips, 121, g.c), dtype=torch.float32, device="cuda")
    gpu.stage_spectrogram_dev(d_pcm.data_ptr(), n, n_clips, d_db.data_ptr())
    d_hp = torch.zeros((n_clips, len(tempos), ct - 99), dtype=torch.int64, device="cuda")
    gpu.hashprints_from_db_tempo_dev(d_db.data_ptr(), n_clips, g.c, tempos, d_hp.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_hp.cpu().numpy().view(np.uint64), hp)
    for i in range(n_clips):
        assert np.array_equal(gpu.extract_tempo(clips[i], tempos)[0], hp[i]), i
    db = d_db.cpu().numpy()
    for i in (0, 93, 94, 199):
        assert np.array_equal(hp[i], _want(oracle, filters, db[i], tempos, None)), i


def test_tempo_refusals(gpu):
    x = synth.gen_clip(1, 2.0)
    g = gpu.geometry(x.size)
    assert g.n_hp > 0 and ref.tempo_columns(g.c, [0.5]) - 99 < 1
    with pytest.raises(hpfw_amd.HpfwError) as e:
        gpu.extract_tempo(x, [0.5, 1.0])
    assert e.value.status == _lib.E_UNSUPPORTED
    assert gpu.extract_tempo(x, [1.0]).shape == (1, 1, g.n_hp)
    gpu.set_projection(0)
    try:
        with pytest.raises(hpfw_amd.HpfwError, match="projection mode 1"):
            gpu.extract_tempo(synth.gen_clip(1, 5.0), [0.96, 1.0])
    finally:
        gpu.set_projection(1)
    for bad in ([], [1.0, 1.0000001], [0.4], [float("nan")]):
        with pytest.raises(ValueError):
            gpu.extract_tempo(x, bad)


def test_tempo_search_is_exact(gpu, oracle):
    """V = 3 tempos x 3 shifts per query through search_topk_transposed equals the merge of the oracle's per-set lists, and
    the winning variant of a query played at (tempo, t semitones) decodes to (tempo, 2t)"""
    tempos, shifts = [0.96, 1.0, 1.04], [-2, 0, 2]
    V = len(tempos) * len(shifts)
    idx = [synth.gen_clip(c, 12.0) for c in range(10)]
    idx_hp = gpu.extract(np.stack(idx))
    db_hp, db_off = _lib._ragged(list(idx_hp), np.uint64)
    gpu.index_clear()
    gpu.index_add(db_hp, db_off)
    truth = [(3, 1.04, 1), (6, 0.96, -1), (8, 1.04, 0), (1, 1.0, 1)]
    sets = []
    for c, rho, t in truth:
        src = ref.gen_clip(c, 12.0, tempo=rho, factor=2.0 ** (t / 12))
        q = src[synth.SR * 2:synth.SR * 7]
        sets.extend(gpu.extract_tempo(q, tempos, shifts)[0])
    q_hp, q_off = _lib._ragged(sets, np.uint64)
    try:
        for k in (1, 4, 12):
            got = gpu.search_topk_transposed(q_hp, q_off, V, k)
            per = oracle.search_topk(db_hp, db_off, q_hp, q_off, k).reshape(len(truth), V, k)
            assert [[tuple(int(v) for v in h) for h in row] for row in got] == transpose_ref.merge_shifts(per, k), k
        best = gpu.search_topk_transposed(q_hp, q_off, V, 1)[:, 0]
        for h, (c, rho, t) in zip(best, truth):
            j, i = divmod(int(h["shift_index"]), len(shifts))
            assert (int(h["clip"]), tempos[j], shifts[i]) == (c, rho, 2 * t), (h, c, rho, t)
    finally:
        gpu.index_clear()


def test_live_identification_across_tempi(tmp_path, gpu):
    """32 thirty-second songs indexed from WAV; 5 s slices of the songs played 8 and 4 % slower and 4 and 8 % faster, at
    10 dB SNR: with tempos [0.92, 0.96, 1, 1.04, 1.08] every query's best clip is its source at its own tempo, at the
    offset of the slice in the indexed recording, and the source's distance is smallest at the true tempo"""
    n_idx, tempos = 32, [0.92, 0.96, 1.0, 1.04, 1.08]
    paths = []
    for c in range(n_idx):
        p = str(tmp_path / f"song{c:02d}.wav")
        synth.write_wav(p, synth.gen_clip(c, 30.0))
        paths.append(p)
    g_idx = gpu.geometry(int(round(30.0 * synth.SR)))
    song = [f"song{c:02d}" for c in range(n_idx)]

    def make(q, rho, t=0):
        src = [None] * n_idx
        c = (5 * q + 3) % n_idx
        src[c] = ref.gen_clip(c, 30.0, tempo=rho, factor=2.0 ** (t / 12))
        pcm, ci, start = synth.gen_query(src, c)
        p = str(tmp_path / f"q{q}_song{ci:02d}.wav")
        synth.write_wav(p, pcm)
        return p, (ci, rho, t, start)

    made = [make(q, (0.92, 0.96, 1.04, 1.08)[q % 4]) for q in range(8)]
    queries, truth = [m[0] for m in made], [m[1] for m in made]
    lsi = hpfw_amd.LiveSongIdentification()
    try:
        lsi.index(paths)
        hits = lsi.top(queries, 1, tempos=tempos)
        plain = lsi.top(queries, 1)
        plain_top1 = sum(bool(row) and row[0][1] == song[ci] for (_, row), (ci, *_) in zip(plain, truth))
        print(f"\ntop-1 of {len(queries)} queries at tempi 0.92-1.08: without tempos {plain_top1}, with tempos "
              f"{sum(b[0][1] == song[ci] for (_, b), (ci, *_) in zip(hits, truth))}")
        ext = lsi.collector.gpu()
        for (label, best), q, (ci, rho, t, start) in zip(hits, queries, truth):
            dist, name, offset, shift, tempo = best[0]
            assert name == song[ci] and tempo == rho and shift == 0, (label, best, rho)
            want_off = round(start * rho * g_idx.c / g_idx.n_samples)
            assert abs(offset - want_off) <= 3, (label, offset, want_off)
            # per variant the source's distance: smallest at the true tempo, below the unscaled query's
            sets = list(ext.extract_tempo(_lib.wav_read(q), tempos)[0])
            q_hp, q_off = _lib._ragged(sets, np.uint64)
            per = lsi._gpu.search_topk(q_hp, q_off, n_idx)
            d = [int(row["dist"][row["clip"] == ci][0]) for row in per]
            assert d[tempos.index(rho)] == min(d) == dist and d[tempos.index(rho)] < d[tempos.index(1.0)], (label, d)
        # tempo and key together: 4 % off and a semitone up or down, found at (tempo, 2t)
        more = [make(8 + q, rho, t) for q, (rho, t) in enumerate(((0.96, 1), (1.04, -1), (0.96, -1), (1.04, 1)))]
        both = lsi.top([m[0] for m in more], 1, shifts=[-2, 0, 2], tempos=[0.96, 1.0, 1.04])
        for (label, best), (_, (ci, rho, t, start)) in zip(both, more):
            dist, name, offset, shift, tempo = best[0]
            assert (name, tempo, shift) == (song[ci], rho, 2 * t), (label, best)
        wrong, acc = lsi.search(queries, tempos=tempos)
        assert wrong == 0 and acc == 1.0
        # files without a hashprint get None, as without tempos; bad lists and mode 0 raise instead
        synth.write_wav(str(tmp_path / "short.wav"), synth.gen_clip(0, 0.5))
        synth.write_wav(str(tmp_path / "r48.wav"), synth.gen_clip(0, 6.0), rate=48000)
        synth.write_wav(str(tmp_path / "two_s.wav"), synth.gen_clip(0, 2.0))
        odd = [str(tmp_path / "short.wav"), str(tmp_path / "missing.wav"), str(tmp_path / "r48.wav")]
        assert lsi.top(odd, 1, tempos=tempos) == [(f, None) for f in odd]
        two = str(tmp_path / "two_s.wav")
        assert lsi.top([two], 1, tempos=[0.5, 1.0]) == [(two, None)]           # too short for the slowest tempo
        assert lsi.top([two], 1, tempos=[1.0])[0][1] is not None
        for bad in ([1.0, 1.0], [], [2.5], [0.0], list(np.linspace(0.9, 1.1, 65))):
            with pytest.raises(ValueError):
                lsi.top(queries[:1], 1, tempos=bad)
        with pytest.raises(ValueError):
            lsi.top(queries[:1], 1, shifts=list(range(-10, 11)), tempos=[0.96, 1.0, 1.04, 1.08])   # 84 variants
        ext.set_projection(0)
        try:
            with pytest.raises(hpfw_amd.HpfwError, match="projection mode 1"):
                lsi.top(queries[:1], 1, tempos=[0.96, 1.0])
        finally:
            ext.set_projection(1)
    finally:
        lsi._gpu.close()
