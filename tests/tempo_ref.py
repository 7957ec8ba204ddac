"""numpy restatement of the tempo query: the step of a tempo factor, the common length of a tempo
list, the time-scaled dB spectrogram, and a synthetic clip played at another tempo."""
import numpy as np

from hpfw_amd import synth


def tempo_step(rho):
    """rint(65536 / rho) for the float32 tempo rho: sixteenths of a source column per output column"""
    return int(np.rint(65536.0 / float(np.float32(rho))))


def tempo_columns(c, tempos):
    """c_t: the fewest columns floor((c - 1) 65536 / step) + 1 any tempo of the list gives a clip of c columns"""
    return min((int(c) - 1) * 65536 // tempo_step(t) + 1 for t in np.atleast_1d(tempos))


def scale_db(db, rho):
    """db [..., C] (float32) -> [..., C_rho]: column k = (S[i] (65536 - w) + S[min(i + 1, C - 1)] w) / 65536 in float64,
    rounded once to float32, with p = k step, i = p >> 16, w = p & 0xFFFF"""
    db = np.asarray(db, np.float32)
    c = db.shape[-1]
    step = tempo_step(rho)
    k = np.arange(tempo_columns(c, [rho]), dtype=np.int64)
    p = k * step
    i, w = p >> 16, (p & 0xFFFF).astype(np.float64)
    a = db[..., i].astype(np.float64)
    b = db[..., np.minimum(i + 1, c - 1)].astype(np.float64)
    return ((a * (65536.0 - w) + b * w) / 65536.0).astype(np.float32)


def gen_clip(clip_id, seconds=30.0, tempo=1.0, factor=1.0, seed=synth.SEED):
    """the notes of synth.gen_clip(clip_id, seconds) -- the same draws in the same order -- played at `tempo` times its
    speed: each note lasts round((SR // 4) / tempo) samples and the clip round(n / tempo), n = round(seconds SR); every
    partial's frequency times `factor` (transpose_ref.gen_clip).  tempo = factor = 1 is synth.gen_clip."""
    rng = np.random.default_rng([seed, int(clip_id)])
    SR = synth.SR
    n = int(round(seconds * SR))
    n_out = int(round(n / tempo))
    note0 = SR // 4
    note = int(round(note0 / tempo))
    x = np.zeros(n_out, np.float64)
    t = np.arange(note) / SR
    fade = np.minimum(1.0, np.minimum(np.arange(note), note - 1 - np.arange(note)) / (0.010 * SR))
    for j, s0 in enumerate(range(0, n, note0)):
        f = synth.FMIN * (synth.FMAX / synth.FMIN) ** rng.random(6)
        if factor != 1.0:
            f = f * factor
        a = rng.uniform(0.05, 0.2, 6)
        ph = rng.uniform(0, 2 * np.pi, 6)
        s = j * note
        m = min(note, n_out - s)
        if m <= 0:
            continue
        seg = (a[:, None] * np.sin(2 * np.pi * f[:, None] * t[None, :m] + ph[:, None])).sum(0)
        x[s:s + m] += seg * fade[:m]
    x += 10 ** (-30 / 20) * rng.standard_normal(n_out)
    return np.clip(np.round(x * 32767 / max(1.0, np.abs(x).max())), -32768, 32767).astype(np.int16)
