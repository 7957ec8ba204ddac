"""The timeline of a long recording restated in Python, independently of the library: the moments of
the per-clip best distances and the score of a hit in exact integers / fractions, the segment rule, the per-window search
over oracle hashprints, and the two synthetic concerts of the end-to-end tests."""
import math
from fractions import Fraction

import numpy as np

from hpfw_amd import synth

NONE = 0xFFFFFFFF


# ---- scored search ----------------------------------------------------------------------------------------------------------
def row_moments(dists, counted):
    """(n, sum d, sum d^2) in Python integers over the clips with counted[c]"""
    d = [int(x) for x, c in zip(dists, counted) if c]
    return len(d), sum(d), sum(x * x for x in d)


def hit_score(dist, counted, n, s, ss):
    """(mean of the others - d) / (their standard deviation), the others being the counted clips but the hit's; NaN when
    the hit's clip is not counted, fewer than two others exist, or they all agree"""
    if not counted or n < 3:
        return float("nan")
    d, m = int(dist), n - 1
    var = Fraction(m * (ss - d * d) - (s - d) ** 2, m * m)
    if var == 0:
        return float("nan")
    assert var > 0
    mean = Fraction(s - d, m)
    # sqrt of the exact variance: the integer square root of the numerator scaled by 4^60 keeps 17+ digits
    num = var.numerator * var.denominator                      # var = num / denominator^2
    root = Fraction(math.isqrt(num << 120), var.denominator << 60)
    return float((mean - d) / root)


def best_per_clip(oracle, q, db_hp, db_off):
    """[(distance, offset) or None] of query q against every clip (None: an empty clip has no offset)"""
    out = []
    for c in range(len(db_off) - 1):
        r = db_hp[db_off[c]:db_off[c + 1]]
        out.append(oracle.match_clip(q, r) if r.size and q.size else None)
    return out


def search_scored(oracle, q, db_hp, db_off):
    """what the scored top-1 search says of query q: (clip, dist, offset, (n, sum, sum_sq), score); clip None when no clip
    has an offset"""
    per = best_per_clip(oracle, q, db_hp, db_off)
    lens = np.diff(db_off)
    counted = [q.size >= 1 and lens[c] >= q.size for c in range(len(per))]
    mom = row_moments([p[0] if p else 0 for p in per], counted)
    live = [(p[0], c) for c, p in enumerate(per) if p]
    if not live:
        return None, None, None, mom, float("nan")
    d, c = min(live)
    return c, d, per[c][1], mom, hit_score(d, counted[c], *mom)


# ---- segments -----------------------------------------------------------------------------------------------------------------
def segments(windows, min_score, hop_cols, win, hop, tol_cols=None, max_gap=1, min_windows=1):
    """windows: [(clip or None, offset, variant, tempo, score)].  The rule, window by window: a strong window (a clip and
    score >= min_score) continues the open segment when it names its clip and its offset advanced from the last accepted
    window l as the time did, |(o_w - o_l) - rho_l (t_w - t_l)| <= tol_cols (w - l) with t = w hop_cols; otherwise it closes
    the segment and opens one.  A segment whose last accepted window lies more than max_gap windows back is closed.
    Returns dicts of the kept segments (at least min_windows strong windows)."""
    if tol_cols is None:
        tol_cols = max(2.0, 0.08 * hop_cols)
    done, cur = [], None

    def shut():
        nonlocal cur
        if cur is not None and len(cur["members"]) >= min_windows:
            done.append(cur)
        cur = None

    for w, (clip, off, variant, tempo, score) in enumerate(windows):
        if cur is not None and w - cur["members"][-1] - 1 > max_gap:
            shut()
        strong = clip is not None and clip != NONE and score >= min_score        # (NaN >= x is False)
        if not strong:
            continue
        if cur is not None and cur["clip"] == clip:
            last = cur["members"][-1]
            o_l, rho_l = windows[last][1], windows[last][3]
            if abs((float(off) - float(o_l)) - rho_l * (w * hop_cols - last * hop_cols)) <= tol_cols * (w - last):
                cur["members"].append(w)
                continue
        shut()
        cur = {"clip": clip, "members": [w]}
    shut()
    out = []
    for s in done:
        mem = s["members"]
        best = max(mem, key=lambda i: (windows[i][4], -i))                        # the highest score, the earliest on ties
        out.append(dict(clip=s["clip"], n_strong=len(mem), first=mem[0], last=mem[-1], start=mem[0] * hop, end=mem[-1] * hop + win,
                        best_window=best, best_score=windows[best][4], best_tempo=windows[best][3], best_offset=windows[best][1],
                        best_variant=windows[best][2], first_offset=windows[mem[0]][1]))
    return out


def windows_of(x, win, hop):
    n_w = 0 if x.size < win else (x.size - win) // hop + 1
    return np.stack([x[w * hop:w * hop + win] for w in range(n_w)]) if n_w else np.zeros((0, win), np.int16)


# ---- the synthetic concerts of the end-to-end tests ------------------------------------------------------------------------
def _overlay(x, rng, snr_db=10.0):
    p = float(np.mean(x ** 2)) + 1e-12
    x = x + np.sqrt(p / 10 ** (snr_db / 10)) * rng.standard_normal(x.size)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def _cut(pcm, a_s, b_s):
    return 0.5 * pcm[int(round(a_s * synth.SR)):int(round(b_s * synth.SR))].astype(np.float64)


def concert_a():
    """song 3 from 2 s for 22 s, 8 s of noise, song 11 from 0 for 28 s, song 21 (not indexed) for 20 s, song 7 from 5 s for
    15 s, song 22 (not indexed) from 3 s for 12 s, all at gain 0.5, then white noise at 10 dB SNR over the whole"""
    rng = np.random.default_rng(5)
    noise = 300.0 * rng.standard_normal(8 * synth.SR)
    parts = [_cut(synth.gen_clip(3, 30.0), 2, 24), noise, _cut(synth.gen_clip(11, 30.0), 0, 28), _cut(synth.gen_clip(21, 30.0), 0, 20),
             _cut(synth.gen_clip(7, 30.0), 5, 20), _cut(synth.gen_clip(22, 30.0), 3, 15)]
    return _overlay(np.concatenate(parts), rng)


def concert_b():
    """song 5 played 4 % faster and a semitone up [2 s, 26 s), song 21 (not indexed) for 15 s, song 9 played 4 % slower
    [1 s, 25 s), all at gain 0.5, white noise at 10 dB SNR over the whole"""
    import tempo_ref
    rng = np.random.default_rng(6)
    parts = [_cut(tempo_ref.gen_clip(5, 30.0, tempo=1.04, factor=2 ** (1 / 12)), 2, 26), _cut(synth.gen_clip(21, 30.0), 0, 15),
             _cut(tempo_ref.gen_clip(9, 30.0, tempo=0.96), 1, 25)]
    return _overlay(np.concatenate(parts), rng)
