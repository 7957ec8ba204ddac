"""The scored overlap search and the timeline under the overlap rule restated in Python, independently
of the library: the rate of a candidate and the moments of a query row in Python integers over the candidates of
tests/overlap_ref.py, the score by tests/timeline_ref.py, the extent of a window on its clip, the trimmed segments, a
reference vectorised over clips of one tiny length, and concert (C) of the end-to-end tests."""
import math

import numpy as np

from hpfw_amd import synth

import overlap_ref
import timeline_ref

RATE_BITS = 10
NONE = 0xFFFFFFFF


def rate(dist, L):
    """floor(dist 2^10 / L) of a candidate (dist, L)"""
    assert 1 <= L <= 16000 and 0 <= dist <= 64 * L
    return (int(dist) << RATE_BITS) // int(L)


def candidates(db_hp, db_off, q, min_overlap):
    """[(dist, L, lag) or None] of query q against every clip"""
    return [overlap_ref.clip_candidate_fast(q, db_hp[db_off[c]:db_off[c + 1]], min_overlap) for c in range(len(db_off) - 1)]


def row_moments(cands, exclude=-1):
    """(n, sum, sum_sq) of the rates of the clips that have a candidate, but clip `exclude`"""
    r = [rate(cand[0], cand[1]) for c, cand in enumerate(cands) if cand is not None and c != exclude]
    return len(r), sum(r), sum(x * x for x in r)


def best_clip(cands, exclude=-1):
    """(clip, (dist, L, lag)) of the row's best clip by dist / L, larger L, smaller clip id; None without candidates"""
    from fractions import Fraction
    live = [((Fraction(cand[0], cand[1]), -cand[1], c), c) for c, cand in enumerate(cands) if cand is not None and c != exclude]
    if not live:
        return None
    c = min(live)[1]
    return c, cands[c]


def search_scored(db_hp, db_off, q, min_overlap, exclude=-1):
    """what the scored top-1 overlap search says of query q: (clip, dist, lag, L, (n, sum, sum_sq), score); clip None when
    no clip has a candidate"""
    cands = candidates(db_hp, db_off, q, min_overlap)
    mom = row_moments(cands, exclude)
    best = best_clip(cands, exclude)
    if best is None:
        return None, None, None, None, mom, float("nan")
    c, (dist, L, lag) = best
    return c, dist, lag, L, mom, timeline_ref.hit_score(rate(dist, L), True, *mom)


# ---- the extent of a window on its clip ---------------------------------------------------------------------------------------
def extent(d, n, k_q, span, win, m):
    """samples [a, b) of a window of k_q hashprints (span columns each, a column 3 win / m samples) found at lag d on a clip
    of n hashprints"""
    col = 3.0 * win / m
    a_cols, b_cols = max(0, -d), min(k_q + span - 1, n + span - 1 - d)
    return math.floor(a_cols * col + 0.5), min(win, math.floor(b_cols * col + 0.5))


def trimmed(seg, windows, clip_len, k_q, span, win, hop, m):
    """(start, end, offset columns) in samples of a timeline_ref.segments() record whose windows [(clip, lag, ...)] were
    searched by the overlap rule"""
    d0, d1 = windows[seg["first"]][1], windows[seg["last"]][1]
    a, _ = extent(d0, clip_len[seg["clip"]], k_q, span, win, m)
    _, b = extent(d1, clip_len[seg["clip"]], k_q, span, win, m)
    return seg["first"] * hop + a, seg["last"] * hop + b, max(0, d0)


# ---- clips of one tiny length, vectorised over the clips ------------------------------------------------------------------------
def tiny_rows(db, queries, min_overlap):
    """db [n_clips][n], queries [n_q][k] (uint64): per query (dist, L, lag) int64 [n_clips] each, the candidate of every clip
    by the order of overlap_ref (dist / L exact, larger L, smaller lag), over all n + k - 1 lags at once"""
    db, queries = np.ascontiguousarray(db, np.uint64), np.ascontiguousarray(queries, np.uint64)
    (n_clips, n), k = db.shape, queries.shape[1]
    assert min_overlap <= min(n, k)
    lags = list(range(min_overlap - k, n - min_overlap + 1))
    out = []
    for q in queries:
        best_d = best_L = best_lag = None
        for d in lags:
            j0, j1 = max(0, -d), min(k, n - d)
            L = j1 - j0
            dist = overlap_ref._popcount((db[:, d + j0:d + j1] ^ q[j0:j1]).ravel()).reshape(n_clips, L).sum(1).astype(np.int64)
            if best_d is None:
                best_d, best_L, best_lag = dist, np.full(n_clips, L, np.int64), np.full(n_clips, d, np.int64)
                continue
            # lags rise: a later lag wins on a smaller rate, or at the same rate on a larger L
            a, b = dist * best_L, best_d * L
            take = (a < b) | ((a == b) & (L > best_L))
            best_d, best_L, best_lag = np.where(take, dist, best_d), np.where(take, L, best_L), np.where(take, d, best_lag)
        out.append((best_d, best_L, best_lag))
    return out


def tiny_moments(row):
    """(n, sum, sum_sq) in Python integers of a tiny_rows() row"""
    r = [(int(d) << RATE_BITS) // int(L) for d, L in zip(row[0], row[1])]
    return len(r), sum(r), sum(x * x for x in r)


def tiny_best(row):
    """(dist, clip, lag, L) of the row's best clip"""
    from fractions import Fraction
    key = (row[0].astype(np.int64) << 29) // row[1]
    c = min(np.flatnonzero(key == key.min()), key=lambda i: (Fraction(int(row[0][i]), int(row[1][i])), -int(row[1][i]), int(i)))
    return int(row[0][c]), int(c), int(row[2][c]), int(row[1][c])


# ---- concert (C) ----------------------------------------------------------------------------------------------------------------
N_SONGS, SONG_S, ITEM_SEED, ITEM_S = 6, 10.0, 50, 3.0
# (from, to, what): a song whole, the item, or a stretch of something outside the index
CONCERT_C = [(0.0, 1.5, ("other", 0)), (1.5, 11.5, ("song", 2)), (11.5, 13.0, ("other", 1)), (13.0, 16.0, ("item", 0)),
             (16.0, 18.5, ("other", 2)), (18.5, 28.5, ("song", 4)), (28.5, 38.5, ("song", 1)), (38.5, 45.0, ("other", 3))]


def concert_c_index():
    """(pcm of songs 0-5 [6][10 s], pcm of the item [3 s], names)"""
    songs = np.stack([synth.gen_clip(i, SONG_S) for i in range(N_SONGS)])
    return songs, synth.gen_clip(ITEM_SEED, ITEM_S), [f"song{i:02d}" for i in range(N_SONGS)] + ["item"]


def concert_c():
    """45 s: song 2, the item, song 4 and song 1 whole, between stretches of clips outside the index, all at gain 0.5, white
    noise at 10 dB SNR over the whole"""
    rng = np.random.default_rng(7)
    parts = []
    for a, b, (kind, i) in CONCERT_C:
        src = {"song": lambda: synth.gen_clip(i, SONG_S), "item": lambda: synth.gen_clip(ITEM_SEED, ITEM_S),
               "other": lambda: synth.gen_clip(100 + i, b - a)}[kind]()
        part = timeline_ref._cut(src, 0.0, b - a)
        assert part.size == int(round((b - a) * synth.SR)), (a, b, part.size)
        parts.append(part)
    return timeline_ref._overlay(np.concatenate(parts), rng)
