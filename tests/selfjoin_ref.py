"""The catalogue self-join restated (include/hpfw_gpu.h) in numpy popcounts, Python integers and Fraction.

Clips a < b of the index in add order, both with at least min_overlap hashprints.  Clip a takes the query's part of the
overlap search (tests/overlap_ref.py) and b the clip's: lag d puts position j of a on position d + j of b,
  L(d) = min(n_a, n_b - d) - max(0, -d),  dist(d) = sum of popcount(a[j] ^ b[d + j]) over the positions both have.
A lag is admissible when L(d) >= min_overlap; candidates are ordered by dist / L (exact), then larger L, then smaller d, and the
pair's candidate is its minimum.  The pair is reported when dist * rate_den <= rate_num * L; pairs come in ascending (a, b)."""
from fractions import Fraction

import numpy as np

import overlap_ref

DUP_PAIR_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("dist", "<u4"), ("overlap", "<u4"), ("lag", "<i4"), ("pad", "<u4")])
MAX_LEN = 2 ** 18 - 1


def pair_candidate(a, b, min_overlap):
    """(dist, L, lag) of the pair's best admissible lag, or None.  The minimum is taken in numpy through
    floor(dist 2^37 / L), which orders distinct fractions with denominators below 2^18 as the fractions themselves (they
    differ by more than 2^-36; dist 2^37 <= 2^61); the key's ties are settled by Fraction."""
    n_a, n_b = len(a), len(b)
    assert n_a <= MAX_LEN and n_b <= MAX_LEN
    if n_a < min_overlap or n_b < min_overlap or min_overlap < 1:
        return None
    dists = overlap_ref.lag_dists(a, b)
    d = np.arange(min_overlap - n_a, n_b - min_overlap + 1, dtype=np.int64)
    L = np.minimum(n_a, n_b - d) - np.maximum(0, -d)
    assert (L >= min_overlap).all()
    dist = dists[d + n_a - 1]
    key = (dist << 37) // L
    best = None
    for i in np.flatnonzero(key == key.min()):
        cand = (Fraction(int(dist[i]), int(L[i])), -int(L[i]), int(d[i]))
        if best is None or cand < best[0]:
            best = (cand, (int(dist[i]), int(L[i]), int(d[i])))
    return best[1]


def reported(dist, L, rate_num, rate_den):
    assert 1 <= rate_den <= 1024 and 0 <= rate_num <= 64 * rate_den
    return dist * rate_den <= rate_num * L


def candidates(db_hp, db_off, min_overlap, cache=None):
    """{(a, b): (dist, L, lag)} for every a < b with a candidate.  cache: a dict that keeps the result per min_overlap"""
    if cache is not None and min_overlap in cache:
        return cache[min_overlap]
    db_hp = np.ascontiguousarray(db_hp, np.uint64)
    n_clips = len(db_off) - 1
    out = {}
    for a in range(n_clips):
        for b in range(a + 1, n_clips):
            cand = pair_candidate(db_hp[db_off[a]:db_off[a + 1]], db_hp[db_off[b]:db_off[b + 1]], min_overlap)
            if cand is not None:
                out[(a, b)] = cand
    if cache is not None:
        cache[min_overlap] = out
    return out


def selfjoin(db_hp, db_off, min_overlap, rate_num, rate_den, clip_base=0, cache=None):
    """DUP_PAIR_DTYPE [n]: the reported pairs in ascending (a, b)"""
    rows = [(clip_base + a, clip_base + b, dist, L, lag, 0)
            for (a, b), (dist, L, lag) in sorted(candidates(db_hp, db_off, min_overlap, cache).items())
            if reported(dist, L, rate_num, rate_den)]
    return np.array(rows, DUP_PAIR_DTYPE) if rows else np.zeros(0, DUP_PAIR_DTYPE)
