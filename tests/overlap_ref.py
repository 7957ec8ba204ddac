"""The overlap search restated (include/hpfw_gpu.h) in numpy popcounts, Python integers and Fraction.

Query q[0..k), clip r[0..n).  Lag d puts query position j on clip position d + j.
  J(d) = {j : 0 <= j < k, 0 <= d + j < n},  L(d) = |J(d)| = min(k, n - d) - max(0, -d),
  dist(d) = sum over J(d) of popcount(q[j] ^ r[d + j]).
A lag is admissible when L(d) >= min_overlap.  Candidates are ordered by dist / L (exact), then larger L, then smaller d; a
clip's candidate is its minimum; the top_k clips of a query are ordered by dist / L, larger L, smaller clip id."""
from fractions import Fraction

import numpy as np

OVERLAP_HIT_DTYPE = np.dtype([("dist", "<u4"), ("clip", "<u4"), ("lag", "<i4"), ("overlap", "<u4")])
PAD = (0xFFFFFFFF, 0xFFFFFFFF, 0, 0)

if hasattr(np, "bitwise_count"):
    _popcount = np.bitwise_count
else:                                                    # (numpy before 2.0)
    _TAB = np.array([bin(i).count("1") for i in range(256)], np.uint8)

    def _popcount(x):
        return _TAB[np.ascontiguousarray(x, np.uint64).view(np.uint8).reshape(-1, 8)].sum(1)


def overlap(k, n, d):
    return min(k, n - d) - max(0, -d)


def lag_dists(q, r):
    """dist(d) for every lag d in -(k - 1) .. n - 1 (all lags with L >= 1), int64 [n + k - 1]; index d + k - 1"""
    q = np.ascontiguousarray(q, np.uint64)
    r = np.ascontiguousarray(r, np.uint64)
    k, n = q.size, r.size
    out = np.zeros(max(n + k - 1, 0), np.int64)
    if k == 0 or n == 0:
        return out
    for j in range(k):                                   # clip position p meets q[j] at lag p - j
        out[k - 1 - j:k - 1 - j + n] += _popcount(q[j] ^ r)
    return out


def clip_candidate(q, r, min_overlap):
    """(dist, L, lag) of the clip's best admissible lag, or None"""
    k, n = len(q), len(r)
    if k < min_overlap or n < min_overlap:
        return None
    dists = lag_dists(q, r)
    best = None
    for d in range(min_overlap - k, n - min_overlap + 1):
        L = overlap(k, n, d)
        assert L >= min_overlap
        key = (Fraction(int(dists[d + k - 1]), L), -L, d)
        if best is None or key < best[0]:
            best = (key, (int(dists[d + k - 1]), L, d))
    return best[1]


def clip_candidate_fast(q, r, min_overlap, dists=None):
    """clip_candidate with the minimum taken in numpy: dist / L compared through floor(dist 2^29 / L), which orders distinct
    fractions with denominators below 2^14 as the fractions themselves (they differ by at least 2^-28); the key's ties are
    then settled by Fraction as in clip_candidate.  dists: lag_dists(q, r) when the caller has it"""
    k, n = len(q), len(r)
    if k < min_overlap or n < min_overlap:
        return None
    if dists is None:
        dists = lag_dists(q, r)
    d = np.arange(min_overlap - k, n - min_overlap + 1, dtype=np.int64)
    L = np.minimum(k, n - d) - np.maximum(0, -d)
    dist = dists[d + k - 1]
    key = (dist << 29) // L
    best = None
    for i in np.flatnonzero(key == key.min()):
        cand = (Fraction(int(dist[i]), int(L[i])), -int(L[i]), int(d[i]))
        if best is None or cand < best[0]:
            best = (cand, (int(dist[i]), int(L[i]), int(d[i])))
    return best[1]


def search_overlap(db_hp, db_off, q_hp, q_off, top_k, min_overlap, exclude=None, clip_base=0, cache=None):
    """OVERLAP_HIT_DTYPE [n_q][top_k].  cache: a dict that keeps lag_dists per (query, clip) between calls on the same index
    and queries (other top_k, min_overlap or exclude)"""
    db_hp = np.ascontiguousarray(db_hp, np.uint64)
    q_hp = np.ascontiguousarray(q_hp, np.uint64)
    n_clips, n_q = len(db_off) - 1, len(q_off) - 1
    out = np.zeros((n_q, top_k), OVERLAP_HIT_DTYPE)
    out[:] = PAD
    for qi in range(n_q):
        q = q_hp[q_off[qi]:q_off[qi + 1]]
        rows = []
        for c in range(n_clips):
            if exclude is not None and int(exclude[qi]) == c:
                continue
            r = db_hp[db_off[c]:db_off[c + 1]]
            dists = None
            if cache is not None and len(q) >= min_overlap and len(r) >= min_overlap:
                if (qi, c) not in cache:
                    cache[(qi, c)] = lag_dists(q, r)
                dists = cache[(qi, c)]
            cand = clip_candidate_fast(q, r, min_overlap, dists)
            if cand is not None:
                dist, L, lag = cand
                rows.append(((Fraction(dist, L), -L, c), (dist, clip_base + c, lag, L)))
        rows.sort(key=lambda t: t[0])
        for t, (_, hit) in enumerate(rows[:top_k]):
            out[qi, t] = hit
    return out


def loop_candidate(q, r, min_overlap):
    """the rule bit by bit, for tiny inputs"""
    k, n = len(q), len(r)
    best = None
    for d in range(-k - 2, n + 3):
        J = [j for j in range(k) if 0 <= d + j < n]
        if len(J) < min_overlap or not J:
            continue
        dist = sum((int(q[j]) >> b & 1) != (int(r[d + j]) >> b & 1) for j in J for b in range(64))
        key = (Fraction(dist, len(J)), -len(J), d)
        if best is None or key < best[0]:
            best = (key, (dist, len(J), d))
    return None if best is None else best[1]
