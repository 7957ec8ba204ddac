"""The local self-join restated (include/hpfw_gpu.h) on top of tests/local_ref.py.

Clips a < b of the index in add order, both non-empty.  Clip a takes the query's part of the local search and b the clip's:
lag d puts position j of a on position d + j of b, x_j = T - popcount(a[j] ^ b[d + j]), a run [j0, j1) scores sum x_j, and the
pair's candidate is local_ref.clip_candidate(a, b, T): larger score, then smaller lag, then smaller j1, then smaller j0.  The
pair is reported when score >= min_score; pairs come in ascending (a, b).  Every lag is looked at: the device's pruning of
lags that overlap less than ceil(min_score / T) is a claim about this rule, which candidate_pruned() states for the tests."""
import numpy as np

import local_ref

PASSAGE_PAIR_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("score", "<i4"), ("lag", "<i4"), ("a_start", "<u4"), ("length", "<u4"),
                               ("dist", "<u4"), ("pad", "<u4")])
MAX_LEN = 2 ** 18 - 1


def candidates(db_hp, db_off, T, cache=None):
    """{(a, b): (score, lag, a_start, length, dist)} for every a < b with a run that scores at least 1.  cache: a dict that
    keeps the result per T"""
    if cache is not None and T in cache:
        return cache[T]
    db_hp = np.ascontiguousarray(db_hp, np.uint64)
    n_clips = len(db_off) - 1
    out = {}
    for a in range(n_clips):
        for b in range(a + 1, n_clips):
            cand = local_ref.clip_candidate(db_hp[db_off[a]:db_off[a + 1]], db_hp[db_off[b]:db_off[b + 1]], T)
            if cand is not None:
                out[(a, b)] = cand
    if cache is not None:
        cache[T] = out
    return out


def localjoin(db_hp, db_off, T, min_score, clip_base=0, cache=None):
    """PASSAGE_PAIR_DTYPE [n]: the reported pairs in ascending (a, b)"""
    assert 1 <= T <= 31 and min_score >= 1
    rows = [(clip_base + a, clip_base + b, score, lag, j0, length, dist, 0)
            for (a, b), (score, lag, j0, length, dist) in sorted(candidates(db_hp, db_off, T, cache).items()) if score >= min_score]
    return np.array(rows, PASSAGE_PAIR_DTYPE) if rows else np.zeros(0, PASSAGE_PAIR_DTYPE)


def candidate_pruned(a, b, T, min_len):
    """clip_candidate over the lags with overlap L(d) = min(n_a, n_b - d) - max(0, -d) >= min_len only, by the forward pass of
    every such lag in rising order (best on strict >)"""
    n_a, n_b = len(a), len(b)
    best = None
    for d in range(min_len - n_a, n_b - min_len + 1):
        run = local_ref.diagonal_run(a, b, d, T)
        if run is not None and (best is None or run[0] > best[0]):
            best = (run[0], d, run[1], run[2] - run[1], T * (run[2] - run[1]) - run[0])
    return best
