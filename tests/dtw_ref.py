"""The warped search (include/hpfw_gpu.h) restated in numpy int64, row by row, with the path walked
back from the recorded choices.  c(i, j) = popcount(q[i] ^ r[j]); D(0, j) = c(0, j), S(0, j) = j; for i >= 1 the smallest of
A: D(i-1, j-1) + c(i, j), B: D(i-1, j-2) + c(i, j), C: D(i-2, j-1) + c(i-1, j) + c(i, j) (i >= 2), ties to the first."""
import numpy as np

DTW_HIT_DTYPE = np.dtype([("dist", "<u4"), ("clip", "<u4"), ("start", "<i4"), ("end", "<i4")])
PAD = (0xFFFFFFFF, 0xFFFFFFFF, 0, 0)
INF = 1 << 40                                            # an unreachable cell (every real D is below 2^20)
MAX_K = 16000
MAX_PATH_CELLS = 1 << 31

if hasattr(np, "bitwise_count"):
    _popcount = np.bitwise_count
else:
    _TAB = np.array([bin(i).count("1") for i in range(256)], np.uint8)

    def _popcount(x):
        return _TAB[np.ascontiguousarray(x, np.uint64).view(np.uint8).reshape(x.shape + (8,))].sum(-1)


def costs(q, r):
    """c [K][n] int64"""
    q, r = np.asarray(q, np.uint64), np.asarray(r, np.uint64)
    return _popcount(q[:, None] ^ r[None, :]).astype(np.int64)


def reachable(k, n):
    """a clip of n columns has a candidate for a query of k hashprints"""
    return k >= 1 and n >= k // 2 + 1


def tables(q, r):
    """(c, D, S, choice) [K][n]: choice 0, 1, 2 for A, B, C (row 0 and unreachable cells: 0)"""
    c = costs(q, r)
    K, n = c.shape
    D = np.full((K, n), INF, np.int64)
    S = np.zeros((K, n), np.int64)
    ch = np.zeros((K, n), np.int8)
    D[0] = c[0]
    S[0] = np.arange(n)
    for i in range(1, K):
        best = np.full(n, INF, np.int64)
        s = np.zeros(n, np.int64)
        k = np.zeros(n, np.int8)
        best[1:] = D[i - 1, :-1]                          # A
        s[1:] = S[i - 1, :-1]
        b = np.full(n, INF, np.int64)                    # B
        sb = np.zeros(n, np.int64)
        b[2:] = D[i - 1, :-2]
        sb[2:] = S[i - 1, :-2]
        m = b < best
        best, s, k = np.where(m, b, best), np.where(m, sb, s), np.where(m, 1, k)
        if i >= 2:                                       # C
            cc = np.full(n, INF, np.int64)
            sc = np.zeros(n, np.int64)
            cc[1:] = np.where(D[i - 2, :-1] < INF, D[i - 2, :-1] + c[i - 1, 1:], INF)
            sc[1:] = S[i - 2, :-1]
            m = cc < best
            best, s, k = np.where(m, cc, best), np.where(m, sc, s), np.where(m, 2, k)
        ok = best < INF
        D[i] = np.where(ok, best + c[i], INF)
        S[i] = np.where(ok, s, 0)
        ch[i] = np.where(ok, k, 0)
    return c, D, S, ch


def pair(q, r, want_path=False):
    """(dist, start, end) of one (query, clip), or None without a candidate; want_path: (dist, start, end, path int32 [K])"""
    q, r = np.asarray(q, np.uint64), np.asarray(r, np.uint64)
    if q.size == 0 or r.size == 0:
        return None
    c, D, S, ch = tables(q, r)
    last = D[-1]
    dist = int(last.min())
    if dist >= INF:
        return None
    end = int(np.argmax(last == dist))                   # the smallest j reaching it
    start = int(S[-1, end])
    if not want_path:
        return dist, start, end
    K = q.size
    path = np.zeros(K, np.int32)
    i, j = K - 1, end
    while i > 0:
        path[i] = j
        k = int(ch[i, j])
        if k == 2:
            path[i - 1] = j
            i, j = i - 2, j - 1
        else:
            i, j = i - 1, j - 1 - k
    if i == 0:
        path[0] = j
    return dist, start, end, path


def path_identities(q, r, dist, start, end, path):
    """the three identities a path must satisfy, as a list of the ones that fail"""
    q, r, path = np.asarray(q, np.uint64), np.asarray(r, np.uint64), np.asarray(path, np.int64)
    bad = []
    if path[0] != start or path[-1] != end:
        bad.append("ends")
    inc = np.diff(path)
    if not np.isin(inc, (0, 1, 2)).all() or (inc.size and inc[0] == 0) or any(inc[t] == 0 and inc[t - 1] != 1 for t in range(1, inc.size)):
        bad.append("increments")
    if path.min() < 0 or path.max() >= r.size or int(_popcount(q ^ r[path]).sum()) != dist:
        bad.append("sum")
    return bad


def hit_of(q, r, clip, cache=None, key=None):
    """the hit of one pair; cache, key: a dict and the pair's key in it, so that a pair is computed once"""
    if cache is not None and key in cache:
        return cache[key]
    got = pair(q, r)
    hit =PAD if got is None else (got[0], clip, got[1], got[2])
    if cache is not None:
        cache[key] = hit
    return hit


def dtw_pairs(db_hp, db_off, q_hp, q_off, pairs):
    """DTW_HIT_DTYPE [n_pairs]: the clip as the pair names it"""
    out = np.zeros(len(pairs), DTW_HIT_DTYPE)
    for p, (qi, ci) in enumerate(pairs):
        out[p] = hit_of(q_hp[q_off[qi]:q_off[qi + 1]], db_hp[db_off[ci]:db_off[ci + 1]], ci)
    return out


def search_dtw(db_hp, db_off, q_hp, q_off, k, cand_clips=None, clip_base=0, cache=None):
    """DTW_HIT_DTYPE [n_q][k]: per query the k best by (dist, clip) of every clip (cand_clips None) or of the clips
    cand_clips[query] (indices in add order: the plain search's candidates), clip_base added, padding behind them;
    cache: a dict that keeps the pairs' hits between calls on the same index and queries"""
    n_q, n_clips = len(q_off) - 1, len(db_off) - 1
    out = np.zeros((n_q, k), DTW_HIT_DTYPE)
    out[:] = PAD
    for qi in range(n_q):
        q = q_hp[q_off[qi]:q_off[qi + 1]]
        clips = range(n_clips) if cand_clips is None else cand_clips[qi]
        hits = [hit_of(q, db_hp[db_off[ci]:db_off[ci + 1]], ci, cache, (qi, ci)) for ci in clips]
        hits = sorted((h[0], h[1], h[2], h[3]) for h in hits if h != PAD)[:k]
        for t, (d, ci, s, e) in enumerate(hits):
            out[qi, t] = (d, ci + clip_base, s, e)
    return out


def rigid_best(q, r):
    """the plain search's (dist, offset) of a clip no shorter than the query"""
    q, r = np.asarray(q, np.uint64), np.asarray(r, np.uint64)
    d = np.array([int(_popcount(q ^ r[o:o + q.size]).sum()) for o in range(r.size - q.size + 1)])
    return int(d.min()), int(d.argmin())


def planted(seed=20, n=2320, k=305, flips=200, start=700):
    """a clip of n random hashprints and a query of k read off it along a random admissible path from column `start` (steps
    1 and 2, a 0 only directly after a 1 and not at row 1), then `flips` distinct bits flipped: (clip, query, path)"""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    path = np.zeros(k, np.int64)
    path[0] = start
    prev = -1
    for i in range(1, k):
        options = (1, 2, 0) if prev == 1 and i >= 2 else (1, 2)
        prev = int(rng.choice(options))
        path[i] = path[i - 1] + prev
    assert path[-1] < n
    q = r[path].copy()
    for cell in rng.choice(k * 64, flips, replace=False):
        q[cell // 64] ^= np.uint64(1) << np.uint64(cell % 64)
    return r, q, path.astype(np.int32)
