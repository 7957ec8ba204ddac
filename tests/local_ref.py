"""The local search restated (include/hpfw_gpu.h) in numpy popcounts and integer arrays.

Query q[0..k), clip r[0..n), max_rate T in 1..31.  Lag d = 1 - k .. n - 1 puts query position j on clip position d + j; both
have the positions [ja, jb), ja = max(0, -d), jb = min(k, n - d).  x_j = T - popcount(q[j] ^ r[d + j]).  A run is a non-empty
[j0, j1) inside [ja, jb): score = sum x_j, dist = sum popcount, length = j1 - j0.  A clip's candidate is its best run over all
lags: larger score, then smaller lag, then smaller j1, then smaller j0; a clip is a hit only with score >= 1; a query's top_k
hits are ordered by larger score, then smaller clip id."""
import numpy as np

LOCAL_HIT_DTYPE = np.dtype([("score", "<i4"), ("clip", "<u4"), ("lag", "<i4"), ("q_start", "<u4"), ("length", "<u4"), ("dist", "<u4")])
PAD = (0, 0xFFFFFFFF, 0, 0, 0, 0)
_CELLS = 1 << 23                                         # cells of one block of lags

if hasattr(np, "bitwise_count"):
    _popcount = np.bitwise_count
else:                                                    # (numpy before 2.0)
    _TAB = np.array([bin(i).count("1") for i in range(256)], np.uint8)

    def _popcount(x):
        x = np.ascontiguousarray(x, np.uint64)
        return _TAB[x.view(np.uint8).reshape(x.shape + (8,))].sum(-1)


def diagonal_run(q, r, d, T):
    """(score, j0, j1) of the best run at lag d by the forward pass -- prefix minimum updated on strict <, best on strict > --
    or None where the lag has no position or no run scores above 0"""
    k, n = len(q), len(r)
    ja, jb = max(0, -d), min(k, n - d)
    if jb <= ja:
        return None
    x = T - _popcount(np.asarray(q[ja:jb], np.uint64) ^ np.asarray(r[d + ja:d + jb], np.uint64)).astype(np.int64)
    p, mn, mpos, best = 0, 0, ja, None
    for j, v in enumerate(x.tolist(), ja):
        p += v
        if best is None or p - mn > best[0]:
            best = (p - mn, mpos, j + 1)
        if p < mn:
            mn, mpos = p, j + 1
    return best if best[0] >= 1 else None


def lag_scores_by_steps(q, r, T):
    """lag_scores one query position at a time: step j advances the forward pass of the n lags that have position j (clip
    position p meets q[j] at lag p - j) and leaves the others alone"""
    q = np.ascontiguousarray(q, np.uint64)
    r = np.ascontiguousarray(r, np.uint64)
    k, n = q.size, r.size
    best = np.zeros(max(n + k - 1, 0), np.int32)
    if k == 0 or n == 0:
        return best.astype(np.int64)
    pre, low = np.zeros_like(best), np.zeros_like(best)
    for j in range(k):
        s = slice(k - 1 - j, k - 1 - j + n)
        pre[s] += np.int32(T) - _popcount(q[j] ^ r).astype(np.int32)
        np.maximum(best[s], pre[s] - low[s], out=best[s])
        np.minimum(low[s], pre[s], out=low[s])
    return best.astype(np.int64)


def lag_scores(q, r, T):
    """the best run's score at every lag d = 1 - k .. n - 1 (0 where no run scores above 0), int64 [n + k - 1]; index d + k - 1.
    Positions outside the query or the clip count as x = -1: every step there is strictly negative, so no best run reaches
    into them (lag_scores_by_steps and enumerate_candidate do without that argument)"""
    q = np.ascontiguousarray(q, np.uint64)
    r = np.ascontiguousarray(r, np.uint64)
    k, n = q.size, r.size
    out = np.zeros(max(n + k - 1, 0), np.int64)
    if k == 0 or n == 0:
        return out
    if k * (n + k - 1) > _CELLS:                         # (long queries: the table of every (lag, position) costs more than k steps)
        return lag_scores_by_steps(q, r, T)
    # row i of either view is lag i - (k - 1): the clip positions query positions 0 .. k - 1 lie on, and whether they exist
    pad = np.zeros(k - 1, np.uint64)
    on = np.lib.stride_tricks.sliding_window_view(np.concatenate([pad, r, pad]), k)
    real = np.lib.stride_tricks.sliding_window_view(np.concatenate([pad, np.ones(n, np.uint64), pad]).astype(bool), k)
    block = max(1, _CELLS // k)
    for i0 in range(0, n + k - 1, block):
        i1 = min(i0 + block, n + k - 1)
        x = np.where(real[i0:i1], np.int8(T) - _popcount(on[i0:i1] ^ q[None, :]).astype(np.int8), np.int8(-1))
        pre = np.cumsum(x, axis=1, dtype=np.int32)
        low = np.minimum.accumulate(pre[:, :-1], axis=1)
        np.minimum(low, 0, out=low)                      # (the empty prefix)
        pre[:, 1:] -= low
        out[i0:i1] = np.maximum(pre.max(axis=1), 0)
    return out


def clip_candidate(q, r, T):
    """(score, lag, j0, length, dist) of the clip's best run, or None"""
    k, n = len(q), len(r)
    if k == 0 or n == 0:
        return None
    scores = lag_scores(q, r, T)
    i = int(np.argmax(scores))                           # (the first maximum: the smaller lag)
    if scores[i] < 1:
        return None
    d = i - (k - 1)
    score, j0, j1 = diagonal_run(q, r, d, T)
    assert score == scores[i]
    return (score, d, j0, j1 - j0, T * (j1 - j0) - score)


def enumerate_candidate(q, r, T):
    """the rule by enumeration of every run of every lag, bit by bit, for tiny inputs"""
    k, n = len(q), len(r)
    best = None
    for d in range(-k - 2, n + 3):
        J = [j for j in range(k) if 0 <= d + j < n]
        for j0 in J:
            for j1 in range(j0 + 1, J[-1] + 2):
                dist = sum((int(q[j]) >> b & 1) != (int(r[d + j]) >> b & 1) for j in range(j0, j1) for b in range(64))
                score = T * (j1 - j0) - dist
                key = (-score, d, j1, j0)
                if score >= 1 and (best is None or key < best[0]):
                    best = (key, (score, d, j0, j1 - j0, dist))
    return None if best is None else best[1]


def half_shared_query(song, foreign, seconds, share, cut_s, snr_db, seed, sr=44100):
    """int16 PCM of `seconds`: the first `share` of it is `song` from second cut_s on, the rest is the start of `foreign`;
    gain 0.5 and white noise at snr_db, as synth.gen_query makes its queries"""
    n = int(round(seconds * sr))
    n_a = int(round(share * n))
    a0 = int(round(cut_s * sr))
    seg = 0.5 * np.concatenate([song[a0:a0 + n_a], foreign[:n - n_a]]).astype(np.float64)
    rng = np.random.default_rng([0x6C6F636C, int(seed)])
    p = float(np.mean(seg ** 2)) + 1e-12
    seg = seg + np.sqrt(p / 10 ** (snr_db / 10)) * rng.standard_normal(n)
    return np.clip(np.round(seg), -32768, 32767).astype(np.int16)


def search_local(db_hp, db_off, q_hp, q_off, top_k, T, clip_base=0):
    """LOCAL_HIT_DTYPE [n_q][top_k]"""
    db_hp = np.ascontiguousarray(db_hp, np.uint64)
    q_hp = np.ascontiguousarray(q_hp, np.uint64)
    n_clips, n_q = len(db_off) - 1, len(q_off) - 1
    out = np.zeros((n_q, top_k), LOCAL_HIT_DTYPE)
    out[:] = PAD
    for qi in range(n_q):
        q = q_hp[q_off[qi]:q_off[qi + 1]]
        rows = []
        for c in range(n_clips):
            cand = clip_candidate(q, db_hp[db_off[c]:db_off[c + 1]], T)
            if cand is not None:
                score, lag, j0, length, dist = cand
                rows.append(((-score, c), (score, clip_base + c, lag, j0, length, dist)))
        rows.sort(key=lambda t: t[0])
        for t, (_, hit) in enumerate(rows[:top_k]):
            out[qi, t] = hit
    return out
