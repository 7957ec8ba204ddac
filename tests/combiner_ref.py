"""Checkers of the AudioCombiner tests (tests/test_gpu_combiner.py, tests/test_combiner_host.py, tools/time_combiner.py).

RefIndex.find is a loop-for-loop restatement of the reference's build_db / find
(include/hpfw/audioproblems/combiner/combiner.h:90-132): dicts and a strict `>`, the query's own recording given as an
id instead of a file name.  numpy_peaks is independent of it: per-diagonal equality counts from the value groups of
query and recording.
"""
import numpy as np

from hpfw_amd import _lib, synth

NONE = 0xFFFFFFFF


class RefIndex:
    def __init__(self, recordings):
        self.lengths = [len(r) for r in recordings]
        self.db = {}                                     # build_db, :90-97
        for j, fp in enumerate(recordings):
            for i, n in enumerate(fp.tolist()):
                self.db.setdefault(n, []).append((j, i))

    def find(self, q, exclude=-1, counts=False):
        """(rec, cnt, confidence, offset) of find (:100-132); with counts=True also the final cnt dict {(j, d): n}"""
        res = (NONE, 0, 0, 0)
        cnt = {}
        for c, n in enumerate(np.asarray(q).tolist()):
            for j, o in self.db.get(n, ()):
                if j == exclude:
                    continue
                diff = c - o
                count = cnt.get((j, diff), 0) + 1
                cnt[(j, diff)] = count
                if count > res[2]:
                    if j != res[0]:
                        res = (j, count, 1, diff)
                    else:
                        res = (j, count, res[2] + 1, diff)
        return (res, cnt) if counts else res

    def peaks(self, q, exclude=-1):
        """peak and smallest offset per recording from find's final counts: {j: (peak, offset)}"""
        _, cnt = self.find(q, exclude, counts=True)
        best = {}
        for (j, d), n in cnt.items():
            p = best.get(j)
            if p is None or n > p[0] or (n == p[0] and d < p[1]):
                best[j] = (n, d)
        return best


def numpy_peaks(q, recordings, exclude=-1):
    """per recording (peak, offset): the most positions c with q[c] == r[c - d] on one diagonal d, the smallest such d;
    (0, 0) for a recording without any equal pair (and for the excluded one)"""
    q = np.asarray(q, np.uint16)
    out = np.zeros((len(recordings), 2), np.int64)
    if q.size == 0:
        return out
    qs = np.argsort(q, kind="stable")
    qv = q[qs]
    for j, r in enumerate(recordings):
        r = np.asarray(r, np.uint16)
        if j == exclude or r.size == 0:
            continue
        rs = np.argsort(r, kind="stable")
        rv = r[rs]
        lo = np.searchsorted(rv, qv, "left")
        m = np.searchsorted(rv, qv, "right") - lo      # equal recording positions of every query position
        total = int(m.sum())
        if total == 0:
            continue
        c = np.repeat(qs, m)
        within = np.arange(total) - np.repeat(np.cumsum(m) - m, m)
        o = rs[np.repeat(lo, m) + within]
        diag = np.bincount(c - o + r.size - 1, minlength=q.size + r.size - 1)
        i = int(np.argmax(diag))                         # first maximum = smallest d
        out[j] = (diag[i], i - (r.size - 1))
    return out


def expected_topk(peaks, k):
    """(rec, peak, offset) rows ordered by (peak desc, rec asc), peak 0 left out, padded with (NONE, 0, 0)"""
    order = sorted((j for j in range(len(peaks)) if peaks[j][0] > 0), key=lambda j: (-peaks[j][0], j))[:k]
    rows = [(j, int(peaks[j][0]), int(peaks[j][1])) for j in order]
    return rows + [(NONE, 0, 0)] * (k - len(rows))


def events_per_query(queries, recordings, exclude):
    """the number of find events of every query (postings of its values outside the excluded recording)"""
    total = np.bincount(np.concatenate(recordings), minlength=65536).astype(np.int64)
    out = []
    for q, ex in zip(queries, exclude):
        per = total - (np.bincount(recordings[ex], minlength=65536) if ex >= 0 else 0)
        out.append(int(per[q].sum()))
    return out


def mel_corpus(g, n_rec=64, seed=0xC0B):
    """n_rec recordings of 60-180 s, two excerpts (at multiples of 441 samples) of each of n_rec / 2 synthetic 200 s
    sources: the combiner's Mel hashprints under filters learned from the first eight (g: hpfw_amd.Gpu)"""
    rng = np.random.default_rng(seed)
    pcm, src = [], None
    for i in range(n_rec):
        if i % 2 == 0:
            src = synth.gen_clip(1000 + i // 2, 200.0)
        dur = int(rng.integers(60, 181)) * synth.SR
        at = int(rng.integers(0, (src.size - dur) // 441 + 1)) * 441
        pcm.append(src[at:at + dur])
    g.cfg_cov_reset(_lib.COMBINER_CONFIG)
    for x in pcm[:8]:
        g.mel_cov_accumulate(x)
    g.cfg_learn_filters(_lib.COMBINER_CONFIG)
    return [g.mel_hashprints(x)[0] for x in pcm]
