"""The search within sets of clips restated in Python (the rule of include/hpfw_gpu.h), independently of
the library: a query with a set is answered by building the index that holds only the set's clips, in the set's order, asking
the CPU oracle's search_topk, and mapping the clip ids back.

The rule.  A call brings n_sets >= 0 sets in CSR form: set_off [n_sets + 1] (set_off[0] = 0, not decreasing) and set_clips,
clip indexes in add order (without clip_base), strictly ascending inside a set; and q_set [n_q], a set per query or -1 for
the whole index.  A clip may be in many sets, a set may be empty, a set may name an emptied slot (it is an empty clip of the
sub-index).  Query q with s = q_set[q] >= 0 gets what search_topk gives on the sub-index of set s: the order (dist, clip), the
offsets, the padding records past the set's size and k = min(k, n) for clips shorter than the query are the sub-index's;
strict ascent makes the sub-index's tie order by position the order by clip id.  clip_base is added to real hits.  The
moments of the scored form are over the counted clips of the set (n_c >= k_q >= 1).  q_set = -1: the unrestricted answer."""
import numpy as np

NONE = 0xFFFFFFFF


def check_sets(set_off, set_clips, q_set, n_q, n_slots):
    """the refusals of the rule, as a ValueError"""
    set_off, set_clips, q_set = (np.asarray(a, np.int64) for a in (set_off, set_clips, q_set))
    n_sets = set_off.size - 1
    if n_sets < 0 or (n_sets > 0 and set_off[0] != 0) or (np.diff(set_off) < 0).any():
        raise ValueError("set_off")
    for s in range(n_sets):
        c = set_clips[set_off[s]:set_off[s + 1]]
        if (c < 0).any() or (np.diff(c) <= 0).any() or (c >= n_slots).any():
            raise ValueError(f"set {s}")
    if q_set.size != n_q or (q_set < -1).any() or (q_set >= n_sets).any():
        raise ValueError("q_set")


def sub_index(db_hp, db_off, clips):
    """(hashprints, offsets) of the index that holds only `clips`, in that order"""
    db_off = np.asarray(db_off, np.int64)
    parts = [db_hp[db_off[c]:db_off[c + 1]] for c in clips]
    off = np.zeros(len(parts) + 1, np.int64)
    off[1:] = np.cumsum([p.size for p in parts])
    hp = np.concatenate(parts) if parts else np.zeros(0, np.uint64)
    return np.ascontiguousarray(hp, np.uint64), off


def _map_back(hits, clips, clip_base):
    out = hits.copy()
    real = out["clip"] != NONE
    out["clip"][real] = (np.asarray(clips, np.int64)[out["clip"][real].astype(np.int64)] + clip_base).astype(np.uint32)
    return out


def search_within(oracle, db_hp, db_off, q_hp, q_off, k, set_off, set_clips, q_set, clip_base=0):
    """HIT_DTYPE [n_q][k]: every query against the sub-index of its set (-1: the index itself)"""
    db_hp, q_hp = np.ascontiguousarray(db_hp, np.uint64), np.ascontiguousarray(q_hp, np.uint64)
    db_off, q_off = np.asarray(db_off, np.int64), np.asarray(q_off, np.int64)
    n_q = q_off.size - 1
    check_sets(set_off, set_clips, q_set, n_q, db_off.size - 1)
    out = np.zeros((n_q, k), oracle.HIT_DTYPE)
    for s in sorted(set(int(x) for x in q_set)):
        clips = np.arange(db_off.size - 1) if s < 0 else np.asarray(set_clips[set_off[s]:set_off[s + 1]], np.int64)
        hp, off = sub_index(db_hp, db_off, clips)
        for q in (i for i in range(n_q) if q_set[i] == s):
            one = oracle.search_topk(hp, off, q_hp[q_off[q]:q_off[q + 1]], np.array([0, q_off[q + 1] - q_off[q]]), k)
            out[q] = _map_back(one, clips, clip_base)[0]
    return out


def moments_within(oracle, db_hp, db_off, q_hp, q_off, set_off, set_clips, q_set):
    """[(n, sum d, sum d^2)] in Python integers: per query the best distances of the counted clips of its set"""
    db_off, q_off = np.asarray(db_off, np.int64), np.asarray(q_off, np.int64)
    out = []
    for q in range(q_off.size - 1):
        s = int(q_set[q])
        clips = range(db_off.size - 1) if s < 0 else set_clips[set_off[s]:set_off[s + 1]]
        qq = q_hp[q_off[q]:q_off[q + 1]]
        d = [oracle.match_clip(qq, db_hp[db_off[c]:db_off[c + 1]])[0] for c in clips if db_off[c + 1] - db_off[c] >= qq.size >= 1]
        out.append((len(d), sum(d), sum(x * x for x in d)))
    return out


def transposed_within(oracle, db_hp, db_off, q_hp, q_off, n_shifts, k, set_off, set_clips, q_set, clip_base=0):
    """[n_q][k] rows of (dist, clip, offset, shift_index): per clip its smallest (dist, shift index) over the query's
    variants, then the k best by (dist, clip); padding (NONE, NONE, 0, -1)"""
    q_off = np.asarray(q_off, np.int64)
    n_q = (q_off.size - 1) // n_shifts
    per = search_within(oracle, db_hp, db_off, q_hp, q_off, k, set_off, set_clips, np.repeat(np.asarray(q_set), n_shifts), clip_base)
    out = []
    for q in range(n_q):
        best = {}
        for i in range(n_shifts):
            for h in per[q * n_shifts + i]:
                if h["clip"] != NONE and (int(h["clip"]) not in best or (int(h["dist"]), i) < best[int(h["clip"])][:2]):
                    best[int(h["clip"])] = (int(h["dist"]), i, int(h["offset"]))
        rows = sorted((d, c, o, i) for c, (d, i, o) in best.items())[:k]
        out.append(rows + [(NONE, NONE, 0, -1)] * (k - len(rows)))
    return out


def brute_force(db_hp, db_off, q, clips, k, clip_base=0):
    """the rule by a bit-by-bit loop, for small cases: [(dist, clip, offset)] of the k best clips of `clips`, padded"""
    rows = []
    for c in clips:
        r = [int(x) for x in db_hp[db_off[c]:db_off[c + 1]]]
        kq = min(len(q), len(r))
        if kq < 1:
            continue
        cand = [(sum(bin(int(q[j]) ^ r[o + j]).count("1") for j in range(kq)), o) for o in range(len(r) - kq + 1)]
        d, o = min(cand)
        rows.append((d, int(c) + clip_base, o))
    rows.sort(key=lambda t: (t[0], t[1]))
    return rows[:k] + [(NONE, NONE, 0)] * (k - min(k, len(rows)))
