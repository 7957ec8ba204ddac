"""What the tests of the voting search's device tally share: a synthetic fixture of neighbour keys with
the cases that tell the rule from its near misses, the rule's parallel form restated in Python, two plausible wrong rules,
and the shard merge in numpy.  No device, no library: tests/test_votes_host.py checks all of this against the oracle's literal
loop, tests/test_gpu_votes.py sends the same fixture through the kernels."""
import numpy as np

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
POS_MASK = (1 << 40) - 1
# clip 1 is empty (an offset repeats), clip 3 holds exactly one item of 64 hashprints
DB_OFF = np.array([0, 100, 100, 300, 364, 1000], np.int64)


def key(d, pos):
    return (int(d) << 40) | int(pos)


def _windows(rows):
    """rows: per window a list of (d, pos) -> keys [n_win][5], every window ascending with padding behind the real keys"""
    out = np.full((len(rows), 5), PAD, np.uint64)
    for w, row in enumerate(rows):
        ks = sorted(key(d, p) for d, p in row)
        assert len(ks) <= 5 and len({k & POS_MASK for k in ks}) == len(ks), "positions within a window are distinct"
        out[w, :len(ks)] = ks
    return out


def _bucket(rows, clip, p0, windows, d):
    """votes for the bucket of clip whose window 0 would lie on position p0 of the clip: window i votes at p0 + i"""
    ds = d if isinstance(d, (list, tuple)) else [d] * len(windows)
    for i, di in zip(windows, ds):
        p = p0 + i
        assert 0 <= p < DB_OFF[clip + 1] - DB_OFF[clip]
        rows[i].append((di, int(DB_OFF[clip]) + p))


def query_tie():
    """case 1 (and 4: d = 0): two buckets end at 2.0; the one of clip 4 gets there first (window 2), clip 0's at window 3"""
    rows = [[] for _ in range(4)]
    _bucket(rows, 4, 10, [0, 2], 0)
    _bucket(rows, 0, 20, [1, 3], 0)
    return _windows(rows), (4, -10, np.float32(2.0))


def query_overtaken():
    """case 2: the bucket of clip 2 leads from window 0 to window 6; clip 4's bucket passes it with its last event (window 7,
    3.5); clip 0's bucket reaches 3.5 too, one window later.  Clip 2 follows the empty clip 1 and is hit in its first hashprint;
    clip 0 is hit in its last hashprint at window 8 (case 7)"""
    rows = [[] for _ in range(9)]
    _bucket(rows, 2, 0, range(0, 6), 1)
    _bucket(rows, 4, 300, range(1, 8), 1)
    _bucket(rows, 0, 91, range(2, 9), 1)
    return _windows(rows), (4, -300, np.float32(3.5))


CHAIN_D = [2, 6, 10, 12, 4, 2, 6, 14, 10, 2]


def query_chain():
    """case 3: one bucket with votes 1/3, 1/7, 1/11, ... in an order where rounding to float after every add gives another
    value than the float64 sum rounded once; around it windows with 0, 1 and 4 real keys (case 5) and the last hashprint of
    clip 4 (case 7)"""
    rows = [[] for _ in range(13)]
    _bucket(rows, 4, 40, range(0, 10), CHAIN_D)
    # window 10 stays empty, window 11 has one real key, window 12 four
    rows[11].append((900, int(DB_OFF[5]) - 1))
    rows[12] += [(700, int(DB_OFF[3])), (700, int(DB_OFF[3]) + 1), (800, 5), (4096, int(DB_OFF[2]) + 199)]
    return _windows(rows), None


def query_one_window():
    """case 6: one window; its first key wins at once"""
    return _windows([[(7, 150), (7, 151), (9, 3)]]), (2, -50, np.float32(1.0 / np.float32(8)))


def query_random(rng, n_win):
    """windows that draw their keys from a few diagonals of three clips, so that buckets collect several votes, with small
    distances (ties between buckets are common), 0 to 5 real keys per window"""
    diags = [(0, int(rng.integers(0, 30))), (2, int(rng.integers(0, 100))), (4, int(rng.integers(0, 500))), (4, int(rng.integers(0, 500))),
             (2, int(rng.integers(0, 100))), (3, 0)]
    rows = []
    for i in range(n_win):
        row, seen = [], set()
        for j in rng.permutation(len(diags))[:int(rng.integers(0, 6))]:
            clip, p0 = diags[j]
            p = p0 + i
            if p >= DB_OFF[clip + 1] - DB_OFF[clip] or int(DB_OFF[clip]) + p in seen:
                continue
            seen.add(int(DB_OFF[clip]) + p)
            row.append((int(rng.integers(0, 4)), int(DB_OFF[clip]) + p))
        rows.append(row)
    return _windows(rows)


def fixture(n_q=33, seed=77):
    """(keys [n_win][5], w_first [n_q + 1], DB_OFF): the designed queries first -- tie, overtaken, chain, one window, no
    window -- then seeded random ones of 0 to 40 windows"""
    rng = np.random.default_rng(seed)
    parts = [query_tie()[0], query_overtaken()[0], query_chain()[0], query_one_window()[0], np.zeros((0, 5), np.uint64)]
    while len(parts) < n_q:
        parts.append(query_random(rng, int(rng.integers(0, 41))))
    parts = parts[:n_q]
    w_first = np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])]).astype(np.int64)
    return np.concatenate(parts), w_first, DB_OFF.copy()


def events(keys, db_off):
    """the events of one query in stream order: (stream index, window, d, clip, offset)"""
    out = []
    for idx, k in enumerate(np.asarray(keys, np.uint64).ravel().tolist()):
        if k == int(PAD):
            continue
        d, pos, i = k >> 40, k & POS_MASK, idx // 5
        clip = min(int(np.searchsorted(db_off, pos, side="right")) - 1, db_off.size - 2)
        out.append((idx, i, d, clip, i - (pos - int(db_off[clip]))))
    return out


def vote_step(cnt, d):
    """annoy_storage.h:53: cnt = (float)((double)cnt + 1.0 / (double)(float)(d + 1))"""
    return np.float32(np.float64(cnt) + np.float64(1.0) / np.float64(np.float32(d + 1)))


def post_values(keys, db_off):
    """the parallel form's middle: events grouped stably by bucket, one chain per bucket -> {stream index: (bucket, value after it)}"""
    groups = {}
    for idx, _, d, clip, off in events(keys, db_off):
        groups.setdefault((clip, off), []).append((idx, d))
    post = {}
    for bucket, evs in groups.items():
        cnt = np.float32(0)
        for idx, d in evs:                                  # (appended in stream order: window order inside a bucket)
            cnt = vote_step(cnt, d)
            post[idx] = (bucket, cnt)
    return post


NONE = (-1, 0, np.float32(0))


def parallel_votes(keys, db_off):
    """the winner as the kernels find it: the earliest event whose post-event value is the largest of the query"""
    post = post_values(keys, db_off)
    if not post:
        return NONE
    top = max(v for _, v in post.values())
    idx = min(i for i, (_, v) in post.items() if v == top)
    return post[idx][0] + (top,)


def wrong_final_argmax(keys, db_off):
    """a plausible wrong rule: the bucket with the largest final value, ties to the smaller clip (then the smaller offset)"""
    post, final = post_values(keys, db_off), {}
    for idx in sorted(post):
        final[post[idx][0]] = post[idx][1]
    if not final:
        return NONE
    top = max(final.values())
    return min(b for b, v in final.items() if v == top) + (top,)


def wrong_last_at_max(keys, db_off):
    """another: the last event whose post-event value is the largest"""
    post = post_values(keys, db_off)
    if not post:
        return NONE
    top = max(v for _, v in post.values())
    idx = max(i for i, (_, v) in post.items() if v == top)
    return post[idx][0] + (top,)


def merge_knn(lists, pos_base):
    """lists [n_shards][n_win][5] with positions inside each shard, pos_base [n_shards] -> [n_win][5]: the 5 smallest keys with
    the bases added, ascending, padding behind them"""
    lists = np.asarray(lists, np.uint64)
    moved = np.where(lists == PAD, PAD, lists + np.asarray(pos_base, np.uint64)[:, None, None])
    allk = np.sort(np.concatenate(list(moved), axis=1), axis=1)
    return np.ascontiguousarray(allk[:, :5])


def shard_lists(rng, n_shards, n_win, spans=None):
    """per window a handful of candidates (d, global position) with few distinct distances, equal ones on both sides of every
    shard boundary; some windows have no candidate at all.  Returns (lists [n_shards][n_win][5] as each shard would report
    its own 5 nearest with positions inside the shard, pos_base [n_shards], the unsharded lists [n_win][5])."""
    spans = spans if spans is not None else rng.integers(0, 400, n_shards)
    pos_base = np.concatenate([[0], np.cumsum(spans)[:-1]]).astype(np.int64)
    total = int(np.sum(spans))
    lists = np.full((n_shards, n_win, 5), PAD, np.uint64)
    whole = np.full((n_win, 5), PAD, np.uint64)
    for w in range(n_win):
        n_c = 0 if (w % 7 == 3 or total == 0) else int(rng.integers(1, 25))
        pos = set(rng.integers(0, max(total, 1), n_c).tolist())
        cand = {p: int(rng.integers(0, 3)) for p in pos}
        for s in range(1, n_shards):                        # the same distance on both sides of the boundary
            b = int(pos_base[s])
            if w % 2 == 0 and 0 < b < total:
                cand[b - 1] = cand[b] = 1
        ks = sorted(key(d, p) for p, d in cand.items())
        whole[w, :min(5, len(ks))] = ks[:5]
        for s in range(n_shards):
            lo, hi = int(pos_base[s]), int(pos_base[s]) + int(spans[s])
            mine = sorted(key(d, p - lo) for p, d in cand.items() if lo <= p < hi)[:5]
            lists[s, w, :len(mine)] = mine
    return lists, pos_base, whole
