"""The ingest check restated (include/hpfw_gpu.h): the join of m recordings that are not in the index
against it is what index_add followed by index_selfjoin would add to the self-join's answer.  So the restatement appends the
recordings to the index, runs tests/selfjoin_ref.py on the concatenation and keeps the pairs (a, b) with n <= b (and a < n
unless among_new): nothing of the rule is stated a second time."""
import numpy as np

import selfjoin_ref

DUP_PAIR_DTYPE = selfjoin_ref.DUP_PAIR_DTYPE


def appended(db_hp, db_off, x_hp, x_off):
    """(hashprints, offsets) of the index with the recordings behind it"""
    db_off, x_off = np.asarray(db_off, np.int64), np.asarray(x_off, np.int64)
    db = np.ascontiguousarray(db_hp, np.uint64).ravel()[db_off[0]:db_off[-1]]
    x = np.ascontiguousarray(x_hp, np.uint64).ravel()[x_off[0]:x_off[-1]]
    return np.concatenate([db, x]), np.concatenate([db_off - db_off[0], x_off[1:] - x_off[0] + db.size])


def join(db_hp, db_off, x_hp, x_off, min_overlap, rate_num, rate_den, among_new, clip_base=0, cache=None):
    """DUP_PAIR_DTYPE [n]: the reported pairs in ascending (a, b).  cache: selfjoin_ref.candidates()'s, for one index and one
    batch"""
    assert among_new in (0, 1)
    n = len(db_off) - 1
    hp, off = appended(db_hp, db_off, x_hp, x_off)
    full = selfjoin_ref.selfjoin(hp, off, min_overlap, rate_num, rate_den, clip_base=clip_base, cache=cache)
    keep = full["b"].astype(np.int64) - clip_base >= n
    if not among_new:
        keep &= full["a"].astype(np.int64) - clip_base < n
    return full[keep]
