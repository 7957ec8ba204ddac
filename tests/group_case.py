"""The smallest shape at which a later pass of a search over its queries can go wrong, for the tests of the searches' table
switches (HPFW_SEARCH_TABLE_KB, HPFW_OVERLAP_TABLE_KB, HPFW_LOCAL_TABLE_KB; include/hpfw_gpu.h): an index of 5 ragged clips,
one of them empty, and 70 ragged queries -- with a table of 32 queries' rows the passes take 32, 32 and 6 of them.  Query
EMPTY has no hashprint, query LONG is longer than every clip, the queries TWINS are equal and lie in different passes; two
in three of the others hold a passage of some clip with one bit in twenty flipped, so that every search has something to find
in every pass."""
import contextlib
import functools
import os

import numpy as np

CLIP_LENGTHS = (40, 300, 0, 133, 211)
N_Q, EMPTY, LONG, TWINS = 70, 66, 40, (10, 69)


@functools.lru_cache(maxsize=None)
def case():
    """(clips, queries): lists of uint64 arrays, built once and shared: leave them unchanged"""
    rng = np.random.default_rng([0x67727073, 1])
    clips = [rng.integers(0, 2 ** 64, n, dtype=np.uint64) for n in CLIP_LENGTHS]
    lengths = [int(v) for v in rng.integers(1, 121, N_Q)]
    lengths[EMPTY], lengths[LONG], lengths[TWINS[0]] = 0, 310, 90
    queries = []
    for i, k in enumerate(lengths):
        q = rng.integers(0, 2 ** 64, k, dtype=np.uint64)
        if k >= 17 and i % 3:
            c = clips[(0, 1, 3, 4)[i % 4]]
            length = min(k, c.size) * 2 // 3
            p0, j0 = (11 * i) % (c.size - length + 1), (k - length) // 2
            noise = np.zeros(length, np.uint64)
            for b in range(64):
                noise |= (rng.random(length) < 0.05).astype(np.uint64) << np.uint64(b)
            q[j0:j0 + length] = c[p0:p0 + length] ^ noise
        queries.append(q)
    queries[TWINS[1]] = queries[TWINS[0]].copy()
    return clips, queries


def planted(i):
    """query i holds a passage of a clip"""
    return i in TWINS or (i != EMPTY and i % 3 != 0 and len(case()[1][i]) >= 17)


@contextlib.contextmanager
def env(**switches):
    """the switches set for the block, and the environment as it was after it"""
    before = {name: os.environ.get(name) for name in switches}
    try:
        os.environ.update({name: str(v) for name, v in switches.items()})
        yield
    finally:
        for name, v in before.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v
