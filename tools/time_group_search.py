"""Host wall time of the group searches on DESIGN.md section 6.1's workload (configs[2]: 10 000 clips x 2320 hashprints,
1 000 queries of 304, k = 10): GpuGroup.search_topk on [0] and on [0] * 8, search_topk_transposed_scored (3 variant sets) on
[0].  One warm-up, then the median of 5, every copy included; one JSON line with the three medians in ms and a digest of
each result.  To compare two builds, alternate fresh processes:
    [HPFW_GPU_LIB=other/libhpfw_gpu.so] python tools/time_group_search.py
(hpfw_amd.multi takes libhpfw_gpu_multi.so from the directory of HPFW_GPU_LIB)."""
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hpfw_amd import _lib, multi  # noqa: E402

N_CLIPS, CLIP, N_Q, Q_LEN, V, K = 10_000, 2320, 1_000, 304, 3, 10


def workload():
    """seeded: query q is a stretch of clip 7 q with one bit flipped per hashprint; its variant sets 1 and 2 flip one and two
    more"""
    rng = np.random.default_rng(61)
    db = rng.integers(0, 2 ** 64, size=N_CLIPS * CLIP, dtype=np.uint64)
    db_off = np.arange(N_CLIPS + 1, dtype=np.int64) * CLIP
    start = db_off[(np.arange(N_Q) * 7) % N_CLIPS] + rng.integers(0, CLIP - Q_LEN + 1, N_Q)
    sets = np.empty((N_Q, V, Q_LEN), np.uint64)
    sets[:, 0] = db[start[:, None] + np.arange(Q_LEN)]
    for v in range(V):
        if v:
            sets[:, v] = sets[:, v - 1]
        sets[:, v] ^= np.uint64(1) << rng.integers(0, 64, size=(N_Q, Q_LEN), dtype=np.uint64)
    return db, db_off, sets


def timed(call):
    call()
    ms, out = [], None
    for _ in range(5):
        t = time.perf_counter()
        out = call()
        ms.append((time.perf_counter() - t) * 1e3)
    parts = out if isinstance(out, tuple) else (out,)
    return round(statistics.median(ms), 3), hashlib.sha256(b"".join(p.tobytes() for p in parts)).hexdigest()[:16]


def main():
    db, db_off, sets = workload()
    plain = np.ascontiguousarray(sets[:, 0]).ravel()
    plain_off = np.arange(N_Q + 1, dtype=np.int64) * Q_LEN
    every, every_off = sets.ravel(), np.arange(N_Q * V + 1, dtype=np.int64) * Q_LEN
    res = {"lib": os.path.dirname(_lib.LIB_PATH), "ms": {}, "sha": {}}
    for devices in ([0], [0] * 8):
        g = multi.GpuGroup(devices)
        try:
            g.index_build(db, db_off)
            cases = {f"plain_{len(devices)}": lambda: g.search_topk(plain, plain_off, K)}
            if len(devices) == 1:
                cases["transposed_scored_1"] = lambda: g.search_topk_transposed_scored(every, every_off, V, K)
            for name, call in cases.items():
                res["ms"][name], res["sha"][name] = timed(call)
        finally:
            g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
