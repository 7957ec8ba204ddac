"""Times the local self-join (k_localjoin.hip) on one MI355X against the only route to the same pairs
before it: the local search all-against-all (hpfw_gpu_search_local_device, k = 64), which computes both orders of every
pair, returns at most 64 clips per query, stops at 16 000 hashprints and takes its xor/popcount kernel above about 3 000.

  index A: 2 000 clips of 2 320 hashprints, T = 22, min_score 22 * 304 (lags that overlap less than 304 are not scanned) and
           1 (every lag, as the search does).
  index B: 64 clips of 14 000 hashprints, min_score 22 * 304: the join on the matrix cores, the search on its popcount kernel.
  Each: the join and the search alternated in one process, device events around each call, one warm-up round, the median
  of --reps rounds.  Half the search's time is what computing each pair once predicts; the ratio is reported, it is not a gate.

    python tools/time_localjoin.py [--reps 9] [--clips 2000] [--out profiles/localjoin.json]

Random hashprints: the work does not depend on the values.  Prints one JSON line and writes --out.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T = 22


def summary(ms):
    return {"ms": round(float(np.median(ms)), 3), "min_max_ms": [round(min(ms), 3), round(max(ms), 3)], "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--clips", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localjoin.json"))
    args = ap.parse_args()

    import torch
    import hpfw_amd
    from hpfw_amd import _lib

    g = hpfw_amd.Gpu(0)
    rng = np.random.default_rng(2600)

    def timed(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def build(n_clips, per):
        hp = rng.integers(0, 2 ** 64, n_clips * per, dtype=np.uint64)
        off = np.arange(0, (n_clips + 1) * per, per, dtype=np.int64)
        g.index_clear()
        g.index_add(hp, off)
        d_q = torch.from_numpy(hp.view(np.int64)).cuda()
        d_hits = torch.zeros(n_clips * 64 * _lib.LOCAL_HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_pairs = torch.zeros(1024 * _lib.PASSAGE_PAIR_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
        join = lambda min_score: g.index_localjoin_dev(T, min_score, d_pairs.data_ptr(), 1024, d_count.data_ptr())
        search = lambda: g.search_local_dev(d_q.data_ptr(), off, 64, T, d_hits.data_ptr())
        return join, search, d_count

    result = {"device": torch.cuda.get_device_name(0), "geometry": dict(zip(("slice", "chunk"), _lib.localjoin_geometry())), "max_rate": T,
              "rows": []}
    for n_clips, per, scores in ((args.clips, 2320, (T * 304, 1)), (64, 14000, (T * 304,))):
        join, search, d_count = build(n_clips, per)
        for min_score in scores:
            join(min_score), search()                     # warm-up: allocations, the kernels' first launch
            torch.cuda.synchronize()
            t_join, t_search = [], []
            for _ in range(args.reps):
                t_join.append(timed(lambda: join(min_score)))
                t_search.append(timed(search))
            row = {"index": f"{n_clips} x {per}", "min_score": min_score, "pairs_reported": int(d_count.cpu()[0]),
                   "localjoin": summary(t_join), "search_local_all_against_all": summary(t_search)}
            row["localjoin_over_search"] = round(row["localjoin"]["ms"] / row["search_local_all_against_all"]["ms"], 3)
            result["rows"].append(row)
    g.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
