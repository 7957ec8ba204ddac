"""Times the catalogue self-join (k_selfjoin.hip) on one MI355X against the only route to the same
pairs before it: the overlap search all-against-all with `exclude` (hpfw_gpu_search_overlap_device, k = 64), which computes
both orders of every pair, returns at most 64 clips per query and stops at 16 000 hashprints.

  index A: 2 000 clips of 2 320 hashprints, min_overlap 304 and 100, threshold 16: the self-join and the overlap search
           alternated in one process, device events around each call, one warm-up round, the median of --reps rounds.
           About half the search's time is what the halved work predicts; the ratio is reported, it is not a gate.
  index B: 64 clips of 14 000 hashprints, min_overlap 304: the self-join on the matrix cores (the overlap search takes
           its xor/popcount kernel above about 3 000 hashprints), one warm-up and --long-reps runs; the search once.

    python tools/time_selfjoin.py [--reps 9] [--long-reps 3] [--clips 2000] [--out profiles/selfjoin.json]

Random hashprints: the work does not depend on the values.  Prints one JSON line and writes --out.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(ms):
    return {"ms": round(float(np.median(ms)), 3), "min_max_ms": [round(min(ms), 3), round(max(ms), 3)], "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--long-reps", type=int, default=3)
    ap.add_argument("--clips", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selfjoin.json"))
    args = ap.parse_args()

    import torch
    import hpfw_amd
    from hpfw_amd import _lib

    g = hpfw_amd.Gpu(0)
    rng = np.random.default_rng(2200)

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
        d_hits = torch.zeros(n_clips * 64 * 16, dtype=torch.uint8, device="cuda")
        d_pairs = torch.zeros(1024 * 24, dtype=torch.uint8, device="cuda")
        d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
        me = np.arange(n_clips, dtype=np.int32)
        join = lambda mo: g.index_selfjoin_dev(mo, 16, 1, d_pairs.data_ptr(), 1024, d_count.data_ptr())
        search = lambda mo: g.search_overlap_dev(d_q.data_ptr(), off, 64, mo, d_hits.data_ptr(), exclude=me)
        return join, search, d_count

    result = {"device": torch.cuda.get_device_name(0), "geometry": dict(zip(("slice", "chunk"), _lib.selfjoin_geometry())), "rows": []}
    join, search, d_count = build(args.clips, 2320)
    for mo in (304, 100):
        join(mo), search(mo)                              # warm-up: allocations, the kernels' first launch
        torch.cuda.synchronize()
        t_join, t_search = [], []
        for _ in range(args.reps):
            t_join.append(timed(lambda: join(mo)))
            t_search.append(timed(lambda: search(mo)))
        row = {"index": f"{args.clips} x 2320", "min_overlap": mo, "pairs_reported": int(d_count.cpu()[0]),
               "selfjoin": summary(t_join), "search_overlap_all_against_all": summary(t_search)}
        row["selfjoin_over_search"] = round(row["selfjoin"]["ms"] / row["search_overlap_all_against_all"]["ms"], 3)
        result["rows"].append(row)
    join, search, d_count = build(64, 14000)
    join(304)
    torch.cuda.synchronize()
    row = {"index": "64 x 14000", "min_overlap": 304, "selfjoin": summary([timed(lambda: join(304)) for _ in range(args.long_reps)]),
           "search_overlap_all_against_all": summary([timed(lambda: search(304))]), "pairs_reported": int(d_count.cpu()[0])}
    row["selfjoin_over_search"] = round(row["selfjoin"]["ms"] / row["search_overlap_all_against_all"]["ms"], 3)
    result["rows"].append(row)
    g.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
