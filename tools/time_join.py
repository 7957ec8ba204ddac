"""Times the ingest check (hpfw_gpu_index_join) on one MI355X against the route a caller had before it:
index_add of the batch, index_selfjoin of the whole index, index_remove of the batch.

  index A: 2 000 clips of 2 320 hashprints, batches of 1, 32 and 200 recordings of 2 320, min_overlap 304, threshold 16.  The
           join and the old route alternate in one process, device events around each, one warm-up round, the median of
           --reps rounds.  The old route's index is rebuilt before each of its rounds (untimed): index_remove keeps the slots,
           and the route would otherwise join a longer index every round.  Then the self-join of index A alone.
  index B: --big clips of 2 320 (default 100 000), batches of 1 and 32: the join, and the overlap search with k = 64 on the
           same batch (reported, no condition).  --big 0 leaves it out.

One invocation is one process and one build.  --tree DIR times the package of another checkout (a build of the parent commit:
it has no join, so only the old route and the self-join are timed); --label names the run, and the run is appended to --out:

    python tools/time_join.py --label this                     # this build: join, old route, self-join, index B
    python tools/time_join.py --label parent-1 --tree ../parent --big 0
    python tools/time_join.py --label this-2 --big 0
    python tools/time_join.py --label parent-2 --tree ../parent --big 0

The join must beat the parent's old route by more than parent-1 and parent-2 differ, and this build's self-join must not be
slower than the parent's by more than that spread (section 23 records both).  Random hashprints: the work does not depend on
the values.  Prints the run as one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summary(ms):
    return {"ms": round(float(np.median(ms)), 3), "min_max_ms": [round(min(ms), 3), round(max(ms), 3)], "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--clips", type=int, default=2000)
    ap.add_argument("--big", type=int, default=100000)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "join.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))

    import torch
    import hpfw_amd

    g = hpfw_amd.Gpu(0)
    has_join = hasattr(g, "index_join_dev")
    rng = np.random.default_rng(2300)
    per, mo = 2320, 304
    d_pairs = torch.zeros(1024 * 24, dtype=torch.uint8, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")

    def timed(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def build(hp, off):
        g.index_clear()
        g.index_add(hp, off)

    def batch(m):
        x = rng.integers(0, 2 ** 64, m * per, dtype=np.uint64)
        return torch.from_numpy(x.view(np.int64)).cuda(), np.arange(0, (m + 1) * per, per, dtype=np.int64)

    run = {"label": args.label, "device": torch.cuda.get_device_name(0), "has_join": has_join, "min_overlap": mo, "threshold": 16, "rows": []}
    n = args.clips
    hp = rng.integers(0, 2 ** 64, n * per, dtype=np.uint64)
    off = np.arange(0, (n + 1) * per, per, dtype=np.int64)
    for m in (1, 32, 200):
        d_x, x_off = batch(m)
        ids = np.arange(n, n + m)

        def old_route():
            g.index_add_dev(d_x.data_ptr(), x_off)
            g.index_selfjoin_dev(mo, 16, 1, d_pairs.data_ptr(), 1024, d_count.data_ptr())
            g.index_remove(ids)

        join = lambda: g.index_join_dev(d_x.data_ptr(), x_off, mo, 16, 1, 1, d_pairs.data_ptr(), 1024, d_count.data_ptr())
        t_join, t_old = [], []
        for rep in range(args.reps + 1):                  # (round 0 is the warm-up: allocations, the kernels' first launch)
            build(hp, off)
            torch.cuda.synchronize()
            if has_join:
                t_join.append(timed(join))
            t_old.append(timed(old_route))
        # workgroup pairs (row group, b): the join's, and the self-join's of the index with the batch appended
        groups = lambda rows: (rows + 31) // 32
        row = {"index": f"{n} x {per}", "batch": m, "add_selfjoin_remove": summary(t_old[1:]),
               "workgroup_pairs": {"join": sum(max(n + m - max(n, 32 * q + 1), 0) for q in range(groups(n + m))),
                                   "selfjoin_of_both": sum(max(n + m - 32 * q - 1, 0) for q in range(groups(n + m)))}}
        if has_join:
            row["join"] = summary(t_join[1:])
            row["join_over_old_route"] = round(row["join"]["ms"] / row["add_selfjoin_remove"]["ms"], 4)
        run["rows"].append(row)
    build(hp, off)
    selfjoin = lambda: g.index_selfjoin_dev(mo, 16, 1, d_pairs.data_ptr(), 1024, d_count.data_ptr())
    selfjoin()
    torch.cuda.synchronize()
    run["selfjoin"] = dict(summary([timed(selfjoin) for _ in range(args.reps)]), index=f"{n} x {per}")

    if args.big and has_join:
        n = args.big
        hp = rng.integers(0, 2 ** 64, n * per, dtype=np.uint64)
        off = np.arange(0, (n + 1) * per, per, dtype=np.int64)
        build(hp, off)
        del hp
        for m in (1, 32):
            d_x, x_off = batch(m)
            d_hits = torch.zeros(m * 64 * 16, dtype=torch.uint8, device="cuda")
            join = lambda: g.index_join_dev(d_x.data_ptr(), x_off, mo, 16, 1, 1, d_pairs.data_ptr(), 1024, d_count.data_ptr())
            search = lambda: g.search_overlap_dev(d_x.data_ptr(), x_off, 64, mo, d_hits.data_ptr())
            join(), search()
            torch.cuda.synchronize()
            t_join, t_search = [], []
            for _ in range(args.reps):
                t_join.append(timed(join))
                t_search.append(timed(search))
            run["rows"].append({"index": f"{n} x {per}", "batch": m, "join": summary(t_join), "search_overlap_k64": summary(t_search)})
    g.close()

    result = {"runs": []}
    if os.path.exists(args.out):
        with open(args.out) as f:
            result = json.load(f)
    result["runs"] = [r for r in result["runs"] if r["label"] != args.label] + [run]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(run))


if __name__ == "__main__":
    main()
