"""Times the search within sets (hpfw_gpu_search_topk_within_device) on one MI355X against the search of
the whole index.

  The index is BASELINE configs[2]: 10 000 clips of 2 320 random hashprints, 1 000 queries of 304, k = 10.  Device events
  around each call, one warm-up round, the median of --reps rounds, the calls alternated in one process:
    whole      search_topk_dev of the whole index (the only call a build of the parent commit has)
    one100     every query within one set of 100 clips
    sets32     32 different sets of 100 clips over the 1 000 queries
    one5000    every query within one set of 5 000 clips
  then, on a second handle that holds just the 100 clips of `one100`, search_topk_dev (`sub100`).

One invocation is one process and one build.  --tree DIR times the package of another checkout (a build of the parent commit:
it has no search within sets, so only `whole` and `sub100` are timed); --label names the run, and the run is appended to --out:

    python tools/time_within.py --label this-1
    python tools/time_within.py --label parent-1 --tree ../parent
    python tools/time_within.py --label this-2
    python tools/time_within.py --label parent-2 --tree ../parent

Two conditions, each against the parent (section 24 records both): `one100` of this build is faster than the parent's `whole`
by more than parent-1 and parent-2 differ, and this build's `whole` is not slower than the parent's by more than that spread.
Random hashprints: the work does not depend on the values.  Prints the run as one JSON line.
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
    ap.add_argument("--clips", type=int, default=10000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "within.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))

    import torch
    import hpfw_amd

    if not torch.cuda.is_available():
        raise SystemExit("time_within.py needs an MI355X: there is no fallback")
    g, small = hpfw_amd.Gpu(0), hpfw_amd.Gpu(0)
    has_within = hasattr(g, "search_topk_within_dev")
    rng = np.random.default_rng(2400)
    n, per, n_q, kq, k = args.clips, 2320, args.queries, 304, 10
    hp = rng.integers(0, 2 ** 64, n * per, dtype=np.uint64)
    g.index_add(hp, np.arange(0, (n + 1) * per, per, dtype=np.int64))
    sets = [np.sort(rng.choice(n, 100, replace=False)).astype(np.int32) for _ in range(32)]
    half = np.sort(rng.choice(n, n // 2, replace=False)).astype(np.int32)
    small.index_add(np.concatenate([hp[c * per:(c + 1) * per] for c in sets[0]]), np.arange(0, 101 * per, per, dtype=np.int64))
    del hp
    q = rng.integers(0, 2 ** 64, n_q * kq, dtype=np.uint64)
    d_q = torch.from_numpy(q.view(np.int64)).cuda()
    q_off = np.arange(0, (n_q + 1) * kq, kq, dtype=np.int64)
    d_out = torch.zeros(n_q * k * 16, dtype=torch.uint8, device="cuda")
    zeros = np.zeros(n_q, np.int32)
    csr = lambda ss: (np.concatenate([[0], np.cumsum([len(s) for s in ss])]).astype(np.int64), np.concatenate(ss).astype(np.int32))

    calls = {"whole": lambda: g.search_topk_dev(d_q.data_ptr(), q_off, k, d_out.data_ptr())}
    if has_within:
        one, many, big = csr(sets[:1]), csr(sets), csr([half])
        by32 = (np.arange(n_q) % 32).astype(np.int32)
        calls["one100"] = lambda: g.search_topk_within_dev(d_q.data_ptr(), q_off, k, one[0], one[1], zeros, d_out.data_ptr())
        calls["sets32"] = lambda: g.search_topk_within_dev(d_q.data_ptr(), q_off, k, many[0], many[1], by32, d_out.data_ptr())
        calls["one5000"] = lambda: g.search_topk_within_dev(d_q.data_ptr(), q_off, k, big[0], big[1], zeros, d_out.data_ptr())
    calls["sub100"] = lambda: small.search_topk_dev(d_q.data_ptr(), q_off, k, d_out.data_ptr())

    def timed(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    times = {name: [] for name in calls}
    for rep in range(args.reps + 1):                      # (round 0 is the warm-up: allocations, the kernels' first launch)
        for name, call in calls.items():
            torch.cuda.synchronize()
            times[name].append(timed(call))
    run = {"label": args.label, "device": torch.cuda.get_device_name(0), "has_within": has_within, "index": f"{n} x {per}",
           "queries": f"{n_q} x {kq}", "k": k, "rows": {name: summary(ms[1:]) for name, ms in times.items()}}
    g.close()
    small.close()

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
