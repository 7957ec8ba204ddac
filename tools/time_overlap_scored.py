"""Times the scored overlap search (overlap_stats_kernel of k_stats.hip) against the unscored one on one
MI355X.

  search   the index of BASELINE.json configs[2] (10 000 clips of 2 320 hashprints, 1 000 queries of 304, k = 1, random
           hashprints, min_overlap = 100): hpfw_gpu_search_overlap_device and hpfw_gpu_search_overlap_scored_device of the same
           build ALTERNATED in one process, device events around each call (one warm-up round, --reps rounds): medians and
           the ratio scored / unscored per round
  kernel   --reps + 1 calls of each, for `rocprofv3 --kernel-trace --stats` in a run of its own; --stats FILE then reads
           rocprofv3's output (the rocpd SQLite database, or kernel_stats.csv with `-f csv`) and adds the device time per call of
           the scan, the selection and the stats kernel to --out

    python tools/time_overlap_scored.py [--parts search] [--reps 9] [--out profiles/overlap_scored.json]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/time_overlap_scored.py --parts kernel [--out ...]
    python tools/time_overlap_scored.py --stats DIR/run_results.db [--out ...]     (no GPU: merges into --out)

Prints one JSON line per part and merges the parts into --out.
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_IDX, PER, N_Q, KQ, K, MIN_OVERLAP = 10_000, 2320, 1000, 304, 1, 100


def _setup(torch, g):
    rng = np.random.default_rng(77)
    db = rng.integers(0, 2 ** 64, size=N_IDX * PER, dtype=np.uint64)
    g.index_clear()
    g.index_add(db, np.arange(0, (N_IDX + 1) * PER, PER, dtype=np.int64))
    q = rng.integers(0, 2 ** 64, size=N_Q * KQ, dtype=np.uint64)
    q_off = np.arange(0, (N_Q + 1) * KQ, KQ, dtype=np.int64)
    d_q = torch.from_numpy(q.view(np.int64)).cuda()
    d_out = torch.empty((N_Q, K, 4), dtype=torch.int32, device="cuda")
    d_stats = torch.empty((N_Q, 3), dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream()
    calls = {"unscored": lambda: g.search_overlap_dev(d_q.data_ptr(), q_off, K, MIN_OVERLAP, d_out.data_ptr(), stream=s.cuda_stream),
             "scored": lambda: g.search_overlap_scored_dev(d_q.data_ptr(), q_off, K, MIN_OVERLAP, d_out.data_ptr(), d_stats.data_ptr(),
                                                           stream=s.cuda_stream)}
    return calls, s, (d_q, d_out, d_stats)


def part_search(torch, g, reps):
    calls, s, keep = _setup(torch, g)
    names = list(calls)
    ms = {name: [] for name in names}
    for r in range(reps + 1):
        for name in names if r % 2 == 0 else names[::-1]:   # alternated, the order reversed every round
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            calls[name]()
            b.record(s)
            b.synchronize()
            if r:
                ms[name].append(a.elapsed_time(b))
    n = keep[2].cpu().numpy()[:, 2] & 0xFFFFFFFF
    g.index_clear()
    out = {"workload": f"{N_Q} queries of {KQ} hashprints against {N_IDX} clips of {PER}, k = {K}, min_overlap = {MIN_OVERLAP}; the calls "
                       f"alternated in one process, device events, {reps} rounds after one warm-up round",
           "counted_clips_per_row": [int(n.min()), int(n.max())]}
    for name in names:
        out[name + "_ms"] = round(float(np.median(ms[name])), 3)
        out[name + "_min_max_ms"] = [round(min(ms[name]), 3), round(max(ms[name]), 3)]
    ratio = [y / x for x, y in zip(ms["unscored"], ms["scored"])]
    out["scored_over_unscored"] = round(float(np.median(ratio)), 4)
    out["scored_over_unscored_min_max"] = [round(min(ratio), 4), round(max(ratio), 4)]
    out["unscored_run_to_run_spread"] = round((max(ms["unscored"]) - min(ms["unscored"])) / float(np.median(ms["unscored"])), 4)
    return out


def part_kernel(torch, g, reps):
    calls, s, keep = _setup(torch, g)
    for name, call in calls.items():
        for _ in range(reps + 1):
            call()
    torch.cuda.synchronize()
    g.index_clear()
    return {"calls": reps + 1}


KERNELS = {"overlap_scan": "overlap_mfma", "overlap_select": "overlap_select", "overlap_stats": "overlap_stats"}


def merge_stats(path, rec):
    calls = rec.get("kernel_run", {}).get("calls")
    if not calls:
        raise SystemExit("no kernel_run record in --out: run --parts kernel under rocprofv3 first (with the same --out)")
    if path.endswith(".csv"):
        with open(path) as f:
            rows = [(r["Name"], float(r["TotalDurationNs"]), int(r["Calls"]), float(r["MinNs"]), float(r["MaxNs"])) for r in csv.DictReader(f)]
    else:
        import sqlite3
        with sqlite3.connect(path) as db:
            rows = db.execute("SELECT name, sum(duration), count(*), min(duration), max(duration) FROM kernels GROUP BY name").fetchall()
    # the scan and the selection run in both searches, the stats kernel in the scored one only
    n_calls = {"overlap_scan": 2 * calls, "overlap_select": 2 * calls, "overlap_stats": calls}
    out = {"source": "rocprofv3 --kernel-trace --stats, a run of its own", "calls_of_each_search": calls, "ms_per_call": {}}
    for key, pat in KERNELS.items():
        sel = [r for r in rows if pat in r[0]]
        if not sel:
            raise SystemExit(f"{path}: no launch of {pat}")
        out["ms_per_call"][key] = round(sum(r[1] for r in sel) / n_calls[key] / 1e6, 4)
        out["ms_per_call"][key + "_launches_per_call"] = sum(r[2] for r in sel) / n_calls[key]
        out["ms_per_call"][key + "_min_max"] = [round(min(r[3] for r in sel) / 1e6, 4), round(max(r[4] for r in sel) / 1e6, 4)]
    m = out["ms_per_call"]
    out["overlap_stats_over_scan"] = round(m["overlap_stats"] / m["overlap_scan"], 6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="search")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlap_scored.json"))
    args = ap.parse_args()
    rec = {}
    if os.path.exists(args.out) and os.path.getsize(args.out):
        with open(args.out) as f:
            rec = json.load(f)
    rec["what"] = "the scored overlap search against the unscored one on one MI355X (DESIGN.md section 18; tools/time_overlap_scored.py)"
    if args.stats is not None:
        rec["kernels"] = merge_stats(args.stats, rec)
        print(json.dumps(rec["kernels"]))
    else:
        import torch
        import hpfw_amd
        g = hpfw_amd.Gpu(0)
        for part in args.parts.split(","):
            res = {"search": part_search, "kernel": part_kernel}[part](torch, g, args.reps)
            rec[{"search": "search_1000q_10000clips", "kernel": "kernel_run"}[part]] = res
            print(json.dumps({part: res}), flush=True)
        g.close()
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
