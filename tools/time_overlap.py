"""Times the overlap search (k_search_overlap.hip) against the plain search on one MI355X.

  search   the index of BASELINE.json configs[2] (10 000 clips of 30 s = 2 320 hashprints, 1 000 query slices of 5 s = 304
           hashprints, k = 10, random hashprints): hpfw_gpu_search_topk_device and hpfw_gpu_search_overlap_device of the same
           build with min_overlap = 100 and 304, ALTERNATED in one process, device events around each call (one warm-up
           round, --reps rounds): medians, the ratios overlap / plain per round, and the ratio of lags counted
           (n + k - 2 min_overlap + 1) / (n - k + 1)
  kernel   --reps + 1 calls of each of the three, for `rocprofv3 --kernel-trace --stats` in a run of its own; --stats FILE
           then reads rocprofv3's output (the rocpd SQLite database, or kernel_stats.csv with `-f csv`) and adds the device
           time per call of the scans and the selections to --out

    python tools/time_overlap.py [--parts search] [--reps 9] [--out profiles/overlap.json]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/time_overlap.py --parts kernel [--out ...]
    python tools/time_overlap.py --stats DIR/run_results.db [--out ...]     (no GPU: merges into --out)

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

N_IDX, PER, N_Q, KQ, K = 10_000, 2320, 1000, 304, 10
MIN_OVERLAPS = (100, 304)


def _setup(torch, g):
    rng = np.random.default_rng(77)
    db = rng.integers(0, 2 ** 64, size=N_IDX * PER, dtype=np.uint64)
    g.index_clear()
    g.index_add(db, np.arange(0, (N_IDX + 1) * PER, PER, dtype=np.int64))
    q = rng.integers(0, 2 ** 64, size=N_Q * KQ, dtype=np.uint64)
    q_off = np.arange(0, (N_Q + 1) * KQ, KQ, dtype=np.int64)
    d_q = torch.from_numpy(q.view(np.int64)).cuda()
    d_out = torch.empty((N_Q, K, 4), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream()
    calls = {"plain": lambda: g.search_topk_dev(d_q.data_ptr(), q_off, K, d_out.data_ptr(), s.cuda_stream)}
    for mo in MIN_OVERLAPS:
        calls[f"overlap_{mo}"] = lambda mo=mo: g.search_overlap_dev(d_q.data_ptr(), q_off, K, mo, d_out.data_ptr(), stream=s.cuda_stream)
    return calls, s, (d_q, d_out)


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
    g.index_clear()
    out = {"workload": f"{N_Q} queries of {KQ} hashprints against {N_IDX} clips of {PER}, k = {K}; the calls alternated in one process, "
                       f"device events, {reps} rounds after one warm-up round"}
    for name in names:
        out[name + "_ms"] = round(float(np.median(ms[name])), 3)
        out[name + "_min_max_ms"] = [round(min(ms[name]), 3), round(max(ms[name]), 3)]
    for mo in MIN_OVERLAPS:
        ratio = [y / x for x, y in zip(ms["plain"], ms[f"overlap_{mo}"])]
        out[f"overlap_{mo}_over_plain"] = round(float(np.median(ratio)), 4)
        out[f"overlap_{mo}_over_plain_min_max"] = [round(min(ratio), 4), round(max(ratio), 4)]
        out[f"lags_{mo}_over_plain_offsets"] = round((PER + KQ - 2 * mo + 1) / (PER - KQ + 1), 4)
    out["plain_run_to_run_spread"] = round((max(ms["plain"]) - min(ms["plain"])) / float(np.median(ms["plain"])), 4)
    return out


def part_kernel(torch, g, reps):
    calls, s, keep = _setup(torch, g)
    for name, call in calls.items():
        for _ in range(reps + 1):
            call()
    torch.cuda.synchronize()
    g.index_clear()
    return {"calls": reps + 1}


KERNELS = {"plain_scan": "hamming_mfma", "plain_topk": "topk_kernel", "overlap_scan": "overlap_mfma", "overlap_select": "overlap_select",
           "expand_queries": "expand_queries"}


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
    # the plain search runs once per round, the overlap search once per min_overlap: per-call figures divide by that
    n_calls = {"plain_scan": calls, "plain_topk": calls, "overlap_scan": calls * len(MIN_OVERLAPS), "overlap_select": calls * len(MIN_OVERLAPS),
               "expand_queries": calls * (1 + len(MIN_OVERLAPS))}
    out = {"source": "rocprofv3 --kernel-trace --stats, a run of its own", "calls_of_each_search": calls, "ms_per_call": {}}
    for key, pat in KERNELS.items():
        sel = [r for r in rows if pat in r[0]]
        if not sel:
            raise SystemExit(f"{path}: no launch of {pat}")
        out["ms_per_call"][key] = round(sum(r[1] for r in sel) / n_calls[key] / 1e6, 4)
        out["ms_per_call"][key + "_launches_per_call"] = sum(r[2] for r in sel) / n_calls[key]
        out["ms_per_call"][key + "_min_max"] = [round(min(r[3] for r in sel) / 1e6, 4), round(max(r[4] for r in sel) / 1e6, 4)]
    m = out["ms_per_call"]
    out["overlap_scan_over_plain_scan"] = round(m["overlap_scan"] / m["plain_scan"], 4)
    out["overlap_select_share"] = round(m["overlap_select"] / (m["overlap_scan"] + m["overlap_select"]), 4)
    out["note"] = ("overlap_scan and overlap_select are means over min_overlap = " + " and ".join(str(mo) for mo in MIN_OVERLAPS) +
                   "; the shortest and the longest launch of overlap_scan are those of the largest and the smallest min_overlap")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="search")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlap.json"))
    args = ap.parse_args()
    rec = {}
    if os.path.exists(args.out) and os.path.getsize(args.out):
        with open(args.out) as f:
            rec = json.load(f)
    rec["what"] = "the overlap search against the plain search on one MI355X (DESIGN.md section 17; tools/time_overlap.py)"
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
