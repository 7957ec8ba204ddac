"""Times the two entry points of the voting search (votes.hip, k_votes.hip) of one build on one MI355X:
the host entry point, a round trip over the device entry point, and the device entry point itself.  To compare two builds,
run fresh processes in turn: [HPFW_GPU_LIB=other/libhpfw_gpu.so] python tools/time_votes.py ...

  search   the index of BASELINE.json configs[2] (10 000 clips of 30 s = 2 320 hashprints, random hashprints); the queries of
           --workload: 304 = 1 000 queries of 304 hashprints (241 windows each), 2320 = 64 queries of 2 320 (2 257 windows
           each).  hpfw_gpu_search_votes (host arrays in and out) and hpfw_gpu_search_votes_device plus the copy of the votes
           to the host, ALTERNATED in one process (--calls host or --calls device: that one alone); host wall clock around
           both, since the host entry point takes no stream (the queries of the device entry point are on the device already,
           as they are behind an extraction); one warm-up round, --reps rounds: medians with min and max, and whether the two
           gave the same bytes
  kernel   --reps + 1 calls of the device entry point alone, for `rocprofv3 --kernel-trace --stats` in a run of its own; --stats FILE
           then reads rocprofv3's output (the rocpd SQLite database, or kernel_stats.csv with `-f csv`) and adds the device time
           per call of the neighbour scan and of the tally to --out

    python tools/time_votes.py [--parts search] [--workload 304] [--reps 9] [--calls host,device] [--out profiles/votes.json]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/time_votes.py --parts kernel --workload 304 [--out ...]
    python tools/time_votes.py --stats DIR/run_results.db --workload 304 [--out ...]     (no GPU: merges into --out)

Prints one JSON line per part and merges the parts into --out.
"""
import argparse
import csv
import hashlib
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_IDX, PER = 10_000, 2320
WORKLOADS = {"304": (1000, 304), "2320": (64, 2320)}


def _setup(torch, g, workload):
    n_q, k_q = WORKLOADS[workload]
    rng = np.random.default_rng(77)
    db = rng.integers(0, 2 ** 64, size=N_IDX * PER, dtype=np.uint64)
    g.index_clear()
    g.index_add(db, np.arange(0, (N_IDX + 1) * PER, PER, dtype=np.int64))
    q = rng.integers(0, 2 ** 64, size=n_q * k_q, dtype=np.uint64)
    for i in range(0, n_q, 2):                             # every other query is a noisy cut of a clip: buckets that collect votes
        c, o = int(rng.integers(0, N_IDX)), int(rng.integers(0, PER - k_q + 1))
        flips = np.uint64(1) << rng.integers(0, 64, size=k_q, dtype=np.uint64)
        q[i * k_q:(i + 1) * k_q] = db[c * PER + o:c * PER + o + k_q] ^ flips
    q_off = np.arange(0, (n_q + 1) * k_q, k_q, dtype=np.int64)
    d_q = torch.from_numpy(q.view(np.int64)).cuda()
    d_out = torch.zeros(n_q * 24, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream()

    def host():
        return g.search_votes(q, q_off).tobytes()

    def device():
        g.search_votes_dev(d_q.data_ptr(), q_off, d_out.data_ptr(), s.cuda_stream)
        return d_out.cpu().numpy().tobytes()              # (the copy waits for the stream)
    return {"host_entry": host, "device_entry": device}, (n_q, k_q)


def part_search(torch, g, reps, workload, which=("host", "device")):
    calls, (n_q, k_q) = _setup(torch, g, workload)
    names = [name for name in calls if name.split("_")[0] in which]
    ms, same = {name: [] for name in names}, True
    for r in range(reps + 1):
        got = {}
        for name in names if r % 2 == 0 else names[::-1]:   # alternated, the order reversed every round
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got[name] = calls[name]()
            t1 = time.perf_counter()
            if r:
                ms[name].append((t1 - t0) * 1e3)
            print(f"round {r} {name}: {(t1 - t0) * 1e3:.1f} ms", file=sys.stderr, flush=True)
        same = same and len(set(got.values())) == 1
    g.index_clear()
    out = {"workload": f"{n_q} queries of {k_q} hashprints ({n_q * (k_q - 63)} windows) against {N_IDX} clips of {PER}; "
                       f"{' and '.join(names)} in turn in one process, host wall clock, {reps} rounds after one warm-up round",
           "same_bytes": same, "sha": hashlib.sha256(got[names[0]]).hexdigest()[:16]}
    for name in names:
        out[name + "_ms"] = round(float(np.median(ms[name])), 2)
        out[name + "_min_max_ms"] = [round(min(ms[name]), 2), round(max(ms[name]), 2)]
        out[name + "_all_ms"] = [round(x, 2) for x in ms[name]]
    if len(names) == 2:
        ratio = [y / x for x, y in zip(ms["host_entry"], ms["device_entry"])]
        out["device_over_host"] = round(float(np.median(ratio)), 4)
        out["device_over_host_min_max"] = [round(min(ratio), 4), round(max(ratio), 4)]
    return out


def part_kernel(torch, g, reps, workload):
    calls, _ = _setup(torch, g, workload)
    for _ in range(reps + 1):
        calls["device_entry"]()
    torch.cuda.synchronize()
    g.index_clear()
    return {"calls": reps + 1}


SCAN = ("hamming_mfma", "expand_windows")
TALLY = ("window_starts", "sort_knn_slots", "vote_events", "vote_chain", "vote_pick", "radix", "onesweep", "rocprim", "hipcub")


def merge_stats(path, rec, workload):
    calls = rec.get("kernel_run_" + workload, {}).get("calls")
    if not calls:
        raise SystemExit("no kernel_run record in --out: run --parts kernel under rocprofv3 first (with the same --out and --workload)")
    if path.endswith(".csv"):
        with open(path) as f:
            rows = [(r["Name"], float(r["TotalDurationNs"]), int(r["Calls"])) for r in csv.DictReader(f)]
    else:
        import sqlite3
        with sqlite3.connect(path) as db:
            rows = db.execute("SELECT name, sum(duration), count(*) FROM kernels GROUP BY name").fetchall()
    out = {"source": "rocprofv3 --kernel-trace --stats, a run of its own", "calls": calls, "ms_per_call": {}, "launches_per_call": {}}
    scan = tally = other = 0.0
    for name, total, n in rows:
        kind = "scan" if any(p in name for p in SCAN) else "tally" if any(p in name for p in TALLY) else "other"
        m = re.search(r"(?:\w+::)*(\w+)[<(]", name.replace("(anonymous namespace)::", ""))
        short = m.group(1) if m else name[:60]
        out["ms_per_call"][short] = round(out["ms_per_call"].get(short, 0.0) + total / calls / 1e6, 4)
        out["launches_per_call"][short] = round(out["launches_per_call"].get(short, 0.0) + n / calls, 2)
        scan, tally, other = scan + (kind == "scan") * total, tally + (kind == "tally") * total, other + (kind == "other") * total
    out["neighbour_scan_ms_per_call"] = round(scan / calls / 1e6, 3)
    out["tally_ms_per_call"] = round(tally / calls / 1e6, 3)
    out["other_ms_per_call"] = round(other / calls / 1e6, 3)
    out["tally_over_scan"] = round(tally / scan, 5) if scan else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="search")
    ap.add_argument("--workload", default="304", choices=sorted(WORKLOADS))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", default="host,device", help="the entry points the search part times: host, device or host,device")
    ap.add_argument("--stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "votes.json"))
    args = ap.parse_args()
    rec = {}
    if os.path.exists(args.out) and os.path.getsize(args.out):
        with open(args.out) as f:
            rec = json.load(f)
    rec["what"] = "the voting search: its host and its device entry point, one MI355X (DESIGN.md section 19; tools/time_votes.py)"
    if args.stats is not None:
        rec["kernels_" + args.workload] = merge_stats(args.stats, rec, args.workload)
        print(json.dumps(rec["kernels_" + args.workload]))
    else:
        import torch
        import hpfw_amd
        g = hpfw_amd.Gpu(0)
        for part in args.parts.split(","):
            extra = (tuple(args.calls.split(",")),) if part == "search" else ()
            res = {"search": part_search, "kernel": part_kernel}[part](torch, g, args.reps, args.workload, *extra)
            rec[{"search": "search_", "kernel": "kernel_run_"}[part] + args.workload] = res
            print(json.dumps({part: res}), flush=True)
        g.close()
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
