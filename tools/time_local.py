"""Times the local search (k_search_local.hip) against the plain search on one MI355X.

  search   the index of BASELINE.json configs[2] (10 000 clips of 30 s = 2 320 hashprints, 1 000 query slices of 5 s = 304
           hashprints, k = 10, random hashprints, the shapes of tools/time_overlap.py): hpfw_gpu_search_topk_device and
           hpfw_gpu_search_local_device of the same build with max_rate = 22 and 31, ALTERNATED in one process, device
           events around each call (one warm-up round, --reps rounds): medians with min and max, the ratios local / plain
           per round, the ratio of lags counted (n + k - 1) / (n - k + 1), and a digest of each call's hits

    python tools/time_local.py [--reps 9] [--out profiles/local.json]
    python tools/time_local.py --lib A/libhpfw_gpu.so --lib B/libhpfw_gpu.so [--turns 1]

--lib (may repeat): the part runs for each library named, each run in a process of its own (HPFW_GPU_LIB), the libraries
taken in turn --turns times; the record of a run is then keyed "<library>#<turn>".  Random hashprints score nothing at 22
bits a hashprint and nearly every clip has a run at 31: the scan's work is the same, the top-k's is not.

Prints one JSON line per run and merges the runs into --out.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_IDX, PER, N_Q, KQ, K = 10_000, 2320, 1000, 304, 10
MAX_RATES = (22, 31)


def _setup(torch, g):
    rng = np.random.default_rng(77)
    db = rng.integers(0, 2 ** 64, size=N_IDX * PER, dtype=np.uint64)
    g.index_clear()
    g.index_add(db, np.arange(0, (N_IDX + 1) * PER, PER, dtype=np.int64))
    q = rng.integers(0, 2 ** 64, size=N_Q * KQ, dtype=np.uint64)
    q_off = np.arange(0, (N_Q + 1) * KQ, KQ, dtype=np.int64)
    d_q = torch.from_numpy(q.view(np.int64)).cuda()
    outs = {"plain": torch.zeros((N_Q, K, 4), dtype=torch.int32, device="cuda")}
    s = torch.cuda.current_stream()
    calls = {"plain": lambda: g.search_topk_dev(d_q.data_ptr(), q_off, K, outs["plain"].data_ptr(), s.cuda_stream)}
    for T in MAX_RATES:
        outs[f"local_{T}"] = torch.zeros((N_Q, K, 6), dtype=torch.int32, device="cuda")
        calls[f"local_{T}"] = lambda T=T: g.search_local_dev(d_q.data_ptr(), q_off, K, T, outs[f"local_{T}"].data_ptr(), stream=s.cuda_stream)
    return calls, s, outs, d_q


def part_search(torch, g, reps):
    calls, s, outs, keep = _setup(torch, g)
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
        out[name + "_sha256"] = hashlib.sha256(outs[name].cpu().numpy().tobytes()).hexdigest()
    for T in MAX_RATES:
        ratio = [y / x for x, y in zip(ms["plain"], ms[f"local_{T}"])]
        out[f"local_{T}_over_plain"] = round(float(np.median(ratio)), 4)
        out[f"local_{T}_over_plain_min_max"] = [round(min(ratio), 4), round(max(ratio), 4)]
    out["lags_over_plain_offsets"] = round((PER + KQ - 1) / (PER - KQ + 1), 4)
    out["plain_run_to_run_spread"] = round((max(ms["plain"]) - min(ms["plain"])) / float(np.median(ms["plain"])), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--lib", action="append", default=[])
    ap.add_argument("--turns", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local.json"))
    args = ap.parse_args()
    rec = {}
    if os.path.exists(args.out) and os.path.getsize(args.out):
        with open(args.out) as f:
            rec = json.load(f)
    rec["what"] = "the local search against the plain search on one MI355X (DESIGN.md section 25; tools/time_local.py)"
    if args.lib:
        for turn in range(args.turns):
            for lib in args.lib:                              # a fresh process for every library and turn
                env = dict(os.environ, HPFW_GPU_LIB=os.path.abspath(lib))
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--out", os.devnull], env=env,
                                   capture_output=True, text=True)
                if r.returncode != 0:
                    raise SystemExit(f"{lib}: exit status {r.returncode}\n{r.stderr[-2000:]}")
                res = json.loads(r.stdout.strip().splitlines()[-1])["search"]
                rec[f"{lib}#{turn}"] = res
                print(json.dumps({f"{lib}#{turn}": res}), flush=True)
    else:
        import torch
        import hpfw_amd
        g = hpfw_amd.Gpu(0)
        res = part_search(torch, g, args.reps)
        g.close()
        rec["search_1000q_10000clips"] = res
        print(json.dumps({"search": res}), flush=True)
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
