"""Times the warped search (k_dtw.hip) on one MI355X: device events on the stream around each call, one
warm-up round, the median of --reps rounds, the calls of a round alternated (the order reversed every round).

  pairs     10 000 pairs of K = 305 by n = 2 320 (hpfw_gpu_dtw_pairs_device; query p mod 1000 against clip p): cells per second,
            and with --valu-per-cell the share of the 78.6 T lane-operations per second of SURVEY.md section 8(d)
  every     one query, candidates = 0, against the index of 10 000 clips of 2 320 (hpfw_gpu_search_dtw_device): ms per query
  rerank    1 000 queries of 305, candidates = 16, k = 10: ms per call
  plain     hpfw_gpu_search_topk_device for the same 1 000 queries, k = 10, as context

    python tools/time_dtw.py [--reps 5] [--valu-per-cell 17.3] [--out profiles/dtw.json]

Random hashprints: the kernel's work does not depend on the values.  Prints one JSON line and writes --out.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_IDX, PER, N_Q, KQ, K, CAND = 10_000, 2320, 1000, 305, 10, 16
PEAK_LANE_OPS = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--valu-per-cell", type=float, default=17.3,
                    help="VALU instructions per cell of the pairs kernel's row loop, counted from the disassembly (DESIGN.md section 20)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtw.json"))
    args = ap.parse_args()
    import torch
    import hpfw_amd
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    g = hpfw_amd.Gpu(0)
    rng = np.random.default_rng(77)
    db = rng.integers(0, 2 ** 64, size=N_IDX * PER, dtype=np.uint64)
    g.index_clear()
    g.index_add(db, np.arange(0, (N_IDX + 1) * PER, PER, dtype=np.int64))
    q = rng.integers(0, 2 ** 64, size=N_Q * KQ, dtype=np.uint64)
    q_off = np.arange(0, (N_Q + 1) * KQ, KQ, dtype=np.int64)
    pairs = np.stack([np.arange(N_IDX) % N_Q, np.arange(N_IDX)], 1).astype(np.int32)
    d_q = torch.from_numpy(q.view(np.int64)).cuda()
    d_pairs_out = torch.empty((N_IDX, 4), dtype=torch.int32, device="cuda")
    d_out = torch.empty((N_Q, K, 4), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream()
    calls = {
        "pairs": lambda: g.dtw_pairs_dev(d_q.data_ptr(), q_off, pairs, d_pairs_out.data_ptr(), stream=s.cuda_stream),
        "every": lambda: g.search_dtw_dev(d_q.data_ptr(), q_off[:2], K, 0, d_out.data_ptr(), stream=s.cuda_stream),
        "rerank": lambda: g.search_dtw_dev(d_q.data_ptr(), q_off, K, CAND, d_out.data_ptr(), stream=s.cuda_stream),
        "plain": lambda: g.search_topk_dev(d_q.data_ptr(), q_off, K, d_out.data_ptr(), s.cuda_stream),
    }
    names = list(calls)
    ms = {name: [] for name in names}
    for r in range(args.reps + 1):
        for name in names if r % 2 == 0 else names[::-1]:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            calls[name]()
            b.record(s)
            b.synchronize()
            if r:
                ms[name].append(a.elapsed_time(b))
    g.index_clear()
    g.close()
    med = {name: float(np.median(ms[name])) for name in names}
    cells = N_IDX * KQ * PER
    rec = {
        "what": "the warped search on one MI355X (DESIGN.md section 20; tools/time_dtw.py): device events on the stream, "
                f"one warm-up round, the median of {args.reps} rounds, the calls alternated",
        "index": f"{N_IDX} clips of {PER} random hashprints",
        "pairs": {"workload": f"{N_IDX} pairs of K = {KQ} by n = {PER}", "ms": round(med["pairs"], 3),
                  "min_max_ms": [round(min(ms["pairs"]), 3), round(max(ms["pairs"]), 3)],
                  "cells_per_s": round(cells / (med["pairs"] * 1e-3)),
                  "valu_lane_ops_per_cell": args.valu_per_cell,
                  "share_of_78.6T_lane_ops_per_s": round(args.valu_per_cell * cells / (med["pairs"] * 1e-3) / PEAK_LANE_OPS, 4)},
        "every_clip": {"workload": f"1 query of {KQ}, candidates = 0, k = {K}", "ms_per_query": round(med["every"], 3),
                       "min_max_ms": [round(min(ms["every"]), 3), round(max(ms["every"]), 3)]},
        "rerank": {"workload": f"{N_Q} queries of {KQ}, candidates = {CAND}, k = {K}", "ms": round(med["rerank"], 3),
                   "min_max_ms": [round(min(ms["rerank"]), 3), round(max(ms["rerank"]), 3)]},
        "plain": {"workload": f"hpfw_gpu_search_topk_device, the same {N_Q} queries, k = {K}", "ms": round(med["plain"], 3),
                  "min_max_ms": [round(min(ms["plain"]), 3), round(max(ms["plain"]), 3)]},
    }
    print(json.dumps(rec), flush=True)
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
