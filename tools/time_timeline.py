"""Times the timeline of a long recording (k_stats.hip, k_windows.hip) on one MI355X.

  search   the index of BASELINE.json configs[2] (10 000 clips of 30 s = 2 320 hashprints, 1 000 query slices of 5 s = 304
           hashprints, k = 10, random hashprints): hpfw_gpu_search_topk_device and hpfw_gpu_search_topk_scored_device of the
           same build ALTERNATED in one process, device events around each call (one warm-up pair, --reps pairs): medians,
           the ratio scored / plain per pair and its spread
  kernel   --reps + 1 scored searches of that workload and --reps + 1 extractions of the windows (5 s every 2.5 s) of a
           10-minute recording, for `rocprofv3 --kernel-trace --stats` in a run of its own; --stats FILE then reads
           rocprofv3's output (the rocpd SQLite database, or kernel_stats.csv with `-f csv`) and adds the device time per
           call of dist_stats_kernel against the top-k kernel's and the scan's, and gather_windows_kernel's share of the
           device time of the window extraction, to --out
  margin   the separation of the score on a larger synthetic index: 1 000 songs of 30 s indexed, the 41 windows of concert
           (A) of tests/timeline_ref.py (songs 3, 11 and 7 inside, noise and songs 21, 22 of the index now) scored

    python tools/time_timeline.py [--parts search,margin] [--reps 9] [--out profiles/timeline.json]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/time_timeline.py --parts kernel [--out ...]
    python tools/time_timeline.py --stats DIR/run_results.db [--out ...]     (no GPU: merges into --out)

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
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_IDX, PER, N_Q, KQ, K = 10_000, 2320, 1000, 304, 10
WIN, HOP, REC_S = 220500, 110250, 600


def _index(g):
    rng = np.random.default_rng(77)
    db = rng.integers(0, 2 ** 64, size=N_IDX * PER, dtype=np.uint64)
    g.index_clear()
    g.index_add(db, np.arange(0, (N_IDX + 1) * PER, PER, dtype=np.int64))
    q = rng.integers(0, 2 ** 64, size=N_Q * KQ, dtype=np.uint64)
    return q, np.arange(0, (N_Q + 1) * KQ, KQ, dtype=np.int64)


def part_search(torch, g, reps):
    q, q_off = _index(g)
    d_q = torch.from_numpy(q.view(np.int64)).cuda()
    d_out = torch.empty((N_Q, K, 4), dtype=torch.int32, device="cuda")
    d_stats = torch.empty((N_Q, 3), dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream()
    calls = {"plain": lambda: g.search_topk_dev(d_q.data_ptr(), q_off, K, d_out.data_ptr(), s.cuda_stream),
             "scored": lambda: g.search_topk_scored_dev(d_q.data_ptr(), q_off, K, d_out.data_ptr(), d_stats.data_ptr(), s.cuda_stream)}
    ms = {"plain": [], "scored": []}
    for r in range(reps + 1):
        for name in ("plain", "scored") if r % 2 == 0 else ("scored", "plain"):   # alternated, the order swapped every pair
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            calls[name]()
            b.record(s)
            b.synchronize()
            if r:
                ms[name].append(a.elapsed_time(b))
    ratio = [y / x for x, y in zip(ms["plain"], ms["scored"])]
    g.index_clear()
    return {"workload": f"{N_Q} queries of {KQ} hashprints against {N_IDX} clips of {PER}, k = {K}; the two calls alternated in one "
                        f"process, device events, {reps} pairs after one warm-up pair",
            "plain_ms": round(float(np.median(ms["plain"])), 3), "plain_min_max_ms": [round(min(ms["plain"]), 3), round(max(ms["plain"]), 3)],
            "scored_ms": round(float(np.median(ms["scored"])), 3), "scored_min_max_ms": [round(min(ms["scored"]), 3), round(max(ms["scored"]), 3)],
            "scored_over_plain": round(float(np.median(ratio)), 4), "scored_over_plain_min_max": [round(min(ratio), 4), round(max(ratio), 4)],
            "plain_run_to_run_spread": round((max(ms["plain"]) - min(ms["plain"])) / float(np.median(ms["plain"])), 4)}


def part_kernel(torch, g, reps):
    from hpfw_amd import synth
    q, q_off = _index(g)
    d_q = torch.from_numpy(q.view(np.int64)).cuda()
    d_out = torch.empty((N_Q, K, 4), dtype=torch.int32, device="cuda")
    d_stats = torch.empty((N_Q, 3), dtype=torch.int64, device="cuda")
    for _ in range(reps + 1):
        g.search_topk_scored_dev(d_q.data_ptr(), q_off, K, d_out.data_ptr(), d_stats.data_ptr())
    torch.cuda.synchronize()
    g.index_clear()
    base = np.concatenate([synth.gen_clip(700 + i, 30.0) for i in range(4)])
    x = np.tile(base, REC_S // 120)
    d_pcm = torch.from_numpy(x).cuda()
    n_w = (x.size - WIN) // HOP + 1
    d_hp = torch.empty((n_w, g.geometry(WIN).n_hp), dtype=torch.int64, device="cuda")
    for _ in range(reps + 1):
        g.extract_windows_dev(d_pcm.data_ptr(), x.size, WIN, HOP, d_hp.data_ptr())
    torch.cuda.synchronize()
    return {"calls": reps + 1, "windows": int(n_w), "recording_s": REC_S}


SEARCH_KERNELS = {"dist_stats": "dist_stats_kernel", "topk": "topk_kernel", "scan": "hamming_mfma", "expand_queries": "expand_queries"}


def merge_stats(path, rec):
    k = rec.get("kernel_run", {})
    calls = k.get("calls")
    if not calls:
        raise SystemExit("no kernel_run record in --out: run --parts kernel under rocprofv3 first (with the same --out)")
    if path.endswith(".csv"):
        with open(path) as f:
            rows = [(r["Name"], float(r["TotalDurationNs"]), int(r["Calls"])) for r in csv.DictReader(f)]
    else:
        import sqlite3
        with sqlite3.connect(path) as db:
            rows = db.execute("SELECT name, sum(duration), count(*) FROM kernels GROUP BY name").fetchall()
    out = {"source": "rocprofv3 --kernel-trace --stats, a run of its own", "calls_of_each_workload": calls, "search_ms_per_call": {}}
    for key, pat in SEARCH_KERNELS.items():
        sel = [r for r in rows if pat in r[0]]
        out["search_ms_per_call"][key] = round(sum(r[1] for r in sel) / calls / 1e6, 4)
        out["search_ms_per_call"][key + "_launches_per_call"] = sum(r[2] for r in sel) / calls
    sm = out["search_ms_per_call"]
    if not sm["dist_stats"] or not sm["topk"]:
        raise SystemExit(f"{path}: no dist_stats_kernel / topk_kernel launch")
    out["dist_stats_over_topk"] = round(sm["dist_stats"] / sm["topk"], 4)
    searching = ("dist_stats_kernel", "topk_", "hamming_", "expand_queries")
    windows = [r for r in rows if not any(p in r[0] for p in searching)]
    total = sum(r[1] for r in windows)
    gather = sum(r[1] for r in windows if "gather_windows_kernel" in r[0])
    if not gather:
        raise SystemExit(f"{path}: no gather_windows_kernel launch")
    out["windows"] = {"recording_s": k.get("recording_s"), "windows": k.get("windows"), "device_ms_per_call": round(total / calls / 1e6, 4),
                      "gather_ms_per_call": round(gather / calls / 1e6, 4), "gather_share": round(gather / total, 5)}
    return out


def part_margin(g):
    """the score's separation with 1 000 indexed songs: windows inside an indexed song against every other window"""
    from hpfw_amd import _lib, synth
    import timeline_ref as ref
    n_idx = 1000
    hp = np.concatenate([g.extract(np.stack([synth.gen_clip(i, 30.0) for i in range(c0, c0 + 50)])) for c0 in range(0, n_idx, 50)])
    g.index_clear()
    g.index_add(hp, np.arange(n_idx + 1, dtype=np.int64) * hp.shape[1])
    w_hp = g.extract_windows(ref.concert_a(), WIN, HOP)
    hits, stats = g.search_topk_scored(w_hp, np.arange(w_hp.shape[0] + 1, dtype=np.int64) * w_hp.shape[1], 1)
    g.index_clear()
    score = [_lib.hit_score(h["dist"], True, s) for h, s in zip(hits[:, 0], stats)]
    # windows with at least 4.5 s of one song that can be aligned (window 23 holds 4.5 s of song 21 from its first sample, behind
    # 0.5 s of song 11: its offset would be negative, so it is no match)
    inside = {3: range(0, 8), 11: range(12, 22), 21: range(24, 30), 7: range(31, 36), 22: range(37, 41)}
    in_song = [score[w] for c, ws in inside.items() for w in ws]
    right = all(int(hits[w, 0]["clip"]) == c for c, ws in inside.items() for w in ws)
    rest = [score[w] for w in range(len(score)) if not any(w in ws for ws in inside.values())]
    return {"index": f"{n_idx} songs of 30 s (hpfw_amd.synth.gen_clip), fixture filters; concert (A) of tests/timeline_ref.py, whose songs "
                     "21 and 22 are in this index", "windows_inside_an_indexed_song": len(in_song),
            "noise_only_windows_9_to_11": [round(score[w], 2) for w in (9, 10, 11)], "their_clip_is_right": right,
            "score_inside_min_max": [round(min(in_song), 2), round(max(in_song), 2)],
            "score_elsewhere_min_max": [round(min(rest), 2), round(max(rest), 2)],
            "elsewhere": "windows of noise (9-11) and windows straddling two parts (8, 22, 23, 30, 36)",
            "scores": [round(x, 2) for x in score]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="search,margin")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timeline.json"))
    args = ap.parse_args()
    rec = {}
    if os.path.exists(args.out) and os.path.getsize(args.out):
        with open(args.out) as f:
            rec = json.load(f)
    rec["what"] = "the timeline of a long recording on one MI355X (DESIGN.md section 13; tools/time_timeline.py)"
    if args.stats is not None:
        rec["kernels"] = merge_stats(args.stats, rec)
        print(json.dumps(rec["kernels"]))
    else:
        import torch
        import hpfw_amd
        from hpfw_amd import synth
        g = hpfw_amd.Gpu(0)
        g.set_filters(synth.make_filters())
        for part in args.parts.split(","):
            res = part_margin(g) if part == "margin" else {"search": part_search, "kernel": part_kernel}[part](torch, g, args.reps)
            rec[{"search": "search_1000q_10000clips", "kernel": "kernel_run", "margin": "score_margin_1000_songs"}[part]] = res
            print(json.dumps({part: res}), flush=True)
        g.close()
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
