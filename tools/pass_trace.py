"""pass_trace.py -- the pass boundaries of the extraction in a kernel trace of bench.py's workload.

  rocprofv3 --kernel-trace --stats -d DIR -o t --output-format csv -- python bench.py --gpus 1 --steps 10 --warmup 3 --no-parity
  python tools/pass_trace.py DIR [out.json [step.csv]]     (step.csv: the launches of one step in the middle of the run)

From the dispatch timestamps, per front-end pass (one launch of every chirp-z class, the launches of a class taken in
order): `tail` = from the end of cq_kernel<6144> to the end of the later of <8192> / <12288> (the time in which only
the two largest classes are resident), `gap` = from the last chirp-z end to the first forward column launch that
starts after it (passes followed by the hashprint kernel have none), `fwd_under_cq` = how much of the next pass's
forward launches lies before the last chirp-z end (0 where the passes are joined).  The step is the distance between
the ends of consecutive hashprint kernels.  Launches of other grids than a kernel's most frequent one are left out.
"""
import collections
import csv
import glob
import json
import os
import statistics
import sys


def load(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {d}")
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                grid = (r.get("Grid_Size_X") or r.get("Grid_Size") or "", r.get("Grid_Size_Y") or "", r.get("Grid_Size_Z") or "")
                rows.append((r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]), grid, r.get("Queue_Id", ""), r.get("Stream_Id", "")))
    return rows


def write_step(rows, hp, path):
    """the launches of one step in the middle of the run (from the end of a hashprint kernel to the end of the next), times
    in microseconds from its first launch"""
    if len(hp) < 3:
        return
    a, b = hp[len(hp) // 2 - 1][2], hp[len(hp) // 2][2]
    mine = sorted((r for r in rows if a <= r[1] and r[2] <= b), key=lambda r: r[1])
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["kernel", "queue", "stream", "start_us", "end_us", "grid_x"])
        for r in mine:
            w.writerow([r[0][:40], r[4], r[5], round((r[1] - mine[0][1]) / 1e3, 1), round((r[2] - mine[0][1]) / 1e3, 1), r[3][0]])


def modal(rows, key):
    """the launches whose name holds `key`, of the most frequent (name, grid) among them, by start"""
    mine = [r for r in rows if key in r[0]]
    if not mine:
        return []
    top = collections.Counter((r[0], r[3]) for r in mine).most_common(1)[0][0]
    return sorted((r for r in mine if (r[0], r[3]) == top), key=lambda r: r[1])


def med(v):
    return round(statistics.median(v) / 1e3, 1) if v else None


def main():
    rows = load(sys.argv[1])
    cls = {k: modal(rows, f"cq_kernel<{k}") for k in (3072, 4096, 6144, 8192, 12288)}
    n = min(len(v) for v in cls.values())
    if n == 0:
        raise SystemExit("a chirp-z class has no launch in the trace")
    hp = modal(rows, "hashprint_q")
    cols = sorted((r for r in rows if "fwd_cols" in r[0]), key=lambda r: r[1])
    fwd = sorted((r for r in rows if "fwd_cols" in r[0] or "fwd_rows" in r[0]), key=lambda r: r[1])
    steps = [b[2] - a[2] for a, b in zip(hp, hp[1:])]
    step_ns = statistics.median(steps) if steps else 0
    steps = [s for s in steps if s < 2 * step_ns]  # (the distance across bench.py's sections is no step)
    tails, gaps, under, spans = [], [], [], []
    for i in range(n):
        first = min(cls[k][i][1] for k in cls)
        last = max(cls[k][i][2] for k in cls)
        spans.append(last - first)
        tails.append(max(0, max(cls[8192][i][2], cls[12288][i][2]) - cls[6144][i][2]))
        nxt = min(cls[k][i + 1][1] for k in cls) if i + 1 < n else None
        between = [r for r in fwd if r[1] >= first and (nxt is None or r[1] < nxt)]
        hp_next = next((r[1] for r in hp if r[1] >= first), None)
        between = [r for r in between if hp_next is None or r[1] < hp_next]
        if not between:
            continue  # the group's last pass: the hashprint kernel follows
        under.append(sum(max(0, min(r[2], last) - r[1]) for r in between))
        later = [r[1] for r in cols if r[1] >= last and (hp_next is None or r[1] < hp_next)]
        if later and not any(r[1] < last for r in between):
            gaps.append(later[0] - last)
    passes_per_step = round(n / max(len(hp), 1))
    per_step = (statistics.median(tails) * passes_per_step + (statistics.median(gaps) if gaps else 0) * max(passes_per_step - 1, 0))
    out = {"passes": n, "passes_per_step": passes_per_step, "step_us": med(steps), "steps_seen": len(steps),
           "cq_span_us": med(spans), "tail_us": med(tails), "tail_range_us": [round(min(tails) / 1e3, 1), round(max(tails) / 1e3, 1)],
           "gap_us": med(gaps), "gaps_seen": len(gaps), "fwd_under_cq_us": med(under),
           "tail_and_gap_per_step_us": round(per_step / 1e3, 1), "share_of_step": round(per_step / step_ns, 4) if step_ns else None,
           "class_us": {str(k): med([r[2] - r[1] for r in v]) for k, v in cls.items()},
           "hashprint_us": med([r[2] - r[1] for r in hp])}
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as fh:
            json.dump(out, fh, indent=1)
    if len(sys.argv) > 3:
        write_step(rows, hp, sys.argv[3])


if __name__ == "__main__":
    main()
