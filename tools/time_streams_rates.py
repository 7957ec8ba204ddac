"""Times live feeds at 48 kHz (k_streams_resample.hip) on one MI355X against the same feeds at 44.1 kHz.

  ticks    the index of BASELINE.json configs[2] (10 000 clips of 2 320 random hashprints) plus 20 synthetic songs of 30 s;
           32 feeds, each a loop over songs of the index, once as they are (44.1 kHz) and once converted to 48 kHz on the host
           (scipy's resample_poly).  A tick delivers one hop (2.5 s: 110 250 samples at 44.1 kHz, 120 000 at 48 kHz) per feed
           from host memory and is push -> extract -> scored search (k = 1) -> hits and moments on the host.  The 48 kHz tick
           (one ring_resample_append_kernel launch) is ALTERNATED in the same process, tick by tick and with the order swapped
           every tick, with the yardstick: the tick of the same audio at 44.1 kHz through the unchanged path (one
           ring_append_kernel launch).  Host wall clock per tick: medians, min / max, the difference per tick, and how much of
           it the larger upload is: the difference between pinned host-to-device copies of the two ticks' bytes, timed in the
           same process.
  kernel   --reps ticks of 32 feeds at 48 kHz through the streams alone, on an index of random hashprints, for
           `rocprofv3 --kernel-trace --stats` in a run of its own; --stats FILE then reads rocprofv3's output (the rocpd SQLite
           database, or kernel_stats.csv with `-f csv`) and adds the time per tick of ring_resample_append_kernel and
           ring_gather_windows_kernel and their share of the tick's kernel time to --out

    python tools/time_streams_rates.py [--parts ticks] [--reps 40] [--out profiles/streams_rates.json]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/time_streams_rates.py --parts kernel [--out ...]
    python tools/time_streams_rates.py --stats DIR/run_results.db [--out ...]     (no GPU: merges into --out)

Not measured here: sets of mixed rates (one more launch per distinct rate), more than 32 feeds, the device form of the push,
real feeds.  Prints one JSON line per part and merges the parts into --out.
"""
import argparse
import csv
import json
import os
import sys
import time
from math import gcd

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_streams as ts  # noqa: E402  (the index, the feeds and the summary of the 44.1 kHz measurement)

RATE, N_FEEDS = 48000, 32
WIN, HOP = ts.WIN, ts.HOP
HOP_IN = HOP * RATE // 44100                                # 120 000
WARM = 3


def _at_rate(x44, fs):
    from scipy.signal import resample_poly
    g = gcd(44100, fs)
    return np.clip(np.round(resample_poly(x44.astype(np.float64), fs // g, 44100 // g)), -32768, 32767).astype(np.int16)


class Tick:
    """one set of feeds at one rate and its way through a tick"""

    def __init__(self, torch, g, n_feeds, rate):
        self.g, self.n = g, n_feeds
        self.s = g.streams(n_feeds, WIN, HOP, rates=None if rate == 44100 else rate)
        nhp = g.geometry(WIN).n_hp
        self.q_off = np.arange(n_feeds + 1, dtype=np.int64) * nhp
        mk = lambda *shape, dt=torch.int64: torch.empty(shape, dtype=dt, device="cuda")
        self.hp, self.hits, self.stats = mk(n_feeds, nhp), mk(n_feeds, 1, 4, dt=torch.int32), mk(n_feeds, 3)

    def tick(self, chunks):
        t0 = time.perf_counter()
        ready = self.s.push(chunks)
        if ready:
            which = self.s.extract_dev(ready, self.hp.data_ptr())
            assert which.size == self.n
            self.g.search_topk_scored_dev(self.hp.data_ptr(), self.q_off, 1, self.hits.data_ptr(), self.stats.data_ptr())
            self.hits.cpu(), self.stats.cpu()                  # (the copies wait for the null stream)
        return (time.perf_counter() - t0) * 1e3, ready

    def close(self):
        self.s.close()


def _upload_ms(torch, n_bytes, reps):
    src = torch.empty(n_bytes, dtype=torch.uint8).pin_memory()
    dst = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    ms = []
    for _ in range(reps + WARM):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms[WARM:]


def part_ticks(torch, g, reps):
    from hpfw_amd import synth
    songs = [synth.gen_clip(i, 30.0) for i in range(ts.N_SONGS)]
    ts._index(g, g.extract(np.stack(songs)))
    n_ticks = reps + WARM
    feeds44 = ts._feeds(N_FEEDS, n_ticks, songs)
    feeds48 = [_at_rate(x, RATE) for x in feeds44]
    a, b = Tick(torch, g, N_FEEDS, RATE), Tick(torch, g, N_FEEDS, 44100)
    ms48, ms44, found = [], [], [0, 0]
    for tick in range(n_ticks):
        c48 = [x[tick * HOP_IN:(tick + 1) * HOP_IN] for x in feeds48]
        c44 = [x[tick * HOP:(tick + 1) * HOP] for x in feeds44]
        torch.cuda.synchronize()
        for name in (("48", "44") if tick % 2 == 0 else ("44", "48")):
            t, chunks = (a, c48) if name == "48" else (b, c44)
            ms, ready = t.tick(chunks)
            # the 48 kHz feed gives its outputs H inputs late: its window w is complete one tick after the 44.1 kHz feed's
            assert ready == (N_FEEDS if tick >= (2 if name == "48" else 1) else 0), (name, tick, ready)
            if ready:
                found[name == "44"] += int((t.hits.cpu().numpy()[:, 0, 1] >= ts.N_IDX).sum())
            if tick >= WARM:
                (ms48 if name == "48" else ms44).append(ms)
    a.close()
    b.close()
    up48, up44 = _upload_ms(torch, N_FEEDS * HOP_IN * 2, reps), _upload_ms(torch, N_FEEDS * HOP * 2, reps)
    diff = [x - y for x, y in zip(ms48, ms44)]
    out = {"workload": f"{ts.N_IDX} clips of {ts.PER} random hashprints plus {ts.N_SONGS} songs of 30 s; {N_FEEDS} feeds, windows of 5 s every "
                       f"2.5 s; a tick delivers 2.5 s per feed from host memory; {reps} timed ticks after {WARM}, the 48 kHz and the 44.1 kHz "
                       "tick of the same audio alternated tick by tick in one process, host wall clock",
           "tick_48000": ts._summary(ms48), "tick_44100": ts._summary(ms44), "difference_per_tick": ts._summary(diff),
           "difference_of_medians_ms": round(float(np.median(ms48) - np.median(ms44)), 3),
           "uploaded_bytes_per_tick": {"48000": N_FEEDS * HOP_IN * 2, "44100": N_FEEDS * HOP * 2},
           "pinned_upload_alone": {"48000": ts._summary(up48), "44100": ts._summary(up44),
                                   "difference_of_medians_ms": round(float(np.median(up48) - np.median(up44)), 3)},
           "windows_whose_best_clip_is_a_song": {"48000": f"{found[0]} of {(n_ticks - 2) * N_FEEDS}", "44100": f"{found[1]} of {(n_ticks - 1) * N_FEEDS}"}}
    g.index_clear()
    return out


def part_kernel(torch, g, reps):
    ts._index(g)
    rng = np.random.default_rng(5)
    feeds = [rng.integers(-3000, 3000, (reps + 2) * HOP_IN).astype(np.int16) for _ in range(N_FEEDS)]
    t = Tick(torch, g, N_FEEDS, RATE)
    with_windows = 0
    for tick in range(reps):
        with_windows += t.tick([x[tick * HOP_IN:(tick + 1) * HOP_IN] for x in feeds])[1] > 0
    torch.cuda.synchronize()
    t.close()
    g.index_clear()
    return {"ticks": reps, "ticks_with_windows": int(with_windows), "feeds": N_FEEDS, "rate": RATE}


def merge_stats(path, rec):
    k = rec.get("kernel_run", {})
    ticks = k.get("ticks")
    if not ticks:
        raise SystemExit("no kernel_run record in --out: run --parts kernel under rocprofv3 first (with the same --out)")
    if path.endswith(".csv"):
        with open(path) as f:
            rows = [(r["Name"], float(r["TotalDurationNs"]), int(r["Calls"])) for r in csv.DictReader(f)]
    else:
        import sqlite3
        with sqlite3.connect(path) as db:
            rows = db.execute("SELECT name, sum(duration), count(*) FROM kernels GROUP BY name").fetchall()
    total = sum(r[1] for r in rows)
    out = {"source": "rocprofv3 --kernel-trace --stats, a run of its own", "feeds": k.get("feeds"), "rate": k.get("rate"), "ticks": ticks,
           "kernel_ms_per_tick": round(total / ticks / 1e6, 4)}
    for key in ("ring_resample_append_kernel", "ring_gather_windows_kernel"):
        sel = [r for r in rows if key in r[0]]
        if not sel:
            raise SystemExit(f"{path}: no {key} launch")
        out[key] = {"launches": sum(r[2] for r in sel), "ms_per_tick": round(sum(r[1] for r in sel) / ticks / 1e6, 5),
                    "share_of_kernel_time": round(sum(r[1] for r in sel) / total, 5)}
    out["both_share_of_kernel_time"] = round(out["ring_resample_append_kernel"]["share_of_kernel_time"] +
                                             out["ring_gather_windows_kernel"]["share_of_kernel_time"], 5)
    out["ring_append_kernel_launches"] = sum(r[2] for r in rows if "ring_append_kernel" in r[0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ticks")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "streams_rates.json"))
    args = ap.parse_args()
    rec = {}
    if os.path.exists(args.out) and os.path.getsize(args.out):
        with open(args.out) as f:
            rec = json.load(f)
    rec["what"] = "live feeds at 48 kHz against 44.1 kHz on one MI355X (DESIGN.md section 14; tools/time_streams_rates.py)"
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
            res = {"ticks": part_ticks, "kernel": part_kernel}[part](torch, g, args.reps)
            rec[{"ticks": "ticks_10000_clips", "kernel": "kernel_run"}[part]] = res
            print(json.dumps({part: res}), flush=True)
        g.close()
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
