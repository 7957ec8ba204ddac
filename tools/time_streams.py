"""Times live feeds (k_streams.hip, streams.hip) on one MI355X: what cutting windows out of feeds costs.

  ticks    the index of BASELINE.json configs[2] (10 000 clips of 2 320 random hashprints) plus 20 synthetic songs of 30 s;
           1 and 32 feeds, each a loop over songs of the index; a tick delivers one hop (2.5 s) per feed from host memory and
           is push -> extract -> scored search (k = 1) -> hits and moments on the host.  ALTERNATED in the same process, tick
           by tick and with the order swapped every tick, with the yardstick: the same windows already resident on the device
           through the unchanged extract_dev + search_topk_scored_dev, hits and moments to the host (the pattern of bench.py's
           streaming section).  Host wall clock per tick: medians, min / max, and the difference per tick, which is the cost
           of cutting the windows out of feeds (upload, ring_append_kernel, ring_gather_windows_kernel, bookkeeping).  The
           hashprints of both sides are compared on every tick.
  kernel   --reps ticks of 32 feeds through the streams alone, on an index of random hashprints (no other extraction runs
           in the process), for `rocprofv3 --kernel-trace --stats` in a run of its own; --stats FILE then reads rocprofv3's
           output (the rocpd SQLite database, or kernel_stats.csv with `-f csv`) and adds the two kernels' time per tick and
           their share of the tick's kernel time to --out

    python tools/time_streams.py [--parts ticks] [--reps 40] [--out profiles/streams.json]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/time_streams.py --parts kernel [--out ...]
    python tools/time_streams.py --stats DIR/run_results.db [--out ...]     (no GPU: merges into --out)

Prints one JSON line per part and merges the parts into --out.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_IDX, PER, N_SONGS = 10_000, 2320, 20
WIN, HOP = 220500, 110250
WARM = 3                                                   # ticks before the first timed one (the first window needs two)


def _index(g, songs_hp=None):
    rng = np.random.default_rng(77)
    db = rng.integers(0, 2 ** 64, size=N_IDX * PER, dtype=np.uint64)
    g.index_clear()
    g.index_add(db, np.arange(0, (N_IDX + 1) * PER, PER, dtype=np.int64))
    if songs_hp is not None:
        g.index_add(songs_hp, np.arange(songs_hp.shape[0] + 1, dtype=np.int64) * songs_hp.shape[1])


def _feeds(n_feeds, ticks, songs):
    """feed i: the songs in turn from song i on, at half gain, long enough for `ticks` hops"""
    need = (ticks + 2) * HOP
    out = []
    for i in range(n_feeds):
        parts, k = [], i
        while sum(p.size for p in parts) < need:
            parts.append((songs[k % len(songs)] // 2).astype(np.int16))
            k += 1
        out.append(np.concatenate(parts)[:need])
    return out


class Tick:
    """the buffers of one configuration and its two ways through a tick"""

    def __init__(self, torch, g, n_feeds):
        self.torch, self.g, self.n = torch, g, n_feeds
        self.s = g.streams(n_feeds, WIN, HOP)
        nhp = g.geometry(WIN).n_hp
        self.q_off = np.arange(n_feeds + 1, dtype=np.int64) * nhp
        mk = lambda *shape, dt=torch.int64: torch.empty(shape, dtype=dt, device="cuda")
        self.hp_a, self.hp_b = mk(n_feeds, nhp), mk(n_feeds, nhp)
        self.hits, self.stats = mk(n_feeds, 1, 4, dt=torch.int32), mk(n_feeds, 3)
        self.resident = mk(n_feeds, WIN, dt=torch.int16)

    def _search(self, d_hp):
        self.g.search_topk_scored_dev(d_hp.data_ptr(), self.q_off, 1, self.hits.data_ptr(), self.stats.data_ptr())
        return self.hits.cpu(), self.stats.cpu()               # (the copies wait for the null stream)

    def streams(self, chunks):
        t0 = time.perf_counter()
        ready = self.s.push(chunks)
        if ready:
            which = self.s.extract_dev(ready, self.hp_a.data_ptr())
            assert which.size == self.n
            self._search(self.hp_a)
        return (time.perf_counter() - t0) * 1e3, ready

    def yardstick(self):
        t0 = time.perf_counter()
        self.g.extract_dev(self.resident.data_ptr(), WIN, self.n, self.hp_b.data_ptr())
        self._search(self.hp_b)
        return (time.perf_counter() - t0) * 1e3

    def close(self):
        self.s.close()


def _summary(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_max_ms": [round(min(ms), 3), round(max(ms), 3)]}


def part_ticks(torch, g, reps):
    from hpfw_amd import synth
    songs = [synth.gen_clip(i, 30.0) for i in range(N_SONGS)]
    _index(g, g.extract(np.stack(songs)))
    out = {"workload": f"{N_IDX} clips of {PER} random hashprints plus {N_SONGS} songs of 30 s; windows of 5 s every 2.5 s; a tick "
                       f"delivers one hop per feed from host memory; {reps} timed ticks after {WARM}, the two ways alternated tick by "
                       "tick in one process, host wall clock"}
    for n_feeds in (1, 32):
        feeds = _feeds(n_feeds, reps + WARM, songs)
        t = Tick(torch, g, n_feeds)
        a, b, found = [], [], 0
        for tick in range(reps + WARM):
            chunks = [x[tick * HOP:(tick + 1) * HOP] for x in feeds]
            if tick >= 1:                                     # the windows this tick completes, resident before the clock runs
                w = np.stack([x[(tick - 1) * HOP:(tick - 1) * HOP + WIN] for x in feeds])
                t.resident.copy_(torch.from_numpy(w))
            torch.cuda.synchronize()
            order = ("streams", "yardstick") if tick % 2 == 0 else ("yardstick", "streams")
            for name in order:
                if name == "streams":
                    ms_a, ready = t.streams(chunks)
                    assert ready == (n_feeds if tick >= 1 else 0)
                elif tick >= 1:
                    ms_b = t.yardstick()
            if tick >= 1:
                assert torch.equal(t.hp_a, t.hp_b), tick        # the same windows, the same hashprints
                found += int((t.hits.cpu().numpy()[:, 0, 1] >= N_IDX).sum())
            if tick >= WARM:
                a.append(ms_a)
                b.append(ms_b)
        t.close()
        diff = [x - y for x, y in zip(a, b)]
        out[f"feeds_{n_feeds}"] = {"streams_tick": _summary(a), "resident_windows_tick": _summary(b), "difference_per_tick": _summary(diff),
                                   "difference_of_medians_ms": round(float(np.median(a) - np.median(b)), 3),
                                   "uploaded_bytes_per_tick": n_feeds * HOP * 2,
                                   "windows_whose_best_clip_is_a_song": f"{found} of {(reps + WARM - 1) * n_feeds}"}
    g.index_clear()
    return out


def part_kernel(torch, g, reps):
    _index(g)
    rng = np.random.default_rng(5)
    n_feeds = 32
    feeds = [rng.integers(-3000, 3000, (reps + 2) * HOP).astype(np.int16) for _ in range(n_feeds)]
    t = Tick(torch, g, n_feeds)
    for tick in range(reps):
        t.streams([x[tick * HOP:(tick + 1) * HOP] for x in feeds])
    torch.cuda.synchronize()
    t.close()
    g.index_clear()
    return {"ticks": reps, "ticks_with_windows": reps - 1, "feeds": n_feeds}


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
    out = {"source": "rocprofv3 --kernel-trace --stats, a run of its own", "feeds": k.get("feeds"), "ticks": ticks,
           "kernel_ms_per_tick": round(total / ticks / 1e6, 4)}
    for key in ("ring_append_kernel", "ring_gather_windows_kernel"):
        sel = [r for r in rows if key in r[0]]
        if not sel:
            raise SystemExit(f"{path}: no {key} launch")
        out[key] = {"launches": sum(r[2] for r in sel), "ms_per_tick": round(sum(r[1] for r in sel) / ticks / 1e6, 5),
                    "share_of_kernel_time": round(sum(r[1] for r in sel) / total, 5)}
    out["both_share_of_kernel_time"] = round(out["ring_append_kernel"]["share_of_kernel_time"] +
                                             out["ring_gather_windows_kernel"]["share_of_kernel_time"], 5)
    scan = sum(r[1] for r in rows if "hamming_" in r[0])
    out["scan_share_of_kernel_time"] = round(scan / total, 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ticks")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "streams.json"))
    args = ap.parse_args()
    rec = {}
    if os.path.exists(args.out) and os.path.getsize(args.out):
        with open(args.out) as f:
            rec = json.load(f)
    rec["what"] = "live feeds on one MI355X (DESIGN.md section 14; tools/time_streams.py)"
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
