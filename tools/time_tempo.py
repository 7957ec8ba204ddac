"""Times the tempo query (k_tempo.hip) on one MI355X.

  extract  1 000 x 5 s clips from PCM (device buffers): plain extraction, tempos [0.92, 0.96, 1, 1.04, 1.08], and those
           tempos x shifts {-4, -2, 0, 2, 4}; device events around each call (one warm-up, median of --reps), and the
           device time of the projection launches (hpfw_gpu_set_kernel_timing, kind project_mfma)
  kernel   only the tempo extraction of the same workload, --reps + 1 calls, for `rocprofv3 --kernel-trace --stats` in a
           run of its own; --stats FILE then reads rocprofv3's output (the rocpd SQLite database, or kernel_stats.csv with
           `-f csv`) and adds tempo_scale_kernel's time per call and its achieved bandwidth on the compulsory bytes (S read
           once, R 121 c_t 4 bytes written per clip) to --out
  search   200 queries x V sets (V = 1, 5, 25; 271 hashprints each, a 5 s query at the common length of the tempos above)
           against 10 000 indexed clips of 2 320 hashprints through hpfw_gpu_search_topk_transposed_device
  top1     the identification corpus of tests/test_gpu_tempo.py (32 songs of 30 s, 8 queries of 5 s at tempo 0.92 to
           1.08, 10 dB SNR): top-1 hits without and with tempos

    python tools/time_tempo.py [--parts extract,search,top1] [--reps 5] [--out profiles/tempo.json]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/time_tempo.py --parts kernel [--out ...]
    python tools/time_tempo.py --stats DIR/run_results.db [--out ...]     (no GPU: merges into --out)

Prints one JSON line per part and merges the parts into --out.
"""
import argparse
import csv
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TEMPOS = [0.92, 0.96, 1.0, 1.04, 1.08]
SHIFTS = [-4, -2, 0, 2, 4]
N_CLIPS, N_SAMPLES = 1000, 220500


def _clips(torch):
    from hpfw_amd import synth
    base = np.stack([synth.gen_clip(i, 5.0) for i in range(8)])
    return torch.from_numpy(np.ascontiguousarray(base[np.arange(N_CLIPS) % 8])).cuda()


def _timed(torch, g, fn, reps):
    s = torch.cuda.current_stream()
    ms, proj = [], []
    for r in range(reps + 1):
        g.set_kernel_timing(1 << 4)                                  # project_mfma
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn(s.cuda_stream)
        b.record(s)
        b.synchronize()
        if r:
            ms.append(a.elapsed_time(b))
            proj.append(g.kernel_timing().get("project_mfma", (0.0, 0))[0])
    g.set_kernel_timing(0)
    return {"ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "project_ms": round(float(np.median(proj)), 3)}


def part_extract(torch, g, reps):
    from hpfw_amd import _lib
    d_pcm = _clips(torch)
    geo = g.geometry(N_SAMPLES)
    ct = _lib.tempo_columns(geo.c, TEMPOS)
    out = {"workload": f"{N_CLIPS} x 5 s clips (8 clips of hpfw_amd.synth.gen_clip repeated) from device PCM; device events "
                       f"around each call, median of {reps} after one warm-up",
           "columns": int(geo.c), "common_columns": int(ct), "hashprints_plain": int(geo.n_hp), "hashprints_tempo": int(ct - 99)}
    hp = torch.empty((N_CLIPS, geo.n_hp), dtype=torch.int64, device="cuda")
    out["plain"] = _timed(torch, g, lambda st: g.extract_dev(d_pcm.data_ptr(), N_SAMPLES, N_CLIPS, hp.data_ptr(), st), reps)
    for name, shifts in (("tempos5", None), ("tempos5_x_shifts5", SHIFTS)):
        V = len(TEMPOS) * (len(shifts) if shifts else 1)
        hpt = torch.empty((N_CLIPS, V, ct - 99), dtype=torch.int64, device="cuda")
        r = _timed(torch, g, lambda st: g.extract_tempo_dev(d_pcm.data_ptr(), N_SAMPLES, N_CLIPS, TEMPOS, hpt.data_ptr(), shifts, st),
                   reps)
        r["variants"] = V
        r["over_plain"] = round(r["ms"] / out["plain"]["ms"], 3)
        r["project_over_V_plain_projections"] = round(r["project_ms"] / (V * out["plain"]["project_ms"]), 3)
        out[name] = r
        del hpt
    return out


def part_kernel(torch, g, reps):
    d_pcm = _clips(torch)
    geo = g.geometry(N_SAMPLES)
    from hpfw_amd import _lib
    ct = _lib.tempo_columns(geo.c, TEMPOS)
    hpt = torch.empty((N_CLIPS, len(TEMPOS), ct - 99), dtype=torch.int64, device="cuda")
    for _ in range(reps + 1):
        g.extract_tempo_dev(d_pcm.data_ptr(), N_SAMPLES, N_CLIPS, TEMPOS, hpt.data_ptr())
    torch.cuda.synchronize()
    return {"calls": reps + 1, "columns": int(geo.c), "common_columns": int(ct)}


def merge_stats(path, rec):
    """tempo_scale_kernel's line of rocprofv3's kernel stats -> time per extraction call and bandwidth"""
    k = rec.get("kernel_run", {})
    calls, c, ct = k.get("calls"), k.get("columns"), k.get("common_columns")
    if not calls:
        raise SystemExit("no kernel_run record in --out: run --parts kernel under rocprofv3 first (with the same --out)")
    if path.endswith(".csv"):
        with open(path) as f:
            rows = [r for r in csv.DictReader(f) if "tempo_scale_kernel" in r["Name"]]
        total_ns, launches = sum(float(r["TotalDurationNs"]) for r in rows), sum(int(r["Calls"]) for r in rows)
    else:
        import sqlite3
        with sqlite3.connect(path) as db:
            launches, total_ns = db.execute("SELECT count(*), sum(duration) FROM kernels WHERE name LIKE '%tempo_scale_kernel%'").fetchone()
    if not launches:
        raise SystemExit(f"{path}: no tempo_scale_kernel launch")
    per_call_ms = total_ns / calls / 1e6
    bytes_ = N_CLIPS * (121 * c * 4 + len(TEMPOS) * 121 * ct * 4)
    return {"source": "rocprofv3 --kernel-trace --stats, a run of its own", "launches": launches, "extraction_calls": calls,
            "ms_per_call": round(per_call_ms, 4), "compulsory_GB": round(bytes_ / 1e9, 4),
            "achieved_TBps": round(bytes_ / (per_call_ms * 1e-3) / 1e12, 3), "hbm_peak_TBps": 8.0,
            "fraction_of_peak": round(bytes_ / (per_call_ms * 1e-3) / 8.0e12, 3), "target_fraction": 0.4}


def part_search(torch, g, reps):
    from hpfw_amd import _lib
    rng = np.random.default_rng(77)
    n_idx, per, n_q, kq, k = 10_000, 2320, 200, 271, 10
    db = rng.integers(0, 2 ** 64, size=n_idx * per, dtype=np.uint64)
    off = np.arange(0, (n_idx + 1) * per, per, dtype=np.int64)
    g.index_clear()
    g.index_add(db, off)
    out = {"workload": f"{n_q} queries x V sets of {kq} hashprints against {n_idx} clips of {per}, k = {k}; device events, median "
                       f"of {reps} after one warm-up"}
    for V in (1, 5, 25):
        q = rng.integers(0, 2 ** 64, size=n_q * V * kq, dtype=np.uint64)
        q_off = np.arange(0, (n_q * V + 1) * kq, kq, dtype=np.int64)
        d_q = torch.from_numpy(q.view(np.int64)).cuda()
        d_out = torch.empty((n_q, k, 4), dtype=torch.int32, device="cuda")
        r = _timed(torch, g, lambda st: g.search_topk_transposed_dev(d_q.data_ptr(), q_off, V, k, d_out.data_ptr(), st), reps)
        r.pop("project_ms")
        out[f"V{V}"] = r
    for V in (5, 25):
        out[f"V{V}"]["over_V_times_V1"] = round(out[f"V{V}"]["ms"] / (V * out["V1"]["ms"]), 3)
    g.index_clear()
    return out


def part_top1():
    import hpfw_amd
    from hpfw_amd import synth
    import tempo_ref
    work = tempfile.mkdtemp(prefix="time_tempo_")
    n_idx = 32
    paths = []
    for c in range(n_idx):
        p = os.path.join(work, f"song{c:02d}.wav")
        synth.write_wav(p, synth.gen_clip(c, 30.0))
        paths.append(p)
    queries, truth = [], []
    for q in range(8):
        rho = (0.92, 0.96, 1.04, 1.08)[q % 4]
        c = (5 * q + 3) % n_idx
        src = [None] * n_idx
        src[c] = tempo_ref.gen_clip(c, 30.0, tempo=rho)
        pcm, ci, _ = synth.gen_query(src, c)
        p = os.path.join(work, f"q{q}_song{ci:02d}.wav")
        synth.write_wav(p, pcm)
        queries.append(p)
        truth.append(f"song{ci:02d}")
    lsi = hpfw_amd.LiveSongIdentification()
    try:
        lsi.index(paths)
        plain = lsi.top(queries, 1)
        tempo = lsi.top(queries, 1, tempos=TEMPOS)
    finally:
        lsi._gpu.close()
    return {"corpus": "32 songs of 30 s, 8 queries of 5 s at tempo 0.92, 0.96, 1.04, 1.08 (two each), 10 dB SNR",
            "top1_without_tempos": sum(bool(r) and r[0][1] == t for (_, r), t in zip(plain, truth)),
            "top1_with_tempos": sum(bool(r) and r[0][1] == t for (_, r), t in zip(tempo, truth)), "queries": len(queries)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="extract,search,top1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tempo.json"))
    args = ap.parse_args()
    rec = {}
    if os.path.exists(args.out) and os.path.getsize(args.out):
        with open(args.out) as f:
            rec = json.load(f)
    rec["what"] = "queries at another tempo on one MI355X (DESIGN.md section 12; tools/time_tempo.py)"
    if args.stats is not None:
        rec["tempo_scale_kernel"] = merge_stats(args.stats, rec)
        print(json.dumps(rec["tempo_scale_kernel"]))
    else:
        import torch
        import hpfw_amd
        from hpfw_amd import synth
        g = hpfw_amd.Gpu(0)
        g.set_filters(synth.make_filters())
        for part in args.parts.split(","):
            if part == "top1":
                res = part_top1()
            else:
                res = {"extract": part_extract, "kernel": part_kernel, "search": part_search}[part](torch, g, args.reps)
            rec[{"extract": "extract_1000x5s", "kernel": "kernel_run", "search": "search_200q_10000clips"}.get(part, part)] = res
            print(json.dumps({part: res}), flush=True)
        g.close()
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
