"""Times removal from the index in place (k_index.hip) on one MI355X, and what a caller had to do before
it existed.

  --mode remove    hpfw_gpu_index_remove: device events on the stream around the call, one warm-up round, the median of --reps
                   rounds, the index rebuilt from a device copy between rounds.  Per row the bytes the plan moves, the time, the
                   achieved rate (bytes moved / time), and the same number of bytes as ONE device-to-device hipMemcpyAsync (a
                   contiguous Tensor.copy_) between two other buffers in the same run: the runtime's copy, not this code.  A staged chunk reads and writes every byte twice,
                   so about half that rate is what the design predicts; the ratio is reported, it is not a gate.
  --mode rebuild   the baseline: index_get, filter on the host, index_clear, index_add, host clock around the four (the caller
                   waits for all of them).  Uses only entry points older than the removal, so it runs against a library built from
                   an earlier commit: HPFW_TREE=<that commit's checkout, built>.

Indexes: 10 000 x 2 320 hashprints (the benchmark's) and, with --large, 1 000 000 x 2 320.  Removals: one clip at the front, 1 %
of the clips at random, every other clip.  --stage-mb a,b,c repeats the large front removal at those chunk sizes
(HPFW_INDEX_STAGE_MB), which is how the default chunk was chosen.

    python tools/time_index_remove.py --mode remove [--large] [--reps 5] [--stage-mb 4,8,16,32,64,128] [--out FILE]
    HPFW_TREE=... python tools/time_index_remove.py --mode rebuild [--large] [--reps 5] [--large-reps 2] [--out FILE]

Random hashprints: the work does not depend on the values.  Prints one JSON line and writes --out.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# HPFW_TREE: the tree whose hpfw_amd package (and library) is timed -- an earlier commit's checkout for --mode rebuild
sys.path.insert(0, os.environ.get("HPFW_TREE") or ROOT)

PER = 2320
INDEXES = {"10000 x 2320": 10_000, "1000000 x 2320": 1_000_000}


def removals(n_clips):
    rng = np.random.default_rng(2100)
    return {"one clip at the front": np.array([0], np.int64),
            "1 % of the clips at random": np.sort(rng.choice(n_clips, n_clips // 100, replace=False)).astype(np.int64),
            "every other clip": np.arange(0, n_clips, 2, dtype=np.int64)}


def plan_bytes(lib, n_clips, ids, chunk):
    """(bytes the plan moves, of them in staged chunks, chunks)"""
    from hpfw_amd import _lib
    off = np.arange(0, (n_clips + 1) * PER, PER, dtype=np.int64)
    new = np.zeros_like(off)
    n = ctypes.c_int64(0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _lib.check(lib.hpfw_gpu_index_remove_plan(p(off), n_clips, p(ids), ids.size, chunk, p(new), None, 0, ctypes.byref(n)))
    mv = np.zeros(max(n.value, 1), _lib.INDEX_MOVE_DTYPE)
    _lib.check(lib.hpfw_gpu_index_remove_plan(p(off), n_clips, p(ids), ids.size, chunk, p(new), p(mv), mv.size, ctypes.byref(n)))
    mv = mv[:n.value]
    return int(mv["len"].sum()) * 8, int(mv["len"][mv["staged"] != 0].sum()) * 8, int(mv["chunk"].max()) + 1 if mv.size else 0


def summary(ms):
    return {"ms": round(float(np.median(ms)), 3), "min_max_ms": [round(min(ms), 3), round(max(ms), 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("remove", "rebuild"), required=True)
    ap.add_argument("--large", action="store_true", help="the index of 1 000 000 clips as well (18.6 GB, twice in HBM)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--large-reps", type=int, default=None, help="rounds on the large index (default: --reps)")
    ap.add_argument("--stage-mb", default="", help="chunk sizes in MiB for a sweep of the large front removal")
    ap.add_argument("--out", default=os.devnull)
    args = ap.parse_args()
    import torch
    import hpfw_amd
    from hpfw_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    lib = hpfw_amd.lib()
    g = hpfw_amd.Gpu(0)
    s = torch.cuda.current_stream()
    rows = []
    for label, n_clips in INDEXES.items():
        large = n_clips > 10_000
        if large and not args.large:
            continue
        reps = args.large_reps if large and args.large_reps else args.reps
        total = n_clips * PER
        d_src = torch.randint(-2 ** 63, 2 ** 63 - 1, (total,), dtype=torch.int64, device="cuda")
        off = np.arange(0, (n_clips + 1) * PER, PER, dtype=np.int64)

        def rebuild_index():
            g.index_clear()
            g.index_add_dev(d_src.data_ptr(), off, s.cuda_stream)
            torch.cuda.synchronize()

        sweeps = [("", None)]
        if args.mode == "remove" and large and args.stage_mb:
            sweeps += [(" at HPFW_INDEX_STAGE_MB=" + mb, mb) for mb in args.stage_mb.split(",")]
        for suffix, mb in sweeps:
            for what, ids in removals(n_clips).items():
                if mb is not None and what != "one clip at the front":
                    continue
                row = {"index": label, "removal": what + suffix, "clips_removed": int(ids.size)}
                if args.mode == "remove":
                    if mb is not None:
                        os.environ["HPFW_INDEX_STAGE_MB"] = mb
                    geo = [ctypes.c_int64(0), ctypes.c_int64(0)]
                    _lib.check(lib.hpfw_gpu_index_remove_geometry(ctypes.byref(geo[0]), ctypes.byref(geo[1])))
                    chunk = geo[1].value if mb is None else int(mb) * (1 << 20) // 8
                    moved, staged, chunks = plan_bytes(lib, n_clips, ids, chunk)
                    ms, copy_ms = [], []
                    d_a = torch.empty(max(moved // 8, 1), dtype=torch.int64, device="cuda")
                    d_b = torch.empty(max(moved // 8, 1), dtype=torch.int64, device="cuda")
                    for r in range(reps + 1):
                        rebuild_index()
                        a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                        a.record(s)
                        g.index_remove(ids, s.cuda_stream)
                        b.record(s)
                        d_b.copy_(d_a)                     # (contiguous, same device and type: one device-to-device hipMemcpyAsync)
                        c.record(s)
                        c.synchronize()
                        if r:
                            ms.append(a.elapsed_time(b))
                            copy_ms.append(b.elapsed_time(c))
                    os.environ.pop("HPFW_INDEX_STAGE_MB", None)
                    del d_a, d_b
                    row.update(summary(ms))
                    rate = moved / (row["ms"] * 1e-3) / 1e9 if moved else 0.0
                    copy_rate = moved / (float(np.median(copy_ms)) * 1e-3) / 1e9 if moved else 0.0
                    row.update({"chunk_hashprints": chunk, "chunks": chunks, "bytes_moved": moved, "bytes_in_staged_chunks": staged,
                                "GB_per_s": round(rate, 1), "memcpy_dtod": summary(copy_ms), "memcpy_dtod_GB_per_s": round(copy_rate, 1),
                                "rate_over_memcpy": round(rate / copy_rate, 3) if copy_rate else None})
                else:
                    keep = np.ones(n_clips, bool)
                    keep[ids] = False
                    sec = []
                    for r in range(reps + 1):
                        rebuild_index()
                        t0 = time.perf_counter()
                        hp, o = g.index_get()
                        new_hp = hp.reshape(n_clips, PER)[keep].ravel()
                        new_off = np.concatenate([[0], np.cumsum(np.where(keep, np.diff(o), 0))]).astype(np.int64)
                        g.index_clear()
                        g.index_add(new_hp, new_off)
                        torch.cuda.synchronize()
                        if r:
                            sec.append((time.perf_counter() - t0) * 1e3)
                        del hp, new_hp
                    row.update(summary(sec))
                row["rounds"] = reps
                rows.append(row)
                print(json.dumps(row), flush=True)
        g.index_clear()
        del d_src
        torch.cuda.empty_cache()
    g.close()
    rec = {"what": f"tools/time_index_remove.py --mode {args.mode} on one MI355X: "
                   + ("device events on the stream around hpfw_gpu_index_remove" if args.mode == "remove" else
                      "host clock around index_get, the filter on the host, index_clear and index_add")
                   + ", one warm-up round, the median of `rounds` rounds, the index rebuilt from a device copy between rounds",
           "tree": "another (HPFW_TREE)" if os.environ.get("HPFW_TREE") else "this", "rows": rows}
    print(json.dumps(rec), flush=True)
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
