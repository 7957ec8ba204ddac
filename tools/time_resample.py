"""Times the sample-rate conversion to 44.1 kHz (k_resample.hip) on one MI355X.

  kernel  1 000 x 30 s clips at 16, 48 and 96 kHz through hpfw_gpu_resample_pcm16 (device buffers, device events around
          the launch on the current stream, one warm-up, median of --reps); achieved bytes/s on the compulsory bytes
          (every input sample read once, every output sample written once)
  files   ParallelCollector.calc_hashprints over --files equal-length 30 s files written at 48 kHz (switch on) and over
          the same clips at 44.1 kHz, in the same call: files/s, median of --reps after one warm-up pass

    python tools/time_resample.py [--reps 5] [--files 128] [--out profiles/resample.json]

Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys
import tempfile
import time
from math import gcd

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hpfw_amd  # noqa: E402
from hpfw_amd import synth  # noqa: E402


def kernel_times(torch, g, reps, clips=1000, seconds=30):
    out = {}
    for fs in (16000, 48000, 96000):
        n_in = fs * seconds
        n_out = hpfw_amd.resample_length(n_in, fs)
        x = torch.randint(-32768, 32767, (clips, n_in), dtype=torch.int16, device="cuda")
        y = torch.empty((clips, n_out), dtype=torch.int16, device="cuda")
        s = torch.cuda.current_stream()
        ms = []
        for r in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            g.resample_dev(x.data_ptr(), n_in, clips, fs, y.data_ptr(), s.cuda_stream)
            b.record(s)
            b.synchronize()
            if r:
                ms.append(a.elapsed_time(b))
        med = float(np.median(ms))
        L, M, taps = hpfw_amd.resample_table(fs)
        bytes_ = clips * (n_in + n_out) * 2
        out[str(fs)] = {"ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
                        "taps_per_phase": int(taps.shape[1]), "table_bytes": int(taps.nbytes),
                        "compulsory_GB": round(bytes_ / 1e9, 3), "achieved_TBps": round(bytes_ / (med * 1e-3) / 1e12, 3),
                        "int16_MACs_G": round(clips * n_out * taps.shape[1] / 1e9, 2)}
        del x, y
        torch.cuda.empty_cache()
    return out


def file_rates(filters, n_files, reps, seconds=30):
    from scipy.signal import resample_poly
    work = tempfile.mkdtemp(prefix="time_resample_")
    cache = os.path.join(work, "cache")
    os.makedirs(cache)
    with open(os.path.join(cache, "filters.cereal"), "wb") as f:
        f.write(np.array([64, 2420], np.int32).tobytes())
        f.write(np.ascontiguousarray(filters, np.float32).tobytes())
    g = gcd(44100, 48000)
    f44, f48 = [], []
    for i in range(n_files):
        x = synth.gen_clip(3000 + i, seconds)
        p = os.path.join(work, f"a{i:04d}.wav")
        synth.write_wav(p, x)
        f44.append(p)
        y = np.clip(np.round(resample_poly(x.astype(np.float64), 48000 // g, 44100 // g)), -32768, 32767).astype(np.int16)
        p = os.path.join(work, f"b{i:04d}.wav")
        synth.write_wav(p, y[:48000 * seconds], rate=48000)
        f48.append(p)
    c = hpfw_amd.ParallelCollector(resample=True)
    c.load(cache)
    res = {}
    for name, files in (("44100", f44), ("48000", f48)):
        got = c.calc_hashprints(files)                       # warm-up: tables of the length, buffers
        assert all(hp is not None for hp, _ in got), name
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            c.calc_hashprints(files)
            ts.append(time.perf_counter() - t0)
        med = float(np.median(ts))
        res[name] = {"files": n_files, "seconds_each": seconds, "s": round(med, 4), "files_per_s": round(n_files / med, 1)}
    res["ratio_48k_to_44k"] = round(res["48000"]["files_per_s"] / res["44100"]["files_per_s"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--files", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample.json"))
    args = ap.parse_args()
    import torch
    g = hpfw_amd.Gpu(0)
    rec = {"kernel_1000x30s": kernel_times(torch, g, args.reps)}
    g.close()
    rec["calc_hashprints"] = file_rates(synth.make_filters(), args.files, args.reps)
    rec["targets"] = {"kernel_48k_ms_max": 2.5, "files_48k_over_44k_min": 0.8}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
