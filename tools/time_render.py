"""Times the time warp and the fused mix (hpfw_amd/csrc/k_warp.hip) beside the fixed-ratio resampler:

  * mix:      8 tracks of 180 s on clocks up to 400 ppm apart, mixed (hpfw_gpu_mix_pcm16): 180 s of output;
  * warp:     1 000 tracks of 30 s warped (hpfw_gpu_warp_pcm16): --ppm 100 by default, and 0 and 977 for the table's two ends
              (one row per wave; 256 rows per wave);
  * resample: hpfw_gpu_resample_pcm16 from 48 kHz to the same number of output samples -- the yardstick (section 10).

    python tools/time_render.py [--reps 5] [--out profiles/render.json]

Every step is a process of its own under `timeout`, started one after the other; the first that fails ends the run.  A step
times with device events around the call on the stream, operands on the device: the median of --reps after one warm-up.  The
bytes a step must move (int16 in and out, once) over its time is its rate; the JSON holds the figures and the ratios.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR = 44100
STEPS = ("mix", "warp", "warp0", "warp977", "resample")
LIMIT_S = {"mix": 240, "warp": 300, "warp0": 300, "warp977": 300, "resample": 300}
N_TRACKS, TRACK_S = 1000, 30


def _events(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def _noise(torch, n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(-20000, 20000, (n,), generator=g, device="cuda", dtype=torch.int32).to(torch.int16)


def step(name, reps):
    import torch
    import hpfw_amd
    from hpfw_amd import _lib
    g = hpfw_amd.Gpu(0)
    stream = torch.cuda.current_stream().cuda_stream
    if name == "mix":
        n_src, n_out = 180 * SR, 180 * SR
        ppm = (0, 60, -250, 400, -60, 120, 250, -400)
        d_pcm = _noise(torch, len(ppm) * n_src, 1)
        tr = np.zeros(len(ppm), _lib.WARP_TRACK_DTYPE)
        for k, p in enumerate(ppm):
            tr[k] = (k * n_src, n_src, -1000 * k, 12345 * k, int(round(p * 1e-6 * 2 ** 40)), 4096 * (-1 if k % 3 == 2 else 1), 0)
        d_out = torch.zeros(n_out, dtype=torch.int16, device="cuda")
        res = _events(torch, lambda: g.mix_dev(d_pcm.data_ptr(), d_pcm.numel(), tr, 0, n_out, d_out.data_ptr(), stream), reps)
        res.update(tracks=len(ppm), outputs=n_out, bytes=2 * (len(ppm) * n_src + n_out), taps=len(ppm) * n_out * 32)
    elif name.startswith("warp"):
        ppm = {"warp": 100.0, "warp0": 0.0, "warp977": 976.0}[name]
        n_src = TRACK_S * SR
        d_pcm = _noise(torch, N_TRACKS * n_src, 2)
        tr = np.zeros(N_TRACKS, _lib.WARP_TRACK_DTYPE)
        for k in range(N_TRACKS):
            d = int(round(ppm * 1e-6 * 2 ** 40)) * (1 if k % 2 == 0 else -1)
            tr[k] = (k * n_src, n_src, 0, (k * 0x9E3779B1) % (1 << 40), d, 1, 0)
        d_out = torch.zeros(N_TRACKS * n_src, dtype=torch.int16, device="cuda")
        res = _events(torch, lambda: g.warp_dev(d_pcm.data_ptr(), d_pcm.numel(), tr, 0, n_src, d_out.data_ptr(), stream), reps)
        res.update(tracks=N_TRACKS, outputs=N_TRACKS * n_src, ppm=ppm, bytes=4 * N_TRACKS * n_src, taps=N_TRACKS * n_src * 32)
    else:
        n_out = TRACK_S * SR                                            # the outputs of one warped track
        n_in = n_out * 160 // 147
        assert hpfw_amd.resample_length(n_in, 48000) == n_out
        _, _, taps = hpfw_amd.resample_table(48000)
        d_in = _noise(torch, N_TRACKS * n_in, 3)
        d_out = torch.zeros(N_TRACKS * n_out, dtype=torch.int16, device="cuda")
        res = _events(torch, lambda: g.resample_dev(d_in.data_ptr(), n_in, N_TRACKS, 48000, d_out.data_ptr(), stream), reps)
        res.update(tracks=N_TRACKS, outputs=N_TRACKS * n_out, bytes=2 * N_TRACKS * (n_in + n_out), taps=N_TRACKS * n_out * int(taps.shape[1]))
    res["gbytes_per_s"] = res["bytes"] / res["median_ms"] / 1e6
    res["gtaps_per_s"] = res["taps"] / res["median_ms"] / 1e6
    res["outputs_per_s"] = res["outputs"] / res["median_ms"] * 1e3
    g.close()
    print("RESULT " + json.dumps({name: res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render.json"))
    ap.add_argument("--step", choices=STEPS)
    args = ap.parse_args()
    if args.step:
        return step(args.step, args.reps)
    results = {}
    for name in STEPS:                                                  # chained: nothing starts after a step that failed
        cmd = ["timeout", "-k", "10", str(LIMIT_S[name]), sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            print(f"step {name} ended with status {r.returncode}: stopping", flush=True)
            return r.returncode
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                results.update(json.loads(line[len("RESULT "):]))
    rs = results["resample"]
    results["ratios"] = {
        "warp_time_over_resample_time": results["warp"]["median_ms"] / rs["median_ms"],
        "warp0_time_over_resample_time": results["warp0"]["median_ms"] / rs["median_ms"],
        "warp977_time_over_resample_time": results["warp977"]["median_ms"] / rs["median_ms"],
        "mix_outputs_per_s_over_realtime": results["mix"]["outputs_per_s"] / SR,
    }
    results["method"] = f"device events around the call, operands on the device, median of {args.reps} after one warm-up; one process per step"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(results["ratios"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
