"""Times the sample-accurate offsets (hpfw_amd/csrc/k_xcorr.hip) on the corpus of
tools/time_combiner.py (64 recordings of 60-180 s, two excerpts of each of 32 synthetic sources), on both kernels:

  * the refine stage of AudioCombiner.layout(): the pairs layout() selects (align all against all, k = 8, the better hit
    of every pair, peak >= --min-peak), refined in one call -- packing the slices on the host, upload, correlation, peaks;
  * 512 jobs of len = 2^18, radius = 1024 alone, operands already on the device (hpfw_gpu_xcorr_pcm16 + a synchronise).

    python tools/time_xcorr.py [--reps 5] [--min-peak 20]

Median of --reps after one warm-up call, host wall clock.  The matrix-core kernel is the default; HPFW_XCORR=valu (read at
every call) selects the plain integer kernel.  The two must give the same peaks.  Prints one JSON line at the end.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hpfw_amd  # noqa: E402
from hpfw_amd import _lib, synth  # noqa: E402


def corpus_pcm(n_rec=64, seed=0xC0B):
    """the PCM of tests/combiner_ref.py::mel_corpus"""
    rng = np.random.default_rng(seed)
    pcm, src = [], None
    for i in range(n_rec):
        if i % 2 == 0:
            src = synth.gen_clip(1000 + i // 2, 200.0)
        dur = int(rng.integers(60, 181)) * synth.SR
        at = int(rng.integers(0, (src.size - dur) // 441 + 1)) * 441
        pcm.append(src[at:at + dur])
    return pcm


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, float(np.min(ts)) * 1e3, float(np.max(ts)) * 1e3


def both_paths(fn, reps):
    """{path: (median, min, max) ms}, and the results of the two paths"""
    out, res = {}, {}
    for path in ("mfma", "valu"):
        if path == "valu":
            os.environ["HPFW_XCORR"] = "valu"
        else:
            os.environ.pop("HPFW_XCORR", None)
        res[path] = fn()
        out[path] = timed(fn, reps)
    os.environ.pop("HPFW_XCORR", None)
    return out, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-peak", type=int, default=20)
    args = ap.parse_args()
    import torch

    t0 = time.perf_counter()
    pcm = corpus_pcm()
    print(f"corpus: {len(pcm)} recordings, {sum(x.size for x in pcm) / synth.SR:.0f} s, generated in {time.perf_counter() - t0:.1f} s",
          flush=True)
    comb = hpfw_amd.AudioCombiner(keep_audio=True)
    g = comb._gpu
    g.cfg_cov_reset(_lib.COMBINER_CONFIG)
    for x in pcm[:8]:
        g.mel_cov_accumulate(x)
    g.cfg_learn_filters(_lib.COMBINER_CONFIG)
    names = [f"rec{i}" for i in range(len(pcm))]
    for name, x in zip(names, pcm):
        comb._audio[name] = (x, g.mel_kept_frames(x)[0])
    comb.build([(name, g.mel_hashprints(x)[0]) for name, x in zip(names, pcm)])
    t_pairs = timed(lambda: comb._layout_pairs(args.min_peak, 8), args.reps)
    pairs = comb._layout_pairs(args.min_peak, 8)
    print(f"layout: {len(pairs)} pairs with peak >= {args.min_peak}; align all-vs-all + selection: median {t_pairs[0]:.2f} ms", flush=True)

    t_refine, fine = both_paths(lambda: comb._refine_pairs(pairs, 1 << 18, 1024), args.reps)
    same = fine["mfma"] == fine["valu"]
    sources = sum(1 for (qi, h) in pairs if qi // 2 == h.rec // 2)
    good = sum(1 for f in fine["mfma"] if abs(f.score) >= 0.5)
    for path in ("mfma", "valu"):
        m = t_refine[path]
        print(f"refine stage, {path}: median {m[0]:.2f} ms (min {m[1]:.2f}, max {m[2]:.2f})", flush=True)
    print(f"both kernels give the same refined hits: {same}; {sources} pairs share a source, {good} have |score| >= 0.5")

    # 512 jobs alone, on the device
    n_jobs, length, radius = 512, 1 << 18, 1024
    rng = np.random.default_rng(7)
    buf = rng.integers(-32768, 32768, size=1 << 22).astype(np.int16)
    a_len = length + 2 * radius
    rows = [(4096 * i, a_len, (1 << 21) + 2048 * i, length, radius, 0, length, radius, 0) for i in range(n_jobs)]
    jobs = np.array(rows, _lib.XCORR_JOB_DTYPE)
    assert rows[-1][0] + a_len <= buf.size and rows[-1][2] + length <= buf.size
    d_pcm = torch.from_numpy(buf).cuda()
    d_peaks = torch.zeros(n_jobs * _lib.XCORR_PEAK_DTYPE.itemsize, dtype=torch.uint8, device="cuda")

    def run_jobs():
        g.xcorr_dev(d_pcm.data_ptr(), jobs, 0, d_peaks.data_ptr(), 0)
        torch.cuda.synchronize()
        return d_peaks.cpu().numpy().view(_lib.XCORR_PEAK_DTYPE).copy()

    t_jobs, pk = both_paths(run_jobs, args.reps)
    same_jobs = bool(np.array_equal(pk["mfma"], pk["valu"]))
    macs = n_jobs * (2 * radius + 1) * length
    for path in ("mfma", "valu"):
        m = t_jobs[path]
        print(f"{n_jobs} jobs of len 2^18, radius {radius}, {path}: median {m[0]:.2f} ms (min {m[1]:.2f}, max {m[2]:.2f}); "
              f"{macs / m[0] / 1e9:.1f} T int16 products/s", flush=True)
    print(f"both kernels give the same peaks: {same_jobs}")
    comb.close()
    print(json.dumps({"pairs": len(pairs), "pairs_ms": round(t_pairs[0], 3),
                      "refine_ms": {p: round(t_refine[p][0], 3) for p in t_refine},
                      "jobs512_ms": {p: round(t_jobs[p][0], 3) for p in t_jobs},
                      "same_refined": bool(same), "same_peaks": same_jobs}))
    return 0 if same and same_jobs else 1


if __name__ == "__main__":
    sys.exit(main())
