"""ab_cols_variant.py -- two handles of ONE process timed in turn: the column stage as HPFW_COLS_VARIANT=A against =B
(default: 0, the split kernel for even n1, against 2, the un-split register-resident one) on bench.py's workload.
Per pair and handle: the step (extract_dev, HIP events around `steps` calls) and the forward transform's span.

  python tools/ab_cols_variant.py [pairs] [steps] [variant A] [variant B]
"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hpfw_amd  # noqa: E402
from hpfw_amd import synth  # noqa: E402
from bench import synth_clips_gpu  # noqa: E402

pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 6
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
variants = {"a": sys.argv[3] if len(sys.argv) > 3 else "0", "b": sys.argv[4] if len(sys.argv) > 4 else "2"}
n_clips, n = 1000, 1323000


def handle(variant):
    os.environ["HPFW_COLS_VARIANT"] = variant
    try:
        g = hpfw_amd.Gpu(0)
    finally:
        del os.environ["HPFW_COLS_VARIANT"]
    g.set_filters(synth.make_filters())
    return g


H = {k: handle(v) for k, v in variants.items()}
dev = torch.device("cuda", 0)
pcm = synth_clips_gpu(torch, n_clips, n, 0x68706677, dev)
geo = H["a"].geometry(n)
hp = {k: torch.zeros((n_clips, geo.n_hp), dtype=torch.int64, device=dev) for k in H}
stream = torch.cuda.current_stream().cuda_stream
for k, g in H.items():
    for _ in range(2):
        g.extract_dev(pcm.data_ptr(), n, n_clips, hp[k].data_ptr(), stream)
torch.cuda.synchronize()
assert torch.equal(hp["a"], hp["b"]), "the two variants give different hashprints"
step_ms = {k: [] for k in H}
span_ms = {k: [] for k in H}
span_bit = 1 << hpfw_amd.KERNEL_KINDS.index("fwd_span")
for p in range(pairs):
    order = ["a", "b"] if p % 2 == 0 else ["b", "a"]
    for k in order:
        H[k].timer_start(stream)
        for _ in range(steps):
            H[k].extract_dev(pcm.data_ptr(), n, n_clips, hp[k].data_ptr(), stream)
        step_ms[k].append(H[k].timer_stop(stream) / steps)
        torch.cuda.synchronize()
    for k in order:
        H[k].set_kernel_timing(span_bit)
        for _ in range(steps):
            H[k].extract_dev(pcm.data_ptr(), n, n_clips, hp[k].data_ptr(), stream)
        torch.cuda.synchronize()
        span_ms[k].append(H[k].kernel_timing()["fwd_span"][0] / steps)
        H[k].set_kernel_timing(0)
assert torch.equal(hp["a"], hp["b"]), "the two variants give different hashprints"
for k in H:
    print(json.dumps({"HPFW_COLS_VARIANT": variants[k],
                      "step_ms": {"median": round(statistics.median(step_ms[k]), 4), "range": [round(min(step_ms[k]), 4), round(max(step_ms[k]), 4)]},
                      "fwd_span_ms": {"median": round(statistics.median(span_ms[k]), 4), "range": [round(min(span_ms[k]), 4), round(max(span_ms[k]), 4)]},
                      "pairs": pairs, "steps": steps}))
