"""ab_db_term.py -- two handles of ONE process timed in turn: the dB term by table and short polynomial (the default,
db_spec.h db_term_fast) against the specified sequence alone (HPFW_DB_TERM=spec) on bench.py's workload.  Per pair and
handle, after one untimed round: the step (extract_dev, HIP events around `steps` calls) and the constant-Q stage's time (cq_chirpz).  The
hashprints of the two handles are compared before and after.  Prints one JSON document.

  python tools/ab_db_term.py [pairs] [steps]
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
n_clips, n = 1000, 1323000


def handle(value):
    os.environ.pop("HPFW_DB_TERM", None)
    if value:
        os.environ["HPFW_DB_TERM"] = value
    try:
        g = hpfw_amd.Gpu(0)
    finally:
        os.environ.pop("HPFW_DB_TERM", None)
    g.set_filters(synth.make_filters())
    return g


H = {"fast": handle(None), "spec": handle("spec")}
dev = torch.device("cuda", 0)
pcm = synth_clips_gpu(torch, n_clips, n, 0x68706677, dev)
geo = H["fast"].geometry(n)
hp = {k: torch.zeros((n_clips, geo.n_hp), dtype=torch.int64, device=dev) for k in H}
stream = torch.cuda.current_stream().cuda_stream
for k, g in H.items():
    for _ in range(2):
        g.extract_dev(pcm.data_ptr(), n, n_clips, hp[k].data_ptr(), stream)
torch.cuda.synchronize()
equal_before = bool(torch.equal(hp["fast"], hp["spec"]))
# one untimed round: the first steps after the idle comparison above run 0.3 ms slower, whichever handle takes them
for k, g in H.items():
    for _ in range(steps):
        g.extract_dev(pcm.data_ptr(), n, n_clips, hp[k].data_ptr(), stream)
torch.cuda.synchronize()
step_ms = {k: [] for k in H}
cq_ms = {k: [] for k in H}
cq_bit = 1 << hpfw_amd.KERNEL_KINDS.index("cq_chirpz")
for p in range(pairs):
    order = ["fast", "spec"] if p % 2 == 0 else ["spec", "fast"]
    for k in order:
        H[k].timer_start(stream)
        for _ in range(steps):
            H[k].extract_dev(pcm.data_ptr(), n, n_clips, hp[k].data_ptr(), stream)
        step_ms[k].append(H[k].timer_stop(stream) / steps)
        torch.cuda.synchronize()
    for k in order:
        H[k].set_kernel_timing(cq_bit)
        for _ in range(steps):
            H[k].extract_dev(pcm.data_ptr(), n, n_clips, hp[k].data_ptr(), stream)
        torch.cuda.synchronize()
        cq_ms[k].append(H[k].kernel_timing()["cq_chirpz"][0] / steps)
        H[k].set_kernel_timing(0)
equal_after = bool(torch.equal(hp["fast"], hp["spec"]))


def summary(v):
    return {"ms": [round(x, 4) for x in v], "median": round(statistics.median(v), 4), "range": [round(min(v), 4), round(max(v), 4)]}


out = {"what": "one process, two handles in turn (tools/ab_db_term.py): the dB term by table and short polynomial (default) "
               "against HPFW_DB_TERM=spec (the specified sequence alone, as before); %d x 30 s clips, %d alternating pairs of "
               "%d steps; ms per step by HIP events; cq_chirpz = the constant-Q stage per step" % (n_clips, pairs, steps)}
for k in H:
    out[k] = {"step": summary(step_ms[k]), "cq_chirpz": summary(cq_ms[k])}
out["step_ranges_overlap"] = not (max(step_ms["fast"]) < min(step_ms["spec"]) or max(step_ms["spec"]) < min(step_ms["fast"]))
out["hashprints_equal"] = equal_before and equal_after
print(json.dumps(out, indent=1))
sys.exit(0 if out["hashprints_equal"] else 1)
