"""ab_prune.py -- handles of ONE process timed in turn: what the transforms leave out (HPFW_PRUNE at handle creation, a bit
mask: 1 = the row stage's unread last-group outputs) against a handle with none of it (HPFW_PRUNE=0, the kernels as they were) on bench.py's workload.  For every mask given,
`pairs` alternating pairs of `steps` steps, after one untimed round: the step (extract_dev, HIP events around `steps` calls),
the forward span and the constant-Q stage.  The hashprints of all handles are compared before and after.  Prints one JSON
document and writes it to `out` when given.

  python tools/ab_prune.py [masks, comma separated] [pairs] [steps] [out.json]
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

masks = [m for m in (sys.argv[1] if len(sys.argv) > 1 else "1").split(",") if m != "0"]
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 6
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
out_path = sys.argv[4] if len(sys.argv) > 4 else None
n_clips, n = 1000, 1323000


def handle(value):
    os.environ["HPFW_PRUNE"] = value
    try:
        g = hpfw_amd.Gpu(0)
    finally:
        os.environ.pop("HPFW_PRUNE", None)
    g.set_filters(synth.make_filters())
    return g


H = {m: handle(m) for m in ["0"] + masks}
dev = torch.device("cuda", 0)
pcm = synth_clips_gpu(torch, n_clips, n, 0x68706677, dev)
geo = H["0"].geometry(n)
hp = {k: torch.zeros((n_clips, geo.n_hp), dtype=torch.int64, device=dev) for k in H}
stream = torch.cuda.current_stream().cuda_stream


def run(k, count):
    for _ in range(count):
        H[k].extract_dev(pcm.data_ptr(), n, n_clips, hp[k].data_ptr(), stream)


for k in H:
    run(k, 2)
torch.cuda.synchronize()
equal_before = all(bool(torch.equal(hp[k], hp["0"])) for k in H)
KINDS = ("fwd_span", "fwd_rows", "cq_chirpz")


def summary(v):
    return {"ms": [round(x, 4) for x in v], "median": round(statistics.median(v), 4), "range": [round(min(v), 4), round(max(v), 4)]}


def overlap(a, b):
    return not (max(a) < min(b) or max(b) < min(a))


out = {"what": "one process, handles in turn (tools/ab_prune.py): HPFW_PRUNE=<mask> against HPFW_PRUNE=0 (the kernels without any "
               "pruning, as before); %d x 30 s clips, %d alternating pairs of %d steps per mask; ms per step by HIP events; fwd_span = "
               "the forward transform's span, fwd_rows = its row kernel's launches, cq_chirpz = the constant-Q stage, per step" % (n_clips, pairs, steps)}
for m in masks:
    duo = {"on": m, "off": "0"}
    # one untimed round: the first steps after an idle comparison run slower, whichever handle takes them
    for k in duo.values():
        run(k, steps)
    torch.cuda.synchronize()
    ms = {side: {"step": [], **{kind: [] for kind in KINDS}} for side in duo}
    for p in range(pairs):
        order = ["on", "off"] if p % 2 == 0 else ["off", "on"]
        for side in order:
            g = H[duo[side]]
            g.timer_start(stream)
            run(duo[side], steps)
            ms[side]["step"].append(g.timer_stop(stream) / steps)
            torch.cuda.synchronize()
        for kind in KINDS:
            for side in order:
                g = H[duo[side]]
                g.set_kernel_timing(1 << hpfw_amd.KERNEL_KINDS.index(kind))
                run(duo[side], steps)
                torch.cuda.synchronize()
                ms[side][kind].append(g.kernel_timing()[kind][0] / steps)
                g.set_kernel_timing(0)
    res = {side: {q: summary(v) for q, v in ms[side].items()} for side in duo}
    res["ranges_overlap"] = {q: overlap(ms["on"][q], ms["off"][q]) for q in ms["on"]}
    res["median_gain_ms"] = {q: round(statistics.median(ms["off"][q]) - statistics.median(ms["on"][q]), 4) for q in ms["on"]}
    out["HPFW_PRUNE=" + m] = res
torch.cuda.synchronize()
equal_after = all(bool(torch.equal(hp[k], hp["0"])) for k in H)
out["hashprints_equal"] = equal_before and equal_after
text = json.dumps(out, indent=1)
print(text)
if out_path:
    with open(out_path, "w") as f:
        f.write(text + "\n")
sys.exit(0 if out["hashprints_equal"] else 1)
