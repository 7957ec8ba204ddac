"""ab_q_products.py -- two handles of ONE process timed in turn on bench.py's workload: the six-product hashprint kernel
with its fix-up launch (the default) against the nine-product kernel (HPFW_Q_PRODUCTS=9 at handle creation).  After
`untimed` untimed rounds, `pairs` alternating pairs of `steps` steps: the step (extract_dev, HIP events around `steps`
calls) and project_mfma, the span of the hashprint launches (main kernel and fix-up).  The hashprints of both handles are
compared before and after, and the six-product handle's debug counts are reported.  Prints one JSON document and writes it
to `out` when given.

  python tools/ab_q_products.py [untimed] [pairs] [steps] [out.json]
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

untimed = int(sys.argv[1]) if len(sys.argv) > 1 else 1
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 6
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
out_path = sys.argv[4] if len(sys.argv) > 4 else None
n_clips, n = 1000, 1323000


def handle(value):
    os.environ["HPFW_Q_PRODUCTS"] = value
    try:
        g = hpfw_amd.Gpu(0)
    finally:
        os.environ.pop("HPFW_Q_PRODUCTS", None)
    g.set_filters(synth.make_filters())
    return g


H = {k: handle(k) for k in ("6", "9")}
dev = torch.device("cuda", 0)
pcm = synth_clips_gpu(torch, n_clips, n, 0x68706677, dev)
geo = H["9"].geometry(n)
hp = {k: torch.zeros((n_clips, geo.n_hp), dtype=torch.int64, device=dev) for k in H}
stream = torch.cuda.current_stream().cuda_stream


def run(k, count):
    for _ in range(count):
        H[k].extract_dev(pcm.data_ptr(), n, n_clips, hp[k].data_ptr(), stream)


for k in H:
    run(k, 2)
torch.cuda.synchronize()
equal_before = bool(torch.equal(hp["6"], hp["9"]))
tiles, listed, redone = H["6"].debug_q_products()
KIND = "project_mfma"


def summary(v):
    return {"ms": [round(x, 4) for x in v], "median": round(statistics.median(v), 4), "range": [round(min(v), 4), round(max(v), 4)]}


def overlap(a, b):
    return not (max(a) < min(b) or max(b) < min(a))


out = {"what": "one process, two handles in turn (tools/ab_q_products.py): six digit products and the fix-up launch against "
               "HPFW_Q_PRODUCTS=9 (the nine-product kernel); %d x 30 s clips, %d alternating pairs of %d steps; ms per step by HIP "
               "events; project_mfma = the span of the hashprint launches per step" % (n_clips, pairs, steps),
       "six_product_launch": {"tiles": tiles, "listed": listed, "redone": redone, "listed_per_clip": round(listed / n_clips, 2)}}
# untimed rounds: the first steps after an idle comparison run slower, whichever handle takes them
for _ in range(untimed):
    for k in H:
        run(k, steps)
torch.cuda.synchronize()
ms = {k: {"step": [], KIND: []} for k in H}
for p in range(pairs):
    order = ["6", "9"] if p % 2 == 0 else ["9", "6"]
    for k in order:
        H[k].timer_start(stream)
        run(k, steps)
        ms[k]["step"].append(H[k].timer_stop(stream) / steps)
        torch.cuda.synchronize()
    for k in order:
        H[k].set_kernel_timing(1 << hpfw_amd.KERNEL_KINDS.index(KIND))
        run(k, steps)
        torch.cuda.synchronize()
        ms[k][KIND].append(H[k].kernel_timing()[KIND][0] / steps)
        H[k].set_kernel_timing(0)
for k in H:
    out["HPFW_Q_PRODUCTS=" + k] = {q: summary(v) for q, v in ms[k].items()}
out["ranges_overlap"] = {q: overlap(ms["6"][q], ms["9"][q]) for q in ms["6"]}
out["median_gain_ms"] = {q: round(statistics.median(ms["9"][q]) - statistics.median(ms["6"][q]), 4) for q in ms["6"]}
out["keep"] = (not out["ranges_overlap"][KIND]) and out["median_gain_ms"][KIND] > 0 and out["median_gain_ms"]["step"] >= 0
torch.cuda.synchronize()
equal_after = bool(torch.equal(hp["6"], hp["9"]))
out["hashprints_equal"] = equal_before and equal_after
text = json.dumps(out, indent=1)
print(text)
if out_path:
    with open(out_path, "w") as f:
        f.write(text + "\n")
sys.exit(0 if out["hashprints_equal"] else 1)
