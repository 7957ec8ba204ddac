"""ab_q_staging.py -- two handles of ONE process timed in turn on bench.py's workload: the hashprint kernel that stages its
slab by chains (one quantisation per dB term, digit planes by byte permute, loads two tasks ahead) and dispatches the
clips' short last tiles last (the default) against the same kernel with the staging and the workgroup order as they
were (HPFW_Q_STAGING=classic at handle creation).  After `untimed` untimed rounds,
`pairs` alternating pairs of `steps` steps: the step (extract_dev, HIP events around `steps` calls) and project_mfma, the
span of the hashprint launches.  The hashprints of both handles are compared before and after, and the debug counts of
both are reported.  Then the degenerate input: 256 clips of a spectrogram whose Du has one digit (every tile above the
cap), the width of a 30 s clip, hashprints_from_db_dev timed on both handles -- recorded, not part of the rule.  Prints
one JSON document and writes it to `out` when given.

  python tools/ab_q_staging.py [untimed] [pairs] [steps] [out.json]
"""
import json
import os
import statistics
import sys

import numpy as np
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
A, B = "chains", "classic"


def handle(kind):
    if kind == B:
        os.environ["HPFW_Q_STAGING"] = "classic"
    try:
        g = hpfw_amd.Gpu(0)
    finally:
        os.environ.pop("HPFW_Q_STAGING", None)
    g.set_filters(synth.make_filters())
    return g


H = {k: handle(k) for k in (A, B)}
dev = torch.device("cuda", 0)
pcm = synth_clips_gpu(torch, n_clips, n, 0x68706677, dev)
geo = H[A].geometry(n)
hp = {k: torch.zeros((n_clips, geo.n_hp), dtype=torch.int64, device=dev) for k in H}
stream = torch.cuda.current_stream().cuda_stream


def run(k, count):
    for _ in range(count):
        H[k].extract_dev(pcm.data_ptr(), n, n_clips, hp[k].data_ptr(), stream)


for k in H:
    run(k, 2)
torch.cuda.synchronize()
equal_before = bool(torch.equal(hp[A], hp[B]))
counts = {k: H[k].debug_q_products() for k in H}
KIND = "project_mfma"


def summary(v):
    return {"ms": [round(x, 4) for x in v], "median": round(statistics.median(v), 4), "range": [round(min(v), 4), round(max(v), 4)]}


def overlap(a, b):
    return not (max(a) < min(b) or max(b) < min(a))


def timed_kind(k, call, count):
    H[k].set_kernel_timing(1 << hpfw_amd.KERNEL_KINDS.index(KIND))
    for _ in range(count):
        call(k)
    torch.cuda.synchronize()
    ms = H[k].kernel_timing()[KIND][0] / count
    H[k].set_kernel_timing(0)
    return ms


out = {"what": "one process, two handles in turn (tools/ab_q_staging.py): the hashprint kernel staging its slab by chains, short "
               "tiles dispatched last, against HPFW_Q_STAGING=classic (the staging and the workgroup order as they were); %d x 30 s "
               "clips, %d alternating pairs of %d steps; ms per step by HIP events; project_mfma = the span of the hashprint "
               "launches per step" % (n_clips, pairs, steps),
       "debug_counts": {k: dict(zip(("tiles", "listed", "redone"), counts[k])) for k in H}}
# untimed rounds: the first steps after an idle comparison run slower, whichever handle takes them
for _ in range(untimed):
    for k in H:
        run(k, steps)
torch.cuda.synchronize()
ms = {k: {"step": [], KIND: []} for k in H}
for p in range(pairs):
    order = [A, B] if p % 2 == 0 else [B, A]
    for k in order:
        H[k].timer_start(stream)
        run(k, steps)
        ms[k]["step"].append(H[k].timer_stop(stream) / steps)
        torch.cuda.synchronize()
    for k in order:
        ms[k][KIND].append(timed_kind(k, lambda q: run(q, 1), steps))
for k in H:
    out[k] = {q: summary(v) for q, v in ms[k].items()}
out["ranges_overlap"] = {q: overlap(ms[A][q], ms[B][q]) for q in ms[A]}
out["median_gain_ms"] = {q: round(statistics.median(ms[B][q]) - statistics.median(ms[A][q]), 4) for q in ms[A]}
out["keep"] = (not out["ranges_overlap"][KIND]) and out["median_gain_ms"][KIND] > 0 and out["median_gain_ms"]["step"] >= 0
torch.cuda.synchronize()
equal_after = bool(torch.equal(hp[A], hp[B]))
out["hashprints_equal"] = equal_before and equal_after

# the degenerate input: every tile above the cap
del pcm
deg_clips, c = 256, int(geo.c)
rng = np.random.default_rng(9)
one = torch.from_numpy(((-40 * 98304 + rng.integers(0, 128, (4, 121, c))) / 98304.0).astype(np.float32)).to(dev)
sdb = one.repeat(deg_clips // 4, 1, 1).contiguous()
dhp = {k: torch.zeros((deg_clips, c - 99), dtype=torch.int64, device=dev) for k in H}


def from_db(k):
    H[k].hashprints_from_db_dev(sdb.data_ptr(), deg_clips, c, dhp[k].data_ptr(), stream)


for k in H:
    from_db(k)
torch.cuda.synchronize()
deg = {k: [] for k in H}
for p in range(4):
    for k in ([A, B] if p % 2 == 0 else [B, A]):
        deg[k].append(timed_kind(k, from_db, 3))
out["one_digit_input"] = {"clips": deg_clips, "c": c, "debug_counts": {k: list(H[k].debug_q_products()) for k in H},
                          "hashprints_equal": bool(torch.equal(dhp[A], dhp[B])), KIND: {k: summary(v) for k, v in deg.items()}}
text = json.dumps(out, indent=1)
print(text)
if out_path:
    with open(out_path, "w") as f:
        f.write(text + "\n")
sys.exit(0 if out["hashprints_equal"] and out["one_digit_input"]["hashprints_equal"] else 1)
