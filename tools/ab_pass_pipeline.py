"""ab_pass_pipeline.py -- two handles of ONE process timed in turn on bench.py's workload: the passes of a back-end group
joined one after the other (HPFW_PASS_PIPELINE=0) against pipelined (the default; extract.hip run_group_pipelined).
Per pair and handle: the step (extract_dev, HIP events around `steps` calls).  The hashprints of the two handles must be
equal before and after.

  python tools/ab_pass_pipeline.py [pairs] [steps] [plan: HPFW_PASS_PLAN, - = default] [batch, 0 = default] [batch of the joined handle]
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
plan = sys.argv[3] if len(sys.argv) > 3 else "-"
batch = int(sys.argv[4]) if len(sys.argv) > 4 else 0
batch_joined = int(sys.argv[5]) if len(sys.argv) > 5 else batch
n_clips, n = 1000, 1323000


def handle(env, clips_per_pass):
    os.environ.update(env)
    try:
        g = hpfw_amd.Gpu(0)
    finally:
        for key in env:
            del os.environ[key]
    g.set_filters(synth.make_filters())
    if clips_per_pass:
        g.set_batch(clips_per_pass)
    return g


H = {"joined": handle({"HPFW_PASS_PIPELINE": "0"}, batch_joined), "pipelined": handle({} if plan == "-" else {"HPFW_PASS_PLAN": plan}, batch)}
dev = torch.device("cuda", 0)
pcm = synth_clips_gpu(torch, n_clips, n, 0x68706677, dev)
geo = H["joined"].geometry(n)
hp = {k: torch.zeros((n_clips, geo.n_hp), dtype=torch.int64, device=dev) for k in H}
stream = torch.cuda.current_stream().cuda_stream
for k, g in H.items():
    for _ in range(2):
        g.extract_dev(pcm.data_ptr(), n, n_clips, hp[k].data_ptr(), stream)
torch.cuda.synchronize()
assert torch.equal(hp["joined"], hp["pipelined"]), "the two loops give different hashprints"
step_ms = {k: [] for k in H}
for p in range(pairs):
    order = ["joined", "pipelined"] if p % 2 == 0 else ["pipelined", "joined"]
    for k in order:
        hp[k].zero_()
        H[k].timer_start(stream)
        for _ in range(steps):
            H[k].extract_dev(pcm.data_ptr(), n, n_clips, hp[k].data_ptr(), stream)
        step_ms[k].append(H[k].timer_stop(stream) / steps)
        torch.cuda.synchronize()
assert torch.equal(hp["joined"], hp["pipelined"]), "the two loops give different hashprints"
rng = {k: [round(min(v), 4), round(max(v), 4)] for k, v in step_ms.items()}
out = {"plan": "default" if plan == "-" else plan, "batch": {"joined": batch_joined or 256, "pipelined": batch or 256}, "pairs": pairs, "steps": steps,
       "step_ms": {k: {"median": round(statistics.median(v), 4), "range": rng[k], "all": [round(x, 4) for x in v]} for k, v in step_ms.items()},
       "ranges_apart": rng["pipelined"][1] < rng["joined"][0] or rng["joined"][1] < rng["pipelined"][0],
       "pipelined_lower": statistics.median(step_ms["pipelined"]) < statistics.median(step_ms["joined"]), "hashprints_equal": True}
print(json.dumps(out))
