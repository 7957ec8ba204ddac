"""The pipelined pass loop of the extraction (extract.hip run_group_pipelined): the forward chunks of
pass p + 1 are queued behind the chirp-z classes of pass p, pass p keeps its forward bins in X[p & 1], and only events
order the lanes.  Every clip differs from every other, so a stale X buffer, S slot or wave maximum gives wrong hashprints.
HPFW_PASS_PIPELINE=0 at handle creation keeps the joined loop; the clips are 2 s (88 200 samples, 7-smooth)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("HPFW_PASS_PIPELINE", "HPFW_PASS_PLAN", "HPFW_FWD_CHUNK", "HPFW_FWD_STREAMS")


@pytest.fixture(scope="module")
def clips40():
    base = np.stack([synth.gen_clip(1200 + i, 2.0) for i in range(10)])
    clips = np.concatenate([np.roll(base, 41 * r + 3, axis=1) for r in range(4)])      # 40 different clips
    clips[3::10] = -clips[3::10]
    clips.setflags(write=False)
    return clips


@pytest.fixture(scope="module")
def want40(oracle, filters, clips40):
    want = oracle.Plan(clips40.shape[1]).extract_batch(filters, clips40, n_threads=8)
    want.setflags(write=False)
    return want


def make(monkeypatch, filters, batch=12, **env):
    """a handle created under the given switches (read at creation), the others unset"""
    for key in SWITCHES:
        monkeypatch.delenv(key, raising=False)
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    g = hpfw_amd.Gpu(0)
    for key in SWITCHES:
        monkeypatch.delenv(key, raising=False)
    g.set_filters(filters)
    if batch:
        g.set_batch(batch)
    return g


def run_thrice(torch, g, d, n, n_hp, stream):
    """the call twice back to back on `stream` and a third right behind on another stream -> the three results"""
    other = torch.cuda.Stream()
    hp = [torch.zeros((d.shape[0], n_hp), dtype=torch.int64, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    g.extract_dev(d.data_ptr(), n, d.shape[0], hp[0].data_ptr(), stream)
    g.extract_dev(d.data_ptr(), n, d.shape[0], hp[1].data_ptr(), stream)
    g.extract_dev(d.data_ptr(), n, d.shape[0], hp[2].data_ptr(), other.cuda_stream)
    torch.cuda.synchronize()
    return [h.cpu().numpy().view(np.uint64) for h in hp]


def check_against(torch, filters, monkeypatch, clips, want, envs):
    n = clips.shape[1]
    d = torch.from_numpy(np.array(clips)).cuda()
    joined = make(monkeypatch, filters, HPFW_FWD_CHUNK=envs[0]["HPFW_FWD_CHUNK"], HPFW_PASS_PIPELINE="0")
    ref = run_thrice(torch, joined, d, n, want.shape[1], 0)[0]
    one_x = joined.debug_workspace(1)[1]                      # the forward bins of one pass
    joined.close()
    assert np.array_equal(ref, want), "the joined loop differs from the oracle"
    for env in envs:
        g = make(monkeypatch, filters, **env)
        side = torch.cuda.Stream()
        for stream in (0, side.cuda_stream):
            for k, got in enumerate(run_thrice(torch, g, d, n, want.shape[1], stream)):
                assert np.array_equal(got, want), (env, stream, k, int((got != want).any(axis=1).sum()))
                assert np.array_equal(got, ref), (env, stream, k)
        assert g.debug_workspace(1)[1] >= 2 * one_x, "the pipelined loop (two X buffers) did not run"
        g.close()


def test_four_equal_passes(torch_cuda, filters, monkeypatch, clips40, want40):
    """40 clips at a batch of 12: four passes of 10, ten chunks of one clip per pass on two lanes; the default plan of three lanes,
    and the classes spread over five and over four lanes"""
    check_against(torch_cuda, filters, monkeypatch, clips40, want40,
                  [{"HPFW_FWD_CHUNK": "1"}, {"HPFW_FWD_CHUNK": "1", "HPFW_PASS_PLAN": "23401:01"}, {"HPFW_FWD_CHUNK": "1", "HPFW_PASS_PLAN": "23010:01"}])


def test_ragged_passes_and_three_forward_lanes(torch_cuda, filters, monkeypatch, clips40, want40):
    """37 clips: passes of 10, 10, 10 and 7; also with three forward lanes, and with uneven turns"""
    check_against(torch_cuda, filters, monkeypatch, clips40[:37], want40[:37],
                  [{"HPFW_FWD_CHUNK": "1"}, {"HPFW_FWD_CHUNK": "1", "HPFW_FWD_STREAMS": "3"},
                   {"HPFW_FWD_CHUNK": "1", "HPFW_PASS_PLAN": "34012:0121"}])


def test_passes_too_small_take_the_joined_loop(torch_cuda, filters, monkeypatch, clips40, want40):
    """33 clips in chunks of two: passes of 11 are below six chunks, so the joined loop runs (one forward span per pass, and
    every kind may be timed beside it)"""
    torch = torch_cuda
    clips, want = clips40[:33], want40[:33]
    d = torch.from_numpy(np.array(clips)).cuda()
    x_bytes = []
    for env in ({"HPFW_PASS_PIPELINE": "0"}, {}):
        g = make(monkeypatch, filters, HPFW_FWD_CHUNK="2", **env)
        for got in run_thrice(torch, g, d, clips.shape[1], want.shape[1], 0):
            assert np.array_equal(got, want)
        x_bytes.append(g.debug_workspace(1)[1])
        g.close()
    assert x_bytes[1] == x_bytes[0] > 0, "the pipelined loop ran (a second X buffer) on passes below six chunks"


def test_two_back_end_groups(torch_cuda, oracle, filters, monkeypatch, clips40):
    """1030 clips at the default batch: a group of 1024 clips in passes of 206, then a group of 6 through the joined loop"""
    torch = torch_cuda
    n = clips40.shape[1]
    clips = np.concatenate([np.roll(clips40, 97 * r + 11, axis=1) for r in range(26)])[:1030]
    clips[7::13] = -clips[7::13]
    d = torch.from_numpy(clips).cuda()
    plan = oracle.Plan(n)
    got = {}
    for name, env in (("joined", {"HPFW_PASS_PIPELINE": "0"}), ("pipelined", {})):
        g = make(monkeypatch, filters, batch=0, **env)
        hp = torch.zeros((len(clips), plan.n_hp), dtype=torch.int64, device="cuda")
        g.extract_dev(d.data_ptr(), n, len(clips), hp.data_ptr(), 0)
        g.extract_dev(d.data_ptr(), n, len(clips), hp.data_ptr(), 0)
        torch.cuda.synchronize()
        got[name] = hp.cpu().numpy().view(np.uint64)
        g.close()
    assert np.array_equal(got["pipelined"], got["joined"])
    idx = np.unique(np.linspace(0, len(clips) - 1, 32).astype(np.int64))
    want = plan.extract_batch(filters, clips[idx], n_threads=8)
    assert np.array_equal(got["pipelined"][idx], want)


def test_timing_switch(torch_cuda, filters, monkeypatch, clips40, want40):
    """with the hashprint kernel's and the forward span's bits alone the pipelined loop runs and reports one span per pass;
    with every bit set the call takes the joined loop and every kind that reports there reports launches"""
    torch = torch_cuda
    n = clips40.shape[1]
    d = torch.from_numpy(np.array(clips40)).cuda()
    kinds = hpfw_amd.KERNEL_KINDS
    reports = {}
    for name, env in (("joined", {"HPFW_PASS_PIPELINE": "0"}), ("pipelined", {})):
        g = make(monkeypatch, filters, HPFW_FWD_CHUNK="1", **env)
        hp = torch.zeros((len(clips40), want40.shape[1]), dtype=torch.int64, device="cuda")
        g.set_kernel_timing((1 << kinds.index("fwd_span")) | (1 << kinds.index("project_mfma")))
        g.extract_dev(d.data_ptr(), n, len(clips40), hp.data_ptr(), 0)
        torch.cuda.synchronize()
        kt = g.kernel_timing()
        assert kt["fwd_span"][1] == 4 and kt["fwd_span"][0] > 0, kt
        assert kt["project_mfma"][1] == 1, kt
        assert np.array_equal(hp.cpu().numpy().view(np.uint64), want40)
        hp.zero_()
        g.set_kernel_timing(-1)
        g.extract_dev(d.data_ptr(), n, len(clips40), hp.data_ptr(), 0)
        torch.cuda.synchronize()
        reports[name] = {k: v[1] for k, v in g.kernel_timing().items()}
        g.set_kernel_timing(0)
        assert np.array_equal(hp.cpu().numpy().view(np.uint64), want40)
        g.close()
    assert reports["pipelined"] == reports["joined"], reports       # the same launch counts, kind by kind
    for kind in ("fwd_rows", "fwd_cols", "cq_chirpz", "db", "project_mfma", "fwd_span"):
        assert reports["pipelined"][kind] > 0, reports


def test_two_ranks_on_one_gpu(torch_cuda):
    """two processes on the chip, each with the pipelined default: the one-GPU rehearsal of bench.py's two-rank run checks 32
    clips of the batch against the oracle while the other rank's kernels run beside them"""
    env = dict(os.environ, HPFW_BENCH_REHEARSE_ONE_GPU="1")
    for key in SWITCHES:
        env.pop(key, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--nproc-per-node", "2", os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--full", "--no-stream", "--no-search"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, r.stdout[-2000:]
    out = json.loads(lines[-1])
    assert out["parity"]["bit_identical"] is True, out["parity"]
    assert out["parity"]["clips_checked"] == 32
