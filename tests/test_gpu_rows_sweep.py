"""S6's row stage on the GPU at every row length n2 the planner reaches (tests/rows_ref.py row_lengths, frozen as
ROW_SWEEP in tests/test_rows_host.py): forward bins bit-identical to the oracle's AND within the float64 bar of
tests/test_cols_host.py, on full-scale noise and on the column sweep's worst-case clip, and the hashprints of the noise
clip.  Then three long lengths, one per loader class, and clip counts, the fast index of the row kernel's grid.

Every n2 but 6300 runs the run-time dispatcher RuntimeGroups::run (fft_rows.h) with its own sequence of fused groups;
56700 = 9 x 6300 keeps the compile-time sequence in the sweep (k_forward.hip launch_fwd_rows2)."""
import numpy as np
import pytest

import cols_ref
import rows_ref
from conftest import bits_equal
from test_cols_host import FLOAT64_BAR
from test_rows_host import ROW_LONG, ROW_SWEEP

pytestmark = pytest.mark.gpu

# one length per loader class of rows2_body: n2 = 6400 (16-byte pieces), 6750 (n2 % 4 == 2), 4725 (odd)
CLIP_COUNTS = {0: 57600, 2: 60750, "odd": 70875}
_KEEP = set(CLIP_COUNTS.values())      # lengths more than one test uses
_REF = {}


def _case(oracle, n):
    """(clips [2][n]: noise, worst-case columns; the oracle's plan; its forward bins of both): computed once per length"""
    if n in _REF:
        return _REF[n]
    clips = np.stack([cols_ref.noise_clip(n), cols_ref.worst_clip(n)])
    plan = oracle.Plan(n)
    case = (clips, plan, [plan.spectrum(c) for c in clips])
    for a in (clips, *case[2]):
        a.setflags(write=False)
    if n in _KEEP:
        _REF[n] = case
    return case


def _spectrum(g, torch, plan, clips):
    """forward bins [n_clips][kmax - kmin][2] of host clips [n_clips][n]"""
    n_clips, n = clips.shape
    buf = torch.zeros(n_clips * n + 8, dtype=torch.int16, device="cuda")      # as test_gpu_cols_sweep.py lays it
    buf[:n_clips * n] = torch.from_numpy(np.array(clips, np.int16).reshape(-1)).cuda()
    d_x = torch.empty((n_clips, plan.kmax - plan.kmin, 2), dtype=torch.float32, device="cuda")
    g.stage_spectrum_dev(buf.data_ptr(), n, n_clips, d_x.data_ptr())
    torch.cuda.synchronize()
    return d_x.cpu().numpy()


def _check(gpu, torch, oracle, filters, n, n2):
    geo = gpu.geometry(n)
    clips, plan, want = _case(oracle, n)
    assert (geo.n1, geo.n2) == (plan.n1, plan.n2) == cols_ref.split(n) and geo.n2 == n2
    assert (geo.kmin, geo.kmax, geo.n_hp) == (plan.kmin, plan.kmax, plan.n_hp)
    got = _spectrum(gpu, torch, plan, clips)
    where = (n, plan.n1, n2, rows_ref.seq(n2), rows_ref.loader_class(n2))
    for i, kind in enumerate(("noise", "worst")):
        assert bits_equal(got[i], want[i]), (*where, kind)
    for i, kind in enumerate(("noise", "worst")):
        err = cols_ref.float64_error(got[i], clips[i], plan.kmin, plan.kmax)
        print(f"n = {n} = {plan.n1} x {n2} [{rows_ref.seq(n2)}], {kind}: {err:.3g}")
        assert err < FLOAT64_BAR, (*where, kind, err)
    hp = gpu.extract(clips[0])
    assert plan.n_hp >= 1 and np.array_equal(hp[0], plan.extract(filters, clips[0])), where


@pytest.mark.parametrize("n,n2", ROW_SWEEP)
def test_sweep(gpu, torch_cuda, oracle, filters, n, n2):
    _check(gpu, torch_cuda, oracle, filters, n, n2)


@pytest.mark.parametrize("n,n2", ROW_LONG)
def test_long(gpu, torch_cuda, oracle, filters, n, n2):
    assert cols_ref.split(n)[0] > cols_ref.PAIR_N1
    _check(gpu, torch_cuda, oracle, filters, n, n2)


@pytest.mark.parametrize("loader", list(CLIP_COUNTS))
def test_clip_counts(gpu, torch_cuda, oracle, loader):
    """the clip is the fast index of the row kernel's grid: batches of 1, 3, 5 and 9 clips, clip for clip"""
    n = CLIP_COUNTS[loader]
    assert rows_ref.loader_class(cols_ref.split(n)[1]) == loader
    clips2, plan, want2 = _case(oracle, n)
    rng = np.random.default_rng(n + 1)
    clips = np.concatenate([clips2, rng.integers(-32768, 32768, (7, n)).astype(np.int16)])
    want = list(want2) + [plan.spectrum(c) for c in clips[2:]]
    alone = [_spectrum(gpu, torch_cuda, plan, clips[i:i + 1])[0] for i in range(9)]
    for i in range(9):
        assert bits_equal(alone[i], want[i]), (n, 1, i)
    for n_clips in (3, 5, 9):
        got = _spectrum(gpu, torch_cuda, plan, clips[:n_clips])
        for i in range(n_clips):
            assert bits_equal(got[i], alone[i]), (n, n_clips, i)
