"""S6's column stage on the GPU at every n1 <= 255 the planner reaches, and at the chunk edges of the LDS-staged kernel
(tests/cols_ref.py sweep_lengths): forward bins bit-identical to the oracle's AND within the float64 bar of
tests/test_cols_host.py, on full-scale noise and on a clip tiled from the columns that load the paired int32
accumulators most.  Then the parity-split kernel's edge shapes under every load width, clip counts that leave the last
run of the XCD-ordered grid short, and the two kernels behind HPFW_COLS_VARIANT on both clip kinds.

Which kernel a length runs (k_forward.hip launch_cols_q_t): even n1 <= 224 fwd_cols_q4_kernel, odd n1 <= 224
fwd_cols_q3_kernel, 225 .. 255 fwd_cols_q_kernel<SMALL>, above that fwd_cols_q_kernel."""
import os

import numpy as np
import pytest

import cols_ref
from conftest import bits_equal
from test_cols_host import FLOAT64_BAR, SWEEP

pytestmark = pytest.mark.gpu

import hpfw_amd  # noqa: E402

# n1 = 8 (three computed rows, most of K padding), 32 (one live row in the last 16-row tile), 128 (one full 64-sample
# step per parity), 224 (eight row tiles); all with n2 % 4 == 0
EDGE = {8: 54432, 32: 131072, 128: 524288, 224: 917504}
_KEEP = set(EDGE.values()) | {54675, 57624, 65625, 1008420}      # lengths more than one test uses
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


def _spectrum(g, torch, plan, clips, shift=0):
    """forward bins [n_clips][kmax - kmin][2] of host clips [n_clips][n] laid `shift` samples into an aligned buffer"""
    n_clips, n = clips.shape
    buf = torch.zeros(n_clips * n + 8, dtype=torch.int16, device="cuda")
    buf[shift: shift + n_clips * n] = torch.from_numpy(np.array(clips, np.int16).reshape(-1)).cuda()
    d_x = torch.empty((n_clips, plan.kmax - plan.kmin, 2), dtype=torch.float32, device="cuda")
    g.stage_spectrum_dev(buf.data_ptr() + 2 * shift, n, n_clips, d_x.data_ptr())
    torch.cuda.synchronize()
    return d_x.cpu().numpy()


def _check(g, torch, oracle, n, shift=0):
    clips, plan, want = _case(oracle, n)
    got = _spectrum(g, torch, plan, clips, shift)
    for i, kind in enumerate(("noise", "worst")):
        assert bits_equal(got[i], want[i]), (n, plan.n1, kind, shift)
    return clips, plan, got


def _variant_handle(value):
    """a fresh handle created under HPFW_COLS_VARIANT = value (read at creation)"""
    os.environ["HPFW_COLS_VARIANT"] = value
    try:
        return hpfw_amd.Gpu(0)
    finally:
        del os.environ["HPFW_COLS_VARIANT"]


@pytest.mark.parametrize("n", SWEEP)
def test_sweep(gpu, torch_cuda, oracle, filters, n):
    geo = gpu.geometry(n)
    clips, plan, got = _check(gpu, torch_cuda, oracle, n)
    assert (geo.n1, geo.n2) == (plan.n1, plan.n2) == cols_ref.split(n)
    assert (geo.kmin, geo.kmax, geo.n_hp) == (plan.kmin, plan.kmax, plan.n_hp)
    for i, kind in enumerate(("noise", "worst")):
        err = cols_ref.float64_error(got[i], clips[i], plan.kmin, plan.kmax)
        print(f"n = {n} = {plan.n1} x {plan.n2}, {kind}: {err:.3g}")
        assert err < FLOAT64_BAR, (n, kind, err)
    hp = gpu.extract(clips[0])
    assert plan.n_hp >= 1 and np.array_equal(hp[0], plan.extract(filters, clips[0]))


# 8-byte loads at shift 0, 2-byte loads at shift 1, 4-byte loads at shift 2
@pytest.mark.parametrize("n1,shift", [(n1, s) for n1 in EDGE for s in (0, 1, 2)])
def test_load_widths_on_the_split_kernels_edge_shapes(gpu, torch_cuda, oracle, n1, shift):
    assert cols_ref.split(EDGE[n1])[0] == n1 and cols_ref.split(EDGE[n1])[1] % 4 == 0
    _check(gpu, torch_cuda, oracle, EDGE[n1], shift)


@pytest.mark.parametrize("shift", [0, 1])
def test_load_widths_with_n2_twice_an_odd_number(gpu, torch_cuda, oracle, shift):
    """57624 = 12 x 4802: 4-byte loads at best, the scalar store path and a partial last column block"""
    assert cols_ref.split(57624) == (12, 4802)
    _check(gpu, torch_cuda, oracle, 57624, shift)


# 54432 = 8 x 6804 (split kernel, 54 column blocks) and 54675 = 9 x 6075 (un-split, 48 column blocks: n_clips x 48 is
# always a multiple of 8), hence also 65625 = 15 x 4375 (un-split, 35 column blocks): with 1, 3, 5, 9 clips n_clips x 54
# and n_clips x 35 are no multiples of 8, the grid is rounded up and the last XCD's run is short
@pytest.mark.parametrize("n", [54432, 54675, 65625])
def test_clip_counts(gpu, torch_cuda, oracle, n):
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


@pytest.mark.parametrize("n1", [8, 128, 224])
def test_unsplit_kernel_on_even_n1(torch_cuda, oracle, n1):
    """HPFW_COLS_VARIANT bit 2: fwd_cols_q3_kernel on the even n1 that fwd_cols_q4_kernel takes by default"""
    g = _variant_handle("2")
    try:
        _check(g, torch_cuda, oracle, EDGE[n1])
    finally:
        g.close()


@pytest.mark.parametrize("n1", [8, 9, 128, 210, 224])
def test_lds_staged_small_kernel(torch_cuda, oracle, n1):
    """HPFW_COLS_VARIANT bit 1: fwd_cols_q_kernel<SMALL>, by default the kernel of n1 = 225 .. 255 only"""
    n = {9: 54675, 210: 1008420}.get(n1) or EDGE[n1]
    assert cols_ref.split(n)[0] == n1
    g = _variant_handle("1")
    try:
        _check(g, torch_cuda, oracle, n)
    finally:
        g.close()
