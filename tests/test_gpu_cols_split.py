"""S6's column stage for even n1 <= 224: the sum over k1 split by parity (k_forward.hip fwd_cols_q4_kernel), rows
q1 <= n1 / 4 computed and rows n1 / 2 - q1 formed from them.  Same exact integers as the un-split kernel, so the forward
bins stay bit-identical to the oracle's: one tile and many, n1 / 2 odd and even (the middle row reached by both
formulas), every load width, a partial last column block, and the un-split kernel behind its switch."""
import os

import numpy as np
import pytest

from conftest import bits_equal

pytestmark = pytest.mark.gpu

import hpfw_amd  # noqa: E402
from hpfw_amd import synth  # noqa: E402

_REF = {}


def _case(oracle, n):
    """two clips with the ends of the int16 range planted and full-scale noise, and the oracle's forward bins: once per length"""
    if n not in _REF:
        rng = np.random.default_rng(n)
        clips = np.stack([synth.gen_clip(1970 + i, n / 44100.0)[:n] for i in range(2)])
        clips[0, ::97] = 32767
        clips[0, 5::89] = -32768
        clips[1, : n // 3] = rng.integers(-32768, 32768, n // 3).astype(np.int16)   # full-scale noise: every digit value
        clips[1, n // 3: n // 3 + 4096] = -32768                                    # ... and a run of the extreme in every column block
        plan = oracle.Plan(n)
        _REF[n] = (clips, plan, [plan.spectrum(c) for c in clips])
    return _REF[n]


def _check(g, torch, oracle, n, shift):
    clips, plan, want = _case(oracle, n)
    buf = torch.zeros(2 * n + 8, dtype=torch.int16, device="cuda")
    buf[shift: shift + 2 * n] = torch.from_numpy(clips.reshape(-1)).cuda()
    d_x = torch.empty((2, plan.kmax - plan.kmin, 2), dtype=torch.float32, device="cuda")
    g.stage_spectrum_dev(buf.data_ptr() + 2 * shift, n, 2, d_x.data_ptr())
    torch.cuda.synchronize()
    got = d_x.cpu().numpy()
    for i in range(2):
        assert bits_equal(got[i], want[i]), (n, shift, i)


# n1 = 14 (n1 / 2 odd, one tile); 28 (n1 / 2 even: the middle row); 30 with n2 = 6174 (n2 % 4 = 2: 4-byte loads, a partial
# last column block; shifted by one sample: 2-byte loads); 196 (n1 / 2 even, seven tiles); 210 (the 30 s clip); 210 with n2 = 6720
@pytest.mark.parametrize("n,shift", [(88200, 0), (176400, 0), (185220, 0), (185220, 1), (1234800, 0), (1323000, 0), (1411200, 0)])
def test_split_column_stage_is_bit_identical(gpu, torch_cuda, oracle, n, shift):
    _check(gpu, torch_cuda, oracle, n, shift)


def test_unsplit_column_kernel_behind_its_switch(torch_cuda, oracle, filters):
    """HPFW_COLS_VARIANT bit 2: even n1 on the un-split register-resident kernel, as before the split"""
    os.environ["HPFW_COLS_VARIANT"] = "2"
    try:
        g = hpfw_amd.Gpu(0)
    finally:
        del os.environ["HPFW_COLS_VARIANT"]
    try:
        _check(g, torch_cuda, oracle, 1323000, 0)
    finally:
        g.close()
