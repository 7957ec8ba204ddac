"""S15's chirp-z forward transform on the GPU at every class of its kernels' shapes (tests/bz_ref.py sweep_lengths: every
a = n1 / 16 up to 17, 32 and 33, exact fits, every class of the last stage up to a = 59, the row-tile edges of the consumed
rows): forward bins bit-identical to the oracle's, which tests/test_bz_host.py holds to float64, on full-scale noise and on
a clip that knows only the two ends of the int16 range.  The clips lie back to back in a buffer filled with 32767, so a
sample read past a clip's end shows.  Then both 2-byte alignments of the first sample, clip counts, and a 7-smooth length
forced into the transform at the least slack there is.

Which kernels a length runs (k_bluestein.hip): bz_colsin_kernel (a; the operand prefetch pads a to a multiple of 4, a tile
holds 16 outputs), bz_rows2_kernel, bz_cols_kernel<1, step, nt2> (plan.h bz_shape)."""
import numpy as np
import pytest

import bz_ref
from conftest import bits_equal
from test_bz_host import SWEEP

pytestmark = pytest.mark.gpu

import hpfw_amd  # noqa: E402

FILL = 16 * bz_ref.N2 + 8           # samples of 32767 behind the last clip: a whole step of the convolution length
ONE_CLIP_ABOVE = 3400000            # longer lengths run one clip: the oracle's share of the test stays at a few seconds
EXTRACT_UP_TO = 1500000
A1, A16_EXACT, A17 = bz_ref.first_length(1), bz_ref.last_length(16), bz_ref.first_length(17)
_KEEP = {A1, A16_EXACT, A17}        # lengths more than one test uses
_REF = {}


def _case(oracle, n):
    """(clips [2][n]: noise, rail; the oracle's plan; its forward bins of both): computed once per length"""
    if n in _REF:
        return _REF[n]
    clips = np.stack([bz_ref.noise_clip(n), bz_ref.rail_clip(n)])
    plan = oracle.Plan(n)
    case = (clips, plan, [plan.spectrum(c) for c in clips])
    for a in (clips, *case[2]):
        a.setflags(write=False)
    if n in _KEEP:
        _REF[n] = case
    return case


def _spectrum(g, torch, plan, clips, shift=0):
    """forward bins [n_clips][kmax - kmin][2] of host clips [n_clips][n] laid back to back, `shift` samples into an aligned
    buffer of 32767s"""
    n_clips, n = clips.shape
    buf = torch.full((shift + n_clips * n + FILL,), 32767, dtype=torch.int16, device="cuda")
    buf[shift: shift + n_clips * n] = torch.from_numpy(np.array(clips, np.int16).reshape(-1)).cuda()
    d_x = torch.empty((n_clips, plan.kmax - plan.kmin, 2), dtype=torch.float32, device="cuda")
    g.stage_spectrum_dev(buf.data_ptr() + 2 * shift, n, n_clips, d_x.data_ptr())
    torch.cuda.synchronize()
    return d_x.cpu().numpy()


def _tables(g, plan, n):
    """which of the device-generated tables differs from the oracle's (for a failure's message only)"""
    for which, name in enumerate(("w", "T_L", "Bhat", "w[k]/L")):
        if not np.array_equal(g.chirpz_table(n, which).view(np.uint64), plan.chirpz_table(which).view(np.uint64)):
            return f"table {name} differs"
    return "tables equal"


def _check(g, torch, plan, n, clips, want, kinds, shift=0):
    got = _spectrum(g, torch, plan, clips, shift)
    for i, kind in enumerate(kinds):
        if not bits_equal(got[i], want[i]):
            bad = np.nonzero((got[i].view(np.uint32) != want[i].view(np.uint32)).any(axis=1))[0]
            pytest.fail(f"n = {n}, {bz_ref.shape(n)}, {kind} clip, shift {shift}: {bad.size} of {want[i].shape[0]} bins differ, "
                        f"first at k = {plan.kmin + int(bad[0])}, last at {plan.kmin + int(bad[-1])}; {_tables(g, plan, n)}")
    return got


@pytest.mark.parametrize("n", SWEEP)
def test_sweep(gpu, torch_cuda, oracle, filters, n):
    if n > ONE_CLIP_ABOVE:
        clip = bz_ref.rail_clip(n)
        plan = oracle.Plan(n)
        clips, want, kinds, shift = clip[None], [plan.spectrum(clip)], ("rail",), 1
    else:
        clips, plan, want = _case(oracle, n)
        kinds, shift = ("noise", "rail"), 0
    geo = gpu.geometry(n)
    s = bz_ref.shape(n)
    assert (geo.n1, geo.n2) == (plan.n1, plan.n2) == (s.n1, bz_ref.N2)
    assert (geo.kmin, geo.kmax, geo.m, geo.c, geo.n_hp) == (plan.kmin, plan.kmax, plan.m, plan.c, plan.n_hp)
    _check(gpu, torch_cuda, plan, n, clips, want, kinds, shift)
    if n <= EXTRACT_UP_TO:
        hp = gpu.extract(clips)
        assert plan.n_hp >= 1
        for i, kind in enumerate(kinds):
            assert np.array_equal(hp[i], plan.extract(filters, clips[i])), (n, kind)


# a = 1, the a = 16 exact fit (an even length: only the shift brings its clips to a 2-byte boundary) and a = 17; at an odd
# length the second clip starts on the other boundary than the first
@pytest.mark.parametrize("n,shift", [(n, s) for n in (A1, A16_EXACT, A17) for s in (0, 1)])
def test_load_alignment(gpu, torch_cuda, oracle, n, shift):
    assert bz_ref.shape(A1).a == 1 and bz_ref.shape(A17).a == 17
    assert (bz_ref.shape(A16_EXACT).a, bz_ref.shape(A16_EXACT).slack, A16_EXACT % 2) == (16, 0, 0)
    clips, plan, want = _case(oracle, n)
    _check(gpu, torch_cuda, plan, n, clips, want, ("noise", "rail"), shift)


@pytest.mark.parametrize("n", [A1, A17])
def test_clip_counts(gpu, torch_cuda, oracle, n):
    """1, 3 and 5 clips in one call, in one pass and in passes of two: every clip as when it is alone"""
    clips2, plan, want2 = _case(oracle, n)
    rng = np.random.default_rng(n + 2)
    clips = np.concatenate([clips2, rng.integers(-32768, 32768, (3, n)).astype(np.int16)])
    alone = [_spectrum(gpu, torch_cuda, plan, clips[i:i + 1])[0] for i in range(5)]
    for i in range(2):
        assert bits_equal(alone[i], want2[i]), (n, 1, i)
    try:
        for batch in (0, 2):
            gpu.set_batch(batch)
            for n_clips in (1, 3, 5):
                got = _spectrum(gpu, torch_cuda, plan, clips[:n_clips])
                for i in range(n_clips):
                    assert bits_equal(got[i], alone[i]), (n, batch, n_clips, i)
    finally:
        gpu.set_batch(0)


def test_forced_on_a_smooth_length(torch_cuda, oracle, monkeypatch):
    """HPFW_FORCE_BLUESTEIN=1 on the 7-smooth length whose convolution has the least slack (no 7-smooth length with
    a <= 17 fits exactly: tests/test_bz_host.py)"""
    n, slack = bz_ref.forced_smooth_length()
    assert bz_ref.is_smooth(n) and bz_ref.shape(n).slack == slack
    monkeypatch.setenv("HPFW_FORCE_BLUESTEIN", "1")                 # read when the plan of a length is built
    g = hpfw_amd.Gpu(0)
    try:
        plan = oracle.Plan(n, force_bluestein=True)
        geo = g.geometry(n)
        assert (geo.n1, geo.n2) == (plan.n1, plan.n2) == (bz_ref.shape(n).n1, bz_ref.N2)
        clips = np.stack([bz_ref.noise_clip(n), bz_ref.rail_clip(n)])
        want = [plan.spectrum(c) for c in clips]
        for shift in (0, 1):
            _check(g, torch_cuda, plan, n, clips, want, ("noise", "rail"), shift)
    finally:
        g.close()
