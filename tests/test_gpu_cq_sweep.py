"""The constant-Q stage on the GPU at every chirp-z class the planner admits, 256 .. 2^19 points (tests/cq_ref.py LENGTHS;
tests/test_cq_host.py asserts the coverage): the stage entry fed seeded forward bins, its magnitudes bit-identical to the
oracle's from the same bins AND within the project's 1e-4 of float64, its dB values identical.  Classes up to 16384 run in
LDS (k_cq.hip); above, `outer` = 1, 2, 3 radix-4 passes through global memory surround LDS blocks of 3072 .. 8192 points
(k_cq_big.hip).  Then one 600 s clip through both layouts of the forward bins, whose indices pass 2^21.

Full extraction of clips above 180 s is NOT compared with the oracle anywhere: the oracle's forward transform takes a
minute of CPU time at 600 s and four at 20 minutes.  What is pinned above 180 s: the constant-Q and dB stages against the
oracle from given bins at every class (here), the host tables (tests/test_library.py), the forward bins at 600 s against
float64, and the identity of extraction's front end with the chain of stage entries at 600 s."""
import time

import numpy as np
import pytest

import cols_ref
import cq_ref
from conftest import bits_equal, ulp_diff
from test_cols_host import FLOAT64_BAR
from test_cq_host import BAR, ROWS_LENGTH

pytestmark = pytest.mark.gpu


def _per_class(n, got, want):
    """which classes differ, for the failure message: {p: (values that differ, largest ulp)}"""
    out = {}
    for p, (outer, len0, bands) in cq_ref.classes(n).items():
        d = ulp_diff(got[bands], want[bands])
        if d.max() > 0:
            out[p] = (f"outer {outer}, len0 {len0}", int((d > 0).sum()), int(d.max()))
    return out


def _float64_error(mag, x, kmin, n, bands):
    want = cq_ref.cq_from_bins(x[:, 0].astype(np.float64) + 1j * x[:, 1], kmin, n, bands)
    return float((np.abs(mag[bands] - want).max(axis=1) / want.max(axis=1)).max())


@pytest.mark.parametrize("n", cq_ref.LENGTHS)
def test_every_class_from_given_bins(gpu, torch_cuda, oracle, n):
    """two clips of different seeds up to 240 s (the clip pitch of the work buffer and of the grid's z index in the
    global-memory passes), one above.  The float64 side is the first and the last band of every class; measured on an
    MI355X, in the order of LENGTHS (worse clip): 2.9e-7, 2.1e-7, 2.4e-7, 3.2e-7, 2.6e-7, 2.4e-7, 6.3e-7 -- the oracle's own
    figures on those bands, as the magnitudes are its bits."""
    torch = torch_cuda
    t0 = time.time()
    plan = oracle.Plan(n)
    geo = gpu.geometry(n)
    assert (geo.kmin, geo.kmax, geo.m, geo.c) == (plan.kmin, plan.kmax, plan.m, plan.c) == cq_ref.extent(n)
    n_clips = 2 if n <= 10584000 else 1
    nk = plan.kmax - plan.kmin
    x = np.stack([cq_ref.bins(n, nk, n + i) for i in range(n_clips)])
    d_x = torch.from_numpy(x).cuda()
    d_mag = torch.empty((n_clips, cq_ref.BINS, plan.c), dtype=torch.float32, device="cuda")
    gpu.stage_cqmag_dev(d_x.data_ptr(), n, n_clips, d_mag.data_ptr())
    d_db = torch.empty_like(d_mag)
    gpu.stage_db_dev(d_mag.data_ptr(), n_clips, plan.c, d_db.data_ptr())
    torch.cuda.synchronize()
    t_gpu = time.time() - t0
    mag, db = d_mag.cpu().numpy(), d_db.cpu().numpy()
    bands = cq_ref.first_and_last_bands(n)
    for i in range(n_clips):
        want = plan.cqmag(x[i])
        assert bits_equal(mag[i], want), (n, i, _per_class(n, mag[i], want))
        err = _float64_error(mag[i], x[i], plan.kmin, n, bands)
        print(f"n = {n}, clip {i}: {sorted(cq_ref.classes(n))} against float64 {err:.3g} over {len(bands)} bands")
        assert err < BAR, (n, i, err)
        want_db = oracle.db(want)
        assert bits_equal(db[i], want_db), (n, i, int((db[i].view(np.uint32) != want_db.view(np.uint32)).sum()))
    print(f"n = {n}: {time.time() - t0:.1f} s, of which plan and GPU {t_gpu:.1f} s")


def test_rows_layout_past_bin_2_21(gpu, torch_cuda, oracle):
    """600 s = 4200 x 6300, bins 76219 .. 2584099, classes 65536 .. 196608 (outer = 2 and 3).  Path A: forward bins
    gathered into natural order, the constant-Q stage entry, the dB stage entry -- the path test_every_class_from_given_bins
    pins, and pinned here again against the oracle from the same bins.  Path B: extraction's front end, which reads the
    rows layout x[k mod n1][k / n1 - q0] through XsView and XsBandRows and stores dB terms from the last global-memory
    pass.  A and B are bit-identical (tests/test_gpu_parity.py test_stages_bit_exact asserts the same up to 30 s, through
    the oracle).  Path A's input is anchored to float64: the oracle's own forward bins of this clip, computed once on a
    CPU (60 s; not part of any test), lie 8.4e-8 from np.fft.rfft, below tests/test_cols_host.py FLOAT64_BAR = 4e-7, so
    that bar is asserted (measured on an MI355X: 8.4e-8, the same).  Full extraction at this length is not compared with
    the oracle: its forward transform alone takes a minute."""
    torch = torch_cuda
    t0 = time.time()
    n = ROWS_LENGTH
    geo = gpu.geometry(n)
    kmin, kmax, m, c = cq_ref.extent(n)
    assert (geo.n1, geo.n2) == cols_ref.split(n) == (4200, 6300)
    assert (geo.kmin, geo.kmax, geo.m, geo.c) == (kmin, kmax, m, c) and kmax > 2 ** 21
    clip = cols_ref.noise_clip(n)
    d_pcm = torch.from_numpy(clip[None]).cuda()
    d_x = torch.empty((1, kmax - kmin, 2), dtype=torch.float32, device="cuda")
    gpu.stage_spectrum_dev(d_pcm.data_ptr(), n, 1, d_x.data_ptr())
    d_mag = torch.empty((1, cq_ref.BINS, c), dtype=torch.float32, device="cuda")
    gpu.stage_cqmag_dev(d_x.data_ptr(), n, 1, d_mag.data_ptr())
    d_a = torch.empty_like(d_mag)
    gpu.stage_db_dev(d_mag.data_ptr(), 1, c, d_a.data_ptr())
    d_b = torch.empty_like(d_mag)
    gpu.stage_spectrogram_dev(d_pcm.data_ptr(), n, 1, d_b.data_ptr())
    torch.cuda.synchronize()
    t_gpu = time.time() - t0
    x, mag, a, b = d_x.cpu().numpy()[0], d_mag.cpu().numpy()[0], d_a.cpu().numpy()[0], d_b.cpu().numpy()[0]
    err = cols_ref.float64_error(x, clip, kmin, kmax)
    print(f"n = {n}: forward bins against float64 {err:.3g}")
    assert err < FLOAT64_BAR, err
    assert bits_equal(a, b), _per_class(n, a, b)
    plan = oracle.Plan(n)
    want = plan.cqmag(x)
    assert bits_equal(mag, want), _per_class(n, mag, want)
    assert bits_equal(a, oracle.db(want))
    err = _float64_error(mag, x, kmin, n, cq_ref.first_and_last_bands(n))
    print(f"n = {n}: magnitudes against float64 {err:.3g}; {time.time() - t0:.1f} s, of which GPU {t_gpu:.1f} s")
    assert err < BAR, err
