"""What the row stage leaves out (HPFW_PRUNE bit 0, read at handle creation): the last group's outputs outside the consumed
windows.  A handle with it on and one with it off, in one process: forward bins, dB spectrogram and hashprints are the
same bits, and those of the default are the oracle's.  The host side is tests/test_prune_host.py."""
import os

import numpy as np
import pytest

from conftest import bits_equal

pytestmark = pytest.mark.gpu

import hpfw_amd  # noqa: E402
from hpfw_amd import synth  # noqa: E402

MASKS = ("1", "0")


def _handle(value, filters):
    """a fresh handle created under HPFW_PRUNE = value"""
    old = os.environ.pop("HPFW_PRUNE", None)
    os.environ["HPFW_PRUNE"] = value
    try:
        g = hpfw_amd.Gpu(0)
    finally:
        os.environ.pop("HPFW_PRUNE", None)
        if old is not None:
            os.environ["HPFW_PRUNE"] = old
    g.set_filters(filters)
    return g


@pytest.fixture(scope="module")
def handles(torch_cuda, filters):
    h = {m: _handle(m, filters) for m in MASKS}
    yield h
    for g in h.values():
        g.close()


def _stages(torch, g, clips):
    """(forward bins, dB spectrogram, hashprints) of a batch"""
    n_clips, n = clips.shape
    geo = g.geometry(n)
    d_pcm = torch.from_numpy(clips).cuda()
    d_x = torch.empty((n_clips, geo.kmax - geo.kmin, 2), dtype=torch.float32, device="cuda")
    g.stage_spectrum_dev(d_pcm.data_ptr(), n, n_clips, d_x.data_ptr())
    d_db = torch.empty((n_clips, 121, geo.c), dtype=torch.float32, device="cuda")
    g.stage_spectrogram_dev(d_pcm.data_ptr(), n, n_clips, d_db.data_ptr())
    torch.cuda.synchronize()
    return d_x.cpu().numpy(), d_db.cpu().numpy(), g.extract(clips)


# 2 s (n1 = 14) with 1, 3 and 5 clips, 5 s and 30 s: n2 = 6300, the pruned row kernel; 3.5 s: n2 = 6174, the run-time
# group sequence; 88 201 samples: the chirp-z forward transform (neither has a pruned instantiation: unchanged)
@pytest.mark.parametrize("n,n_clips,n2", [(88200, 1, 6300), (88200, 3, 6300), (88200, 5, 6300), (1323000, 1, 6300), (220500, 2, 6300),
                                          (154350, 2, 6174), (88201, 2, None)])
def test_pruned_equals_full_equals_oracle(handles, torch_cuda, oracle, filters, n, n_clips, n2):
    clips = np.stack([synth.gen_clip(4100 + i, n / synth.SR + 0.01)[:n] for i in range(n_clips)])
    if n2 is not None:
        assert handles["1"].geometry(n).n2 == n2
    got = {m: _stages(torch_cuda, g, clips) for m, g in handles.items()}
    x, db, hp = got["1"]
    assert hp.shape[1] > 0 and np.isfinite(x).all()
    for m in MASKS[1:]:
        assert bits_equal(got[m][0], x), "forward bins, HPFW_PRUNE=%s" % m
        assert bits_equal(got[m][1], db), "dB spectrogram, HPFW_PRUNE=%s" % m
        assert np.array_equal(got[m][2], hp), "hashprints, HPFW_PRUNE=%s" % m
    # the oracle on the first clip (the handles agree on the others)
    plan = oracle.Plan(n)
    x_ref = plan.spectrum(clips[0])
    assert bits_equal(x[0], x_ref)
    assert bits_equal(db[0], oracle.db(plan.cqmag(x_ref)))
    assert np.array_equal(hp[0], plan.extract(filters, clips[0]))
