"""The dB term of DESIGN.md S8 by table and short polynomial (db_spec.h db_term_fast) against the specified sequence, on
the device: every float bit pattern through hpfw_gpu_debug_db_term_sweep, and the kernels that use it -- cq_kernel, the
large-band path, db_kernel and the Mel dB kernel -- run both ways (HPFW_DB_TERM=spec at handle creation, and the default)."""
import math
import os

import numpy as np
import pytest

import db_term_ref as ref
from conftest import bits_equal

pytestmark = pytest.mark.gpu

import hpfw_amd  # noqa: E402
from hpfw_amd import synth  # noqa: E402
from hpfw_amd._lib import debug_db_term_sweep  # noqa: E402


def _handle(value, filters):
    """a fresh handle created under HPFW_DB_TERM = value (read at creation), None: unset"""
    old = os.environ.pop("HPFW_DB_TERM", None)
    if value is not None:
        os.environ["HPFW_DB_TERM"] = value
    try:
        g = hpfw_amd.Gpu(0)
    finally:
        os.environ.pop("HPFW_DB_TERM", None)
        if old is not None:
            os.environ["HPFW_DB_TERM"] = old
    g.set_filters(filters)
    return g


@pytest.fixture(scope="module")
def both(torch_cuda, filters):
    h = {"spec": _handle("spec", filters), "fast": _handle(None, filters)}
    yield h
    for g in h.values():
        g.close()


def test_every_bit_pattern(torch_cuda):
    """+0 .. +inf: no pattern differs, and the fallback is taken for exactly the patterns the host program counted (the
    same IEEE operations on both sides: a difference would be a finding about the device's arithmetic)"""
    rec = ref.recorded()["all"]
    bad, fell, first = debug_db_term_sweep(0, ref.INF + 1)
    print("all patterns:", bad, fell, first, "host:", rec["fallbacks"])
    assert (bad, first) == (0, None)
    assert fell == int(rec["fallbacks"])
    assert fell <= ref.CAP * (ref.INF - ref.LOWEST)
    # negative values and NaN take the specified sequence as they are
    assert debug_db_term_sweep(0x80000000 - 4096, 8192) == (0, 0, None)
    assert debug_db_term_sweep(0xFF800000 - 4096, 8192) == (0, 0, None)
    assert debug_db_term_sweep(2 ** 32 - 65536 - 7, 65536 + 7) == (0, 0, None)


def test_fallback_count_equals_the_host_programs(torch_cuda, tmp_path_factory):
    """on ranges the host program walks now: around p = 1 (where most fallbacks lie), across the 1e-10f clamp, a range
    that is no multiple of the sweep's block, and up to +inf"""
    exe = ref.build(tmp_path_factory)
    for first, count in ((0x3F000000, 1 << 24), (ref.LOWEST - 70001, 140003), (0x42C80000, 3 * 65536 + 17), (ref.INF - 99999, 100000)):
        host = ref.run(exe, "range", first, count)
        bad, fell, _ = debug_db_term_sweep(first, count)
        print(hex(first), count, "device:", bad, fell, "host:", host["mismatches"], host["fallbacks"])
        assert bad == 0 and int(host["mismatches"]) == 0
        assert fell == int(host["fallbacks"])


def test_fallback_share_of_a_log_uniform_input(torch_cuda):
    """p log-uniform in [1e-10, 1e6]: a pattern of mantissa m carries the measure log2(1 + ulp / m) <= 2^-23 / ln 2 of its
    binade's 1, so the fallbacks' share is at most their count times that, over the log2(1e16) binades of the range"""
    bad, fell, _ = debug_db_term_sweep(ref.LOWEST, ref.MILLION - ref.LOWEST)
    bound = fell * 2.0 ** -23 / math.log(2.0) / math.log2(1e16)
    print("log-uniform in [1e-10, 1e6]: fallbacks", fell, "share at most", bound)
    assert bad == 0
    assert bound <= ref.CAP


def _clips(n, n_clips=2):
    clips = np.stack([synth.gen_clip(2026 + i, n / synth.SR)[:n] for i in range(n_clips)])
    return np.concatenate([clips, np.zeros((1, n), np.int16)])      # ... and silence: every sample at the 1e-10f clamp


# the shortest admitted clip (chirp-z forward transform); 2 s; 60 s (bands longer than the LDS: k_cq_big.hip)
@pytest.mark.parametrize("n", [54254, 88200, 2646000])
def test_extraction_both_ways(both, torch_cuda, n):
    """hashprints of the whole extraction (cq_kernel's epilogue), the dB spectrogram of the stage entry point from PCM,
    and the one from magnitudes (db_kernel)"""
    torch = torch_cuda
    clips = _clips(n, 2 if n < 2_000_000 else 1)
    n_clips = clips.shape[0]
    hp, spec_pcm, spec_mag = {}, {}, {}
    for k, g in both.items():
        hp[k] = g.extract(clips)
        geo = g.geometry(n)
        d_pcm = torch.from_numpy(clips).cuda()
        d_db = torch.empty((n_clips, 121, geo.c), dtype=torch.float32, device="cuda")
        g.stage_spectrogram_dev(d_pcm.data_ptr(), n, n_clips, d_db.data_ptr())
        d_x = torch.empty((n_clips, geo.kmax - geo.kmin, 2), dtype=torch.float32, device="cuda")
        g.stage_spectrum_dev(d_pcm.data_ptr(), n, n_clips, d_x.data_ptr())
        d_mag = torch.empty_like(d_db)
        g.stage_cqmag_dev(d_x.data_ptr(), n, n_clips, d_mag.data_ptr())
        d_db2 = torch.empty_like(d_db)
        g.stage_db_dev(d_mag.data_ptr(), n_clips, geo.c, d_db2.data_ptr())
        torch.cuda.synchronize()
        spec_pcm[k], spec_mag[k] = d_db.cpu().numpy(), d_db2.cpu().numpy()
    assert hp["fast"].shape[1] > 0 and np.array_equal(hp["fast"], hp["spec"])
    assert bits_equal(spec_pcm["fast"], spec_pcm["spec"])
    assert bits_equal(spec_mag["fast"], spec_mag["spec"])
    assert (spec_pcm["fast"][-1] == 0.0).all()                     # silence: t = t_max = -100 everywhere
    assert spec_pcm["fast"][0].max() == 0.0 and spec_pcm["fast"][0].min() < -40.0


def test_mel_db_both_ways(both):
    clips = _clips(88200)
    mel = {k: g.mel_spectrogram(clips) for k, g in both.items()}
    assert len(mel["fast"]) == 3 and mel["fast"][0].shape[1] > 0
    for a, b in zip(mel["fast"], mel["spec"]):
        assert bits_equal(a, b)
