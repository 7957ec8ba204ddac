"""CPU tests of the time warp: the library's table against the numpy design of tests/warp_ref.py, the
quality of that table, and the C surface.  The library loads without a device; nothing here touches one."""
import ctypes
import os
import re

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib

import warp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
SYMS = ("hpfw_gpu_warp_table", "hpfw_gpu_warp_pcm16", "hpfw_gpu_warp_pcm16_host", "hpfw_gpu_mix_pcm16", "hpfw_gpu_mix_pcm16_host",
        "hpfw_gpu_drift_anchors", "hpfw_gpu_drift_fit", "hpfw_gpu_time_map_q40", "hpfw_gpu_wav_write_pcm16")


@pytest.fixture(scope="module")
def taps():
    return _lib.warp_table()


def test_entry_points_are_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hpfw_gpu.h")).read(), flags=re.S)
    for sym in SYMS:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTS and hasattr(hpfw_amd.lib(), sym)
    assert re.search(r"\}\s*hpfw_warp_track\s*;", header)
    assert _lib.WARP_TRACK_DTYPE.itemsize == 48
    for name in _lib.WARP_TRACK_DTYPE.names[:-1]:
        assert name in header


def test_table_is_the_numpy_design(taps):
    want = ref.design()
    assert taps.shape == want.shape == (ref.P, ref.T) == (4096, 32)
    # float64 sinc / Bessel I0 in C against numpy: equal, or 1 LSB apart in the places listed (none on the build this was
    # written on; the sample-rate conversion's tables differ in up to 8 places)
    diff = np.abs(taps.astype(np.int32) - want)
    places = np.argwhere(diff)
    assert diff.max(initial=0) <= 1 and len(places) <= 8, places
    t = taps.astype(np.int64)
    assert (t.sum(axis=1) == 1 << 14).all()
    assert (32768 * np.abs(t).sum(axis=1) < 1 << 31).all()
    impulse = np.zeros(ref.T, np.int16)
    impulse[ref.H - 1] = 1 << 14
    assert np.array_equal(taps[0], impulse)
    # row p is the fractional delay p / P: the centroid of a row (its delay at 0 Hz) lies p / P past tap H - 1
    centroid = (t * np.arange(ref.T)).sum(axis=1) / float(1 << 14)
    assert np.abs(centroid - (ref.H - 1 + np.arange(ref.P) / ref.P)).max() < 0.01


def test_table_arguments():
    L = hpfw_amd.lib()
    P, T = ctypes.c_int32(), ctypes.c_int32()
    assert L.hpfw_gpu_warp_table(None, 0, ctypes.byref(P), ctypes.byref(T)) == 0 and (P.value, T.value) == (ref.P, ref.T)
    assert L.hpfw_gpu_warp_table(None, 0, None, ctypes.byref(T)) == E_INVALID
    small = np.zeros(ref.P * ref.T - 1, np.int16)
    assert L.hpfw_gpu_warp_table(small.ctypes.data_as(ctypes.c_void_p), small.size, ctypes.byref(P), ctypes.byref(T)) == E_INVALID


def test_identity_map_copies_the_source(taps):
    x = np.random.default_rng(3).integers(-32768, 32768, 500).astype(np.int16)
    for i0 in (0, 7, -7):
        m = np.arange(600) + i0
        want = np.where((m >= 0) & (m < x.size), x[np.clip(m, 0, x.size - 1)], 0)
        assert np.array_equal(ref.warp(x, i0, 0, 0, 0, 600, 1, taps), want)


def _tone(f, n, amp=16000.0):
    return np.rint(amp * np.sin(2 * np.pi * f * np.arange(n) / 44100.0)).astype(np.int16)


def _fit(y, f, rate):
    """least-squares sinusoid at f on the warped time base (source samples per output: rate): (amplitude, SNR in dB)"""
    t = np.arange(y.size) * rate / 44100.0
    A = np.stack([np.sin(2 * np.pi * f * t), np.cos(2 * np.pi * f * t)], 1)
    c, *_ = np.linalg.lstsq(A, y, rcond=None)
    e = y - A @ c
    return float(np.hypot(*c)), 10 * np.log10(((A @ c) ** 2).mean() / (e ** 2).mean())


@pytest.mark.parametrize("ppm, f0", ((300, 0), (-300, 0), (0, (1 << 39) + 12345)))
def test_quality_of_the_library_table(taps, ppm, f0):
    """20 tones from 50 Hz to 0.8 x Nyquist through the library's taps: SNR (noise + distortion against the fitted tone)
    >= 65 dB, the pin of the sample-rate conversion, and the gain within 0.2 dB.  Measured with P = 4096, H = 16, cutoff 1:
    72.6 dB at the worst tone (17 640 Hz) at +-300 ppm, 88.7 dB at a fixed half-sample delay."""
    d = int(round(ppm * 1e-6 * 2 ** 40))
    n = 22050
    for f in np.linspace(50, 0.8 * 22050, 20):
        y = ref.warp(_tone(f, n), 0, f0, d, 0, n - 100, 1, taps).astype(np.float64)[400:-400]
        amp, snr = _fit(y, f, 1 + d / 2.0 ** 40)
        assert snr >= 65, (f, snr)
        assert abs(20 * np.log10(amp / 16000)) < 0.2, (f, amp)


def test_constant_input_gives_the_constant(taps):
    for c in (-32768, -1234, 0, 1, 32767):
        y = ref.warp(np.full(3000, c, np.int16), 5, 12345, 1 << 30, 0, 2900, 1, taps)
        assert (y[ref.T:-ref.T] == c).all()


def test_restatement_mix_and_gain_rules():
    x = np.array([-32768] * 100, np.int16)
    assert (ref.warp(x, 0, 0, 0, 0, 100, -1) == 32767).all() and (ref.warp(x, 0, 0, 0, 0, 100, 3) == -32768).all()
    ys = np.array([[100, -100, 32767], [50, 50, 32767]])
    assert list(ref.mix_tracks(ys, [1 << 15, -(1 << 14)])) == [75, -125, 16384]
    assert list(ref.mix_tracks(ys, [1 << 17, 1 << 17])) == [600, -200, 32767]
    assert list(ref.mix_tracks(ys[:1], [1])) == [0, 0, 1]           # (32767 + 2^14) >> 15
