"""CPU tests of the sample-rate conversion to 44.1 kHz: lengths, the library's tap table against
the numpy design of tests/resample_ref.py, the quality of that table, the any-rate WAV reader, and the C / C++ surfaces
of the switch.  The library loads without a device; nothing here touches one."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, multi, synth

import resample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_IO = -1, -6


def test_lengths():
    assert hpfw_amd.resample_length(1_440_000, 48000) == 1_323_000
    assert hpfw_amd.resample_length(0, 48000) == 0
    assert hpfw_amd.resample_length(1, 48000) == 1
    assert hpfw_amd.resample_length(1, 8000) == 6                 # ceil(441 / 80)
    assert hpfw_amd.resample_length(12345, 44100) == 12345
    for fs in ref.RATES:
        for n in (1, 2, 999, 1_323_001, 26_460_000):
            assert hpfw_amd.resample_length(n, fs) == ref.out_length(n, fs)
    L = hpfw_amd.lib()
    out = ctypes.c_int64(-7)
    for bad in (7999, 192001, 0, -1):
        assert L.hpfw_gpu_resample_length(100, bad, ctypes.byref(out)) == E_INVALID
    assert L.hpfw_gpu_resample_length(-1, 48000, ctypes.byref(out)) == E_INVALID
    with pytest.raises(hpfw_amd.HpfwError):
        hpfw_amd.resample_length(100, 7999)


@pytest.mark.parametrize("fs", ref.RATES)
def test_table_matches_numpy_design(fs):
    L, M, taps = hpfw_amd.resample_table(fs)
    rL, rM, rtaps = ref.design(fs)
    assert (L, M, taps.shape) == (rL, rM, rtaps.shape)
    assert taps.shape[1] == 2 * ref.half_taps(fs)
    diff = np.abs(taps.astype(np.int32) - rtaps)
    assert diff.max() <= 1 and np.count_nonzero(diff) <= 8      # float64 sinc / Bessel I0 in C vs numpy
    assert (taps.astype(np.int64).sum(axis=1) == 1 << 14).all()
    assert (32768 * np.abs(taps.astype(np.int64)).sum(axis=1) < 1 << 31).all()


def test_table_identity_and_bad_rates():
    assert hpfw_amd.resample_table(44100)[:2] == (1, 1) and hpfw_amd.resample_table(44100)[2].size == 0
    L = hpfw_amd.lib()
    a, b, c = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    for bad in (7999, 192001, 0):
        assert L.hpfw_gpu_resample_table(bad, None, 0, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == E_INVALID
    small = np.zeros(4, np.int16)                                     # too small for the 48 kHz table
    assert L.hpfw_gpu_resample_table(48000, small.ctypes.data_as(ctypes.c_void_p), small.size, ctypes.byref(a),
                                     ctypes.byref(b), ctypes.byref(c)) == E_INVALID


def _tone(fs, f, n, amp=16000.0):
    return np.rint(amp * np.sin(2 * np.pi * f * np.arange(n) / fs)).astype(np.int16)


def _fit(y, f):
    """least-squares sinusoid at f (44.1 kHz time base): (its amplitude, SNR of y against it in dB)"""
    t = np.arange(y.size) / 44100.0
    A = np.stack([np.sin(2 * np.pi * f * t), np.cos(2 * np.pi * f * t)], 1)
    c, *_ = np.linalg.lstsq(A, y, rcond=None)
    e = y - A @ c
    return float(np.hypot(*c)), 10 * np.log10(((A @ c) ** 2).mean() / (e ** 2).mean())


@pytest.mark.parametrize("fs", ref.RATES)
def test_quality_of_the_library_table(fs):
    """passband: 20 tones up to 0.8 x the lower Nyquist, SNR (noise + distortion against the fitted tone) >= 65 dB and
    gain within 0.2 dB; stopband: tones in [44100 - 0.9 * 22050, fs / 2) come out >= 55 dB down"""
    _, _, taps = hpfw_amd.resample_table(fs)
    n = fs // 2
    lo = min(fs, 44100) / 2
    for f in np.linspace(50, 0.8 * lo, 20):
        y = ref.resample(_tone(fs, f, n), fs, taps).astype(np.float64)[400:-400]
        amp, snr = _fit(y, f)
        assert snr >= 65, (f, snr)
        assert abs(20 * np.log10(amp / 16000)) < 0.2, (f, amp)
    if fs / 2 > 44100 - 0.9 * 22050:
        for f in np.linspace(44100 - 0.9 * 22050, 0.999 * fs / 2, 5):
            y = ref.resample(_tone(fs, f, n), fs, taps).astype(np.float64)[400:-400]
            rej = 10 * np.log10((16000.0 ** 2 / 2) / max((y ** 2).mean(), 1e-12))
            assert rej >= 55, (f, rej)


@pytest.mark.parametrize("fs", (8000, 48000, 44056, 192000))
def test_constant_input_gives_the_constant(fs):
    _, _, taps = hpfw_amd.resample_table(fs)
    for c in (-32768, -1234, 0, 1, 32767):
        y = ref.resample(np.full(3000, c, np.int16), fs, taps)
        H = taps.shape[1] // 2
        edge = int(np.ceil((H + 1) * 44100 / fs)) + 1
        assert (y[edge:-edge] == c).all()


def _wav(path, raw, rate, channels=1, bits=16, fmt=1):
    data = np.ascontiguousarray(raw).tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<IHHIIHH", 16, fmt, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits))
        f.write(b"data" + struct.pack("<I", len(data)) + data)


def test_wav_read_any(tmp_path):
    rng = np.random.default_rng(7)
    x = rng.integers(-32768, 32768, size=4801).astype(np.int16)
    synth.write_wav(str(tmp_path / "m48.wav"), x, rate=48000)
    got, rate = hpfw_amd.wav_read_any(str(tmp_path / "m48.wav"))
    assert rate == 48000 and np.array_equal(got, x)
    lr = rng.integers(-32768, 32768, size=(1601, 2)).astype(np.int16)
    lr[:3] = [[-3, 0], [3, 0], [-32768, -32767]]
    synth.write_wav(str(tmp_path / "s16.wav"), lr.ravel(), channels=2, rate=16000)
    got, rate = hpfw_amd.wav_read_any(str(tmp_path / "s16.wav"))
    want = np.fix((lr[:, 0].astype(np.int32) + lr[:, 1]) / 2).astype(np.int16)  # the same truncating downmix
    assert rate == 16000 and np.array_equal(got, want) and list(got[:3]) == [-1, 1, -32767]
    synth.write_wav(str(tmp_path / "m44.wav"), x)
    got, rate = hpfw_amd.wav_read_any(str(tmp_path / "m44.wav"))
    assert rate == 44100 and np.array_equal(got, _lib.wav_read(str(tmp_path / "m44.wav")))
    # 48 kHz is still refused by the 44.1 kHz reader
    with pytest.raises(hpfw_amd.HpfwError):
        _lib.wav_read(str(tmp_path / "m48.wav"))


def test_wav_read_any_refuses_what_it_cannot_read(tmp_path):
    L = hpfw_amd.lib()
    n, rate = ctypes.c_int64(-1), ctypes.c_int32(-1)
    cases = {
        "24bit.wav": dict(raw=np.zeros(300, np.uint8), rate=48000, bits=24),
        "3ch.wav": dict(raw=np.zeros(300, np.int16), rate=48000, channels=3),
        "float.wav": dict(raw=np.zeros(100, np.float32), rate=48000, bits=32, fmt=3),
        "7k.wav": dict(raw=np.zeros(100, np.int16), rate=7000),
        "200k.wav": dict(raw=np.zeros(100, np.int16), rate=200000),
    }
    for name, kw in cases.items():
        _wav(tmp_path / name, **kw)
        assert L.hpfw_gpu_wav_read_pcm16_any(os.fsencode(str(tmp_path / name)), None, 0, ctypes.byref(n),
                                             ctypes.byref(rate)) == E_IO, name
        assert n.value == 0
    assert L.hpfw_gpu_wav_read_pcm16_any(os.fsencode(str(tmp_path / "missing.wav")), None, 0, ctypes.byref(n),
                                         ctypes.byref(rate)) == E_IO


def test_switch_entry_points_are_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hpfw_gpu.h")).read(), flags=re.S)
    for sym in ("hpfw_gpu_resample_length", "hpfw_gpu_resample_table", "hpfw_gpu_resample_pcm16",
                "hpfw_gpu_resample_pcm16_host", "hpfw_gpu_wav_read_pcm16_any", "hpfw_gpu_collector_set_resample"):
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTS and hasattr(hpfw_amd.lib(), sym)
    assert hpfw_amd.lib().hpfw_gpu_collector_set_resample(None, 1) == E_INVALID
    mh = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hpfw_gpu_multi_resample.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(hpfw_gpu_group_\w+)\s*\(", mh)) == set(multi.RESAMPLE_EXPORTS)
    M = multi.lib()
    assert all(hasattr(M, s) for s in multi.RESAMPLE_EXPORTS)
    assert M.hpfw_gpu_group_set_resample(None, 1) == E_INVALID


FACADES = r"""
#include <hpfw/gpu/audio_combiner.h>
#include <hpfw/gpu/gpu_collector.h>
#include <hpfw_gpu_multi_resample.h>
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    hpfw::GpuCollector c;
    c.set_resample(true);
    hpfw::GpuAudioCombiner a;
    a.set_resample(true);
    return hpfw_gpu_group_set_resample(nullptr, 1) == HPFW_E_INVALID ? 0 : 1;
}
"""


def test_facades_with_the_switch_compile_and_link(tmp_path):
    src = tmp_path / "facades.cpp"
    src.write_text(FACADES)
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(tmp_path / "facades"), "-L", lib_dir, "-lhpfw_gpu_multi", "-lhpfw_gpu", "-Wl,-rpath," + lib_dir,
           "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "facades")], capture_output=True, text=True)   # no argument: no device touched
    assert r.returncode == 2
