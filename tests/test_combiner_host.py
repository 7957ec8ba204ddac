"""CPU tests of the AudioCombiner surface: the C++ facade and its example compile and link, the WAV reader the facades
share, and the two checkers of tests/test_gpu_combiner.py against each other."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, synth

from combiner_ref import RefIndex, numpy_peaks, expected_topk, NONE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_combiner_example_compiles_and_links(tmp_path):
    """include/hpfw/gpu/audio_combiner.h (header-only over the C-ABI) and examples/combine.cpp"""
    exe = tmp_path / "combine"
    cmd = ["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "combine.cpp"), "-o", str(exe),
           "-L", os.path.dirname(_lib.LIB_PATH), "-lhpfw_gpu", "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH),
           "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)   # no directory: usage, no device touched
    assert r.returncode == 2 and "usage" in r.stderr


def test_wav_reader_mono_and_stereo(tmp_path):
    x = synth.gen_clip(5, 2.0)
    mono = tmp_path / "mono.wav"
    synth.write_wav(str(mono), x)
    assert np.array_equal(_lib.wav_read(str(mono)), x)
    rng = np.random.default_rng(1)
    lr = rng.integers(-32768, 32768, size=(4001, 2)).astype(np.int16)
    lr[:4] = [[-3, 0], [3, 0], [-32768, -32767], [32767, 32766]]   # odd sums: the downmix truncates towards zero
    stereo = tmp_path / "stereo.wav"
    synth.write_wav(str(stereo), lr.ravel(), channels=2)
    want = np.fix((lr[:, 0].astype(np.int32) + lr[:, 1]) / 2).astype(np.int16)
    got = _lib.wav_read(str(stereo))
    assert np.array_equal(got, want)
    assert list(got[:4]) == [-1, 1, -32767, 32766]


def test_wav_reader_rejects_other_rates(tmp_path):
    data = np.arange(100, dtype=np.int16).tobytes()
    p = tmp_path / "48k.wav"
    with open(p, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, 48000, 96000, 2, 16))
        f.write(b"data" + struct.pack("<I", len(data)) + data)
    n = ctypes.c_int64(-1)
    rc = hpfw_amd.lib().hpfw_gpu_wav_read_pcm16(os.fsencode(str(p)), None, 0, ctypes.byref(n))
    assert rc == -6 and n.value == 0                     # HPFW_E_IO
    assert b"44100" in hpfw_amd.lib().hpfw_gpu_last_error()
    with pytest.raises(hpfw_amd.HpfwError):
        _lib.wav_read(str(p))
    rc = hpfw_amd.lib().hpfw_gpu_wav_read_pcm16(os.fsencode(str(tmp_path / "missing.wav")), None, 0, ctypes.byref(n))
    assert rc == -6


def _small_case(seed):
    rng = np.random.default_rng(seed)
    recs = [rng.integers(0, 12, size=int(rng.integers(0, 40))).astype(np.uint16) for _ in range(5)]
    q = rng.integers(0, 12, size=int(rng.integers(1, 50))).astype(np.uint16)
    return recs, q


@pytest.mark.parametrize("seed", range(12))
def test_checkers_agree(seed):
    """the restatement's final per-offset counts and the numpy diagonal counts give the same peaks"""
    recs, q = _small_case(seed)
    ref = RefIndex(recs)
    for ex in (-1, 0, 3):
        got = ref.peaks(q, ex)
        want = numpy_peaks(q, recs, ex)
        for j in range(len(recs)):
            assert tuple(want[j]) == (got.get(j, (0, 0))), (j, ex)
        res, cnt = ref.find(q, ex, counts=True)
        if res[0] != NONE:                                # the result never claims more than its bin holds
            assert res[2] <= res[1] == cnt[(res[0], res[3])]
        assert len(expected_topk(want, 8)) == 8


def test_restatement_on_a_hand_case():
    """combiner.h:100-132 by hand"""
    ref = RefIndex([np.array([1, 2, 3], np.uint16), np.array([1, 1, 2, 2], np.uint16)])
    # c=0: (0, 0) -> 1 sets {0, 1, 1, 0}; c=1: (0, 0) -> 2 > 1 gives {0, 2, 2, 0}; c=2: (0, 0) -> 3 gives {0, 3, 3, 0}
    assert ref.find(np.array([1, 2, 3], np.uint16)) == (0, 3, 3, 0)
    # without recording 0: c=0: (1, 0) -> 1 sets {1, 1, 1, 0}; c=1: (1, -1) -> 2 > 1 gives {1, 2, 2, -1}
    assert ref.find(np.array([1, 2, 3], np.uint16), exclude=0) == (1, 2, 2, -1)
    # a switch: c=0 (0, 0) -> 1 sets {0, 1, 1, 0}; c=1 (1, 0) -> 2 > 1 switches to {1, 2, 1, 0}; c=2 (1, 0) -> 3 > 1
    ref = RefIndex([np.array([5], np.uint16), np.array([5, 6, 7], np.uint16)])
    assert ref.find(np.array([5, 6, 7], np.uint16)) == (1, 3, 2, 0)
    assert ref.find(np.array([9], np.uint16)) == (NONE, 0, 0, 0)
