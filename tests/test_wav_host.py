"""The parsers of files the user supplies -- the RIFF/WAVE reader (hpfw_amd/csrc/wav_file.cpp) and the cache's matrix
images (cache_files.cpp) -- as a stand-alone host program (tests/emu/wav_check.cpp) under AddressSanitizer and UBSan, on
well-formed and malformed files: the samples numpy expects, or the expected message.  One chunk walk serves every entry
point, so what holds here holds for calc_hashprint, calc_hashprints and prepare alike."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hpfw_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "emu", "wav_check.cpp"), os.path.join(CSRC, "wav_file.cpp"), os.path.join(CSRC, "cache_files.cpp")]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("wav") / "wav_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, "-o", out, *SOURCES]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr[-3000:]
    return r.stdout.strip()


def _read(exe, tmp_path, blob, any_rate=False):
    """the program's answer for a file of these bytes: (rate, samples) or the message"""
    p, out = tmp_path / "in.wav", tmp_path / "out.bin"
    p.write_bytes(blob)
    line = _run(exe, "wav", p, out, *(["any"] if any_rate else []))
    if line.startswith("error: "):
        return line[len("error: "):].replace(str(p), "<file>")
    ok, rate, n = line.split()
    pcm = np.fromfile(out, np.int16)
    assert ok == "ok" and pcm.size == int(n)
    return int(rate), pcm


def _fmt(channels=1, rate=44100, size=16):
    body = struct.pack("<HHIIHH", 1, channels, rate, rate * 2 * channels, 2 * channels, 16)
    return b"fmt " + struct.pack("<I", size) + body + b"\0" * (size - 16 + (size & 1) if size > 16 else 0)


def _wav(chunks):
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


def _data(pcm, size=None):
    raw = np.ascontiguousarray(pcm, np.int16).tobytes()
    return b"data" + struct.pack("<I", len(raw) if size is None else size) + raw


X = np.random.default_rng(3).integers(-32768, 32768, 1001).astype(np.int16)
NO_DATA = "<file>: no data chunk"


def test_mono_and_stereo(exe, tmp_path):
    rate, got = _read(exe, tmp_path, _wav(_fmt() + _data(X)))
    assert rate == 44100 and np.array_equal(got, X)
    lr = np.random.default_rng(1).integers(-32768, 32768, size=(4001, 2)).astype(np.int16)
    lr[:4] = [[-3, 0], [3, 0], [-32768, -32767], [32767, 32766]]   # odd sums: the downmix truncates towards zero
    _, got = _read(exe, tmp_path, _wav(_fmt(channels=2) + _data(lr.ravel())))
    assert np.array_equal(got, np.fix((lr[:, 0].astype(np.int32) + lr[:, 1]) / 2).astype(np.int16))
    assert list(got[:4]) == [-1, 1, -32767, 32766]


def test_rates(exe, tmp_path):
    blob = _wav(_fmt(rate=48000) + _data(X))
    assert _read(exe, tmp_path, blob) == "<file>: only PCM16 mono/stereo at 44100 Hz is supported"
    rate, got = _read(exe, tmp_path, blob, any_rate=True)
    assert rate == 48000 and np.array_equal(got, X)
    assert _read(exe, tmp_path, _wav(_fmt(rate=7999) + _data(X)), any_rate=True) == "<file>: only PCM16 mono/stereo at 8000..192000 Hz is supported"


def test_extensible_header_odd_list_chunk_and_streamed_size(exe, tmp_path):
    """the file of test_gpu_api.py::test_stereo_and_unsupported_wav"""
    fmt = struct.pack("<HHIIHHHHIH", 0xFFFE, 1, 44100, 88200, 2, 16, 22, 16, 4, 1) + bytes.fromhex("000000001000800000aa00389b71")
    blob = _wav(b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"LIST" + struct.pack("<I", 5) + b"INFOx" + b"\0" + _data(X, 0xFFFFFFFF))
    rate, got = _read(exe, tmp_path, blob)
    assert rate == 44100 and np.array_equal(got, X)
    _, got = _read(exe, tmp_path, _wav(_fmt() + _data(X, 0)))          # a size of 0 is a streamed file too
    assert np.array_equal(got, X)


def test_data_size_beyond_the_file_and_odd_trailing_byte(exe, tmp_path):
    _, got = _read(exe, tmp_path, _wav(_fmt() + _data(X, 2 * X.size + 1000)))
    assert np.array_equal(got, X)
    _, got = _read(exe, tmp_path, _wav(_fmt() + _data(X, 2 * X.size + 1) + b"\x7f"))
    assert np.array_equal(got, X)
    _, got = _read(exe, tmp_path, _wav(_fmt(channels=2) + _data(X[:999])))   # stereo: a trailing half frame is dropped
    assert got.size == 499


@pytest.mark.parametrize("size", [15, 4097])
def test_fmt_chunk_of_an_unsupported_size(exe, tmp_path, size):
    blob = _wav(b"fmt " + struct.pack("<I", size) + b"\1\0\1\0" + b"\0" * (size - 4 + (size & 1)) + _data(X))
    assert _read(exe, tmp_path, blob) == NO_DATA
    if size == 15:                                                        # 16 and 4096 are the supported ends
        assert np.array_equal(_read(exe, tmp_path, _wav(_fmt(size=16) + _data(X)))[1], X)
    else:
        assert np.array_equal(_read(exe, tmp_path, _wav(_fmt(size=4096) + _data(X)))[1], X)


def test_truncated_files(exe, tmp_path):
    whole = _wav(_fmt() + _data(X))
    assert _read(exe, tmp_path, whole[:12 + 24 + 5]) == NO_DATA           # cut inside the data chunk's header
    assert _read(exe, tmp_path, whole[:12 + 4]) == NO_DATA                # ... inside the fmt chunk's header
    assert _read(exe, tmp_path, whole[:12 + 8 + 9]) == NO_DATA            # ... inside the fmt chunk
    assert _read(exe, tmp_path, b"RIFF0000WAVEjunk") == NO_DATA
    assert _read(exe, tmp_path, whole[:11]) == "<file>: not a RIFF/WAVE file"
    rate, got = _read(exe, tmp_path, whole[:12 + 24 + 8])                 # a data chunk with nothing behind it
    assert got.size == 0


def test_chunk_of_size_0xffffffff_is_stepped_over(exe, tmp_path):
    """a non-data chunk that claims 4 GiB: the walk leaves the file and ends with "no data chunk" (a 32-bit skip would wrap
    to 0 and parse the chunk's body -- here a well-formed data chunk -- as headers)"""
    blob = _wav(_fmt() + b"LIST" + struct.pack("<I", 0xFFFFFFFF) + _data(X))
    assert _read(exe, tmp_path, blob) == NO_DATA


def _load(exe, tmp_path, blob):
    p, out = tmp_path / "spectro", tmp_path / "spectro.out"
    p.write_bytes(blob)
    line = _run(exe, "load", p, out)
    if line == "rejected":
        return None
    return np.fromfile(out, np.float32).reshape(int(line.split()[1]), 121)


def test_spectrogram_image_round_trip(exe, tmp_path):
    s = np.random.default_rng(5).uniform(-80, 0, (121, 37)).astype(np.float32)        # bin-major, as on the device
    src, img = tmp_path / "binmajor.bin", tmp_path / "img"
    s.tofile(src)
    _run(exe, "save", src, 37, img)
    raw = img.read_bytes()
    assert raw == np.array([121, 37], np.int32).tobytes() + np.ascontiguousarray(s.T).tobytes()   # element (b, c) at b + 121 c
    got = _load(exe, tmp_path, raw)
    assert got is not None and np.array_equal(got.view(np.uint32), s.T.view(np.uint32))


def test_spectrogram_images_that_are_rejected(exe, tmp_path):
    def image(rows, cols, floats):
        return np.array([rows, cols], np.int32).tobytes() + np.zeros(floats, np.float32).tobytes()
    assert _load(exe, tmp_path, image(121, 5, 121 * 5)) is not None
    assert _load(exe, tmp_path, image(121, 0, 0)).shape == (0, 121)
    assert _load(exe, tmp_path, image(120, 5, 120 * 5)) is None                    # wrong rows
    assert _load(exe, tmp_path, image(121, -1, 0)) is None                         # negative cols
    assert _load(exe, tmp_path, image(121, (1 << 24) + 1, 0)) is None              # cols above 2^24
    assert _load(exe, tmp_path, image(121, 5, 121 * 5 - 1)) is None                # shorter than its header claims
    assert _load(exe, tmp_path, image(121, 5, 121 * 5 + 1)) is None                # longer
    assert _load(exe, tmp_path, image(121, 5, 121 * 5)[:6]) is None                # cut inside the header
