"""CPU tests of live feeds at other rates than 44.1 kHz: the new entry points are declared and exported,
hpfw_gpu_streams_emitted against the formula in Python integers, the room as its inverse, bad rates refused before any device
is touched, the C++ facade with the new options, and a numpy restatement of the chunked conversion -- a history of T - 1
samples and the count of outputs given so far -- against resample_ref.resample of the whole feed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib

import resample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
SYMS = ("hpfw_gpu_streams_create_rates", "hpfw_gpu_streams_rates", "hpfw_gpu_streams_emitted")
WIN, HOP = 220500, 110250


def emitted(n, fs):
    """the formula of the contract in Python integers"""
    if fs == ref.OUT_RATE:
        return n
    L, M = ref.ratio(fs)
    H = ref.half_taps(fs)
    return 0 if n <= H else -(-(n - H) * L // M)


class ChunkedResampler:
    """The chunked form restated: the last T - 1 input samples and emitted.  push(chunk) returns the outputs the chunk
    completes, y[emitted(n_old) .. emitted(n_old + len(chunk)))."""

    def __init__(self, fs, taps=None):
        self.fs = fs
        (self.L, self.M), self.H = ref.ratio(fs), ref.half_taps(fs)
        self.h = (ref.design(fs)[2] if taps is None else np.asarray(taps)).astype(np.int64)
        self.hist = np.zeros(2 * self.H - 1, np.int64)                         # inputs n - (T - 1) .. n - 1, zeros in front of 0
        self.n = self.emitted = 0

    def push(self, chunk):
        L, M, H, T = self.L, self.M, self.H, 2 * self.H
        x = np.concatenate([self.hist, np.asarray(chunk, np.int16).astype(np.int64)])   # x[j] is input n_old - (T - 1) + j
        n_new = self.n + len(chunk)
        m1 = 0 if n_new <= H else -(-(n_new - H) * L // M)
        m = np.arange(self.emitted, m1, dtype=np.int64)                          # (m M < 2^63 for any feed of this suite)
        i0, p = m * M // L, m * M % L
        first = i0 - H + 1 - (self.n - (T - 1))                                  # the first tap's sample in x
        assert m.size == 0 or (first.min() >= 0 and first.max() + T <= x.size)
        acc = np.zeros(m.size, np.int64)
        for j in range(T):
            acc += x[first + j] * self.h[p, j]
        self.hist = x[x.size - (T - 1):]
        self.n, self.emitted = n_new, m1
        return np.clip((acc + (1 << (ref.SHIFT - 1))) >> ref.SHIFT, -32768, 32767).astype(np.int16)


def test_entry_points_are_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hpfw_gpu.h")).read(), flags=re.S)
    for sym in SYMS:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTS and hasattr(hpfw_amd.lib(), sym)
    assert ctypes.sizeof(_lib.StreamsParams) == 56 and ctypes.sizeof(_lib.StreamsInfo) == 40      # the old layouts stand


@pytest.mark.parametrize("fs", ref.RATES + (44100,))
def test_emitted_equals_the_formula(fs):
    H = ref.half_taps(fs) if fs != 44100 else 0
    L, M = ref.ratio(fs)
    for n in list(range(0, 6 * H + 5)) + [2 ** 40 + k for k in (-1, 0, 1, 2, 7, M, M + 1, 12345)]:
        got = _lib.streams_emitted(n, fs)
        assert got == emitted(n, fs), (fs, n)
        if fs == 44100:
            assert got == n
    # H zero samples behind a feed bring out what the file gives
    for n in (0, 1, H, 4095, 3 * fs + 7):
        assert _lib.streams_emitted(n + H, fs) == ref.out_length(n, fs) == hpfw_amd.resample_length(n, fs)
    # an output is final exactly when the last input it reads has arrived
    for n in (H + 1, H + 2, 2 * H + 3, 5000, 2 ** 40 + 3):
        m = emitted(n, fs)
        assert (m - 1) * M // L + H <= n - 1 < m * M // L + H or fs == 44100


@pytest.mark.parametrize("fs", ref.RATES + (44100,))
def test_room_is_the_inverse_of_emitted(fs):
    H = ref.half_taps(fs) if fs != 44100 else 0
    L, M = ref.ratio(fs)
    for X in (0, 1, 2, 146, 147, 4999, 220500, 225500, 441000, 2 ** 40 + 11):
        n = H + X * M // L
        assert _lib.streams_emitted(n, fs) <= X < _lib.streams_emitted(n + 1, fs), (fs, X)


def test_bad_rates_are_refused_without_a_device():
    L = hpfw_amd.lib()
    n = ctypes.c_int64()
    for bad in (7999, 192001, 0, -44100):
        assert L.hpfw_gpu_streams_emitted(10, bad, ctypes.byref(n)) == E_INVALID
    assert L.hpfw_gpu_streams_emitted(-1, 48000, ctypes.byref(n)) == E_INVALID
    assert L.hpfw_gpu_streams_emitted(10, 48000, None) == E_INVALID
    assert L.hpfw_gpu_streams_rates(None, None, None) == E_INVALID
    p = _lib.StreamsParams(3, 0, 0, 0, WIN, HOP, 0, None, None)
    out = ctypes.c_void_p()
    for rates, feed in (([48000, 7999, 192001], 1), ([192001, 44100, 44100], 0), ([44100, 48000, -1], 2)):
        r = np.array(rates, np.int32)
        assert L.hpfw_gpu_streams_create_rates(None, ctypes.byref(p), _lib._hp(r), ctypes.byref(out)) == E_UNSUPPORTED   # a NULL handle too
        assert out.value is None and f"feed {feed}".encode() in L.hpfw_gpu_last_error(), rates
    good = np.array([48000, 44100, 8000], np.int32)
    for rates in (None, _lib._hp(good)):                                      # good rates: the checks that were there, in their order
        assert L.hpfw_gpu_streams_create_rates(None, ctypes.byref(p), rates, ctypes.byref(out)) == E_INVALID
        assert b"null handle" in L.hpfw_gpu_last_error()
    bad_n = _lib.StreamsParams(0, 0, 0, 0, WIN, HOP, 0, None, None)
    assert L.hpfw_gpu_streams_create_rates(None, ctypes.byref(bad_n), _lib._hp(good), ctypes.byref(out)) == E_INVALID
    assert b"n_streams" in L.hpfw_gpu_last_error()
    assert L.hpfw_gpu_streams_create_rates(None, None, _lib._hp(good), ctypes.byref(out)) == E_INVALID


def _partition(rng, n, T):
    """chunk sizes that sum to n: empty chunks, runs of 1-sample chunks, chunks below T, larger ones"""
    sizes = []
    while sum(sizes) < n:
        r = rng.random()
        if r < 0.1:
            sizes.append(0)
        elif r < 0.25:
            sizes += [1] * int(rng.integers(2, 3 * T))
        elif r < 0.6:
            sizes.append(int(rng.integers(1, T)))
        else:
            sizes.append(int(rng.integers(T, 6000)))
    over = sum(sizes) - n
    while over > 0:
        cut = min(over, sizes[-1])
        sizes[-1] -= cut
        over -= cut
        if sizes[-1] == 0:
            sizes.pop()
    return sizes


@pytest.mark.parametrize("fs", [8000, 22050, 32000, 37800, 48000, 96000])
def test_chunked_restatement_equals_the_whole_feed(fs):
    rng = np.random.default_rng(fs)
    H = ref.half_taps(fs)
    T = 2 * H
    for n in (1, H, T + 1, 20011):
        x = rng.integers(-32768, 32768, size=n).astype(np.int16)
        want = ref.resample(x, fs)
        rs = ChunkedResampler(fs)
        out, at = [], 0
        for size in _partition(rng, n, T):
            out.append(rs.push(x[at:at + size]))
            at += size
            assert rs.n == at and rs.emitted == emitted(at, fs) == sum(o.size for o in out)
            # the oldest input a later output reads is in the history
            assert (rs.emitted * rs.M // rs.L) - H + 1 >= at - (T - 1)
        got = np.concatenate(out)
        assert np.array_equal(got, want[:got.size]) and got.size == emitted(n, fs)
        got = np.concatenate([got, rs.push(np.zeros(H, np.int16))])               # the end of a feed: H zeros
        assert np.array_equal(got, want)


FACADE = r"""
#include <hpfw/gpu/gpu_collector.h>
#include <hpfw/gpu/gpu_storage.h>
#include <hpfw/gpu/sharded_storage.h>
#include <hpfw/gpu/live_streams.h>
template <typename Storage>
int run(const Storage &storage, hpfw_gpu *h)
{
    hpfw::LiveStreamsOptions opt;
    opt.min_score = 10.0;
    opt.resample = true;
    opt.rate = 48000;
    hpfw::LiveStreams<Storage> all(storage, h, 2, opt);
    opt.rates = {48000, 44100, 32000};
    hpfw::LiveStreams<Storage> live(storage, h, 3, opt);
    std::vector<int16_t> a(24000), b;
    auto closed = live.push({{0, a.data(), (int64_t)a.size()}, {1, b.data(), 0}});
    for (auto &c : live.finish()) closed.push_back(c);
    live.reset(2);
    return (int)closed.size();
}
int refused(hpfw_gpu *h)
{
    hpfw::db::GpuStorage<hpfw::GpuCollector> storage;
    hpfw::LiveStreamsOptions opt;
    opt.min_score = 10.0;
    opt.rates = {44100, 48000};
    try {
        hpfw::LiveStreams<hpfw::db::GpuStorage<hpfw::GpuCollector>> live(storage, h, 2, opt);
    } catch (const std::runtime_error &e) {
        return std::string(e.what()).find("44.1 kHz") != std::string::npos ? 3 : 4;
    }
    return 5;
}
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (argv[1][0] == 'r') return refused(nullptr);   // thrown before the handle is used
    hpfw_gpu *h = nullptr;
    if (hpfw_gpu_create(0, &h) != 0) return 1;
    int n;
    if (argv[1][0] == 's') {
        hpfw::db::ShardedGpuStorage<hpfw::GpuCollector> storage(std::vector<int>{0, 0});
        n = run(storage, h);
    } else {
        hpfw::db::GpuStorage<hpfw::GpuCollector> storage;
        n = run(storage, h);
    }
    hpfw_gpu_destroy(h);
    return n;
}
"""


def test_live_streams_facade_compiles_and_links_with_rates(tmp_path):
    src = tmp_path / "live_streams_rates.cpp"
    src.write_text(FACADE)
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(tmp_path / "live_streams_rates"), "-L", lib_dir, "-lhpfw_gpu_multi", "-lhpfw_gpu", "-Wl,-rpath," + lib_dir,
           "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "live_streams_rates")], capture_output=True, text=True)   # no argument: no device touched
    assert r.returncode == 2
