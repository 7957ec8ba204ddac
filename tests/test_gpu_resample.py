"""The sample-rate conversion to 44.1 kHz on the MI355X (k_resample.hip): bitwise against the numpy
restatement of tests/resample_ref.py, through the device entry point on a side stream, and through every file path that
takes the switch -- the collector (prepare, calc_hashprint(s), the spectrogram cache), live identification, the
AudioCombiner, the C++ facade and the multi-GPU group."""
import os
import subprocess
from math import gcd

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, multi, synth

import resample_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rg(torch_cuda):
    g = hpfw_amd.Gpu(0)
    yield g
    g.close()


def _noise(seed, n, clips=None):
    rng = np.random.default_rng(seed)
    shape = (n,) if clips is None else (clips, n)
    return rng.integers(-32768, 32768, size=shape).astype(np.int16)


@pytest.mark.parametrize("fs", ref.RATES)
def test_bitwise_against_the_restatement(rg, fs):
    _, _, taps = ref.design(fs)
    T = taps.shape[1]
    for n in (1, T - 1, 4095, 3 * fs + 7, 30 * fs):
        x = _noise([fs, n], n)
        got = rg.resample(x, fs)
        want = ref.resample(x, fs)
        assert got.shape == want.shape == (ref.out_length(n, fs),)
        assert np.array_equal(got, want), (n, int(np.count_nonzero(got != want)))
    batch = _noise([fs, 3], 9001, clips=3)                            # 3 distinct clips in one launch
    assert np.array_equal(rg.resample(batch, fs), ref.resample(batch, fs))
    # full-scale square waves: the accumulator's extremes and the clamp
    t = np.arange(2 * fs + 3)
    sq = np.where((t // max(1, fs // 1000)) % 2 == 0, 32767, -32768).astype(np.int16)
    sq2 = np.where((t // 7) % 2 == 0, -32768, 32767).astype(np.int16)
    for x in (sq, sq2):
        got, want = rg.resample(x, fs), ref.resample(x, fs)
        assert np.array_equal(got, want)
    assert (rg.resample(sq, fs) == 32767).any() and (rg.resample(sq, fs) == -32768).any()


def test_identity_at_44100(rg):
    x = _noise(3, 44100 * 3 + 5, clips=2)
    assert np.array_equal(rg.resample(x, 44100), x)
    assert np.array_equal(rg.resample(x[0, :1], 44100), x[0, :1])


def test_long_clips_need_the_64_bit_tile_base(rg):
    """10 minutes at 48 kHz; 5 minutes at 44 056 Hz, where m M passes 2^32 (M = 11 014, m up to 13.2 M) and the
    table (0.8 MB) stays in device memory"""
    for fs, sec in ((48000, 600), (44056, 300)):
        x = _noise([fs, sec], fs * sec)
        got = rg.resample(x, fs)
        want = ref.resample(x, fs)
        assert got.size == ref.out_length(x.size, fs)
        assert np.array_equal(got, want), (fs, int(np.count_nonzero(got != want)))
    _, M = ref.ratio(44056)
    assert ref.out_length(300 * 44056, 44056) * M > 2 ** 32


def test_device_entry_point_on_a_stream(rg, torch_cuda):
    torch = torch_cuda
    fs, n, clips = 96000, 96000 * 2 + 11, 3
    x = _noise(9, n, clips)
    n_out = hpfw_amd.resample_length(n, fs)
    pad = 5                                                          # offset views: the staging meets unaligned clips
    d_in = torch.from_numpy(np.concatenate([np.zeros(pad, np.int16), x.ravel()])).cuda()
    d_out = torch.full((clips * n_out + 3,), 7, dtype=torch.int16, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rg.resample_dev(d_in.data_ptr() + 2 * pad, n, clips, fs, d_out.data_ptr(), side.cuda_stream)
        ev = torch.cuda.Event()
        ev.record(side)
    torch.cuda.current_stream().wait_event(ev)
    got = d_out.cpu().numpy()
    assert np.array_equal(got[:clips * n_out].reshape(clips, n_out), ref.resample(x, fs))
    assert (got[clips * n_out:] == 7).all()                          # nothing written past the output


def test_bad_arguments(rg):
    with pytest.raises(hpfw_amd.HpfwError):
        rg.resample(np.zeros(100, np.int16), 7999)
    with pytest.raises(hpfw_amd.HpfwError):
        rg.resample(np.zeros(100, np.int16), 192001)
    assert rg.resample(np.zeros(0, np.int16), 48000).size == 0


# ---- file paths -----------------------------------------------------------------------------------------------------
def _write_filters(cache_dir, filt):
    os.makedirs(cache_dir, exist_ok=True)
    with open(os.path.join(cache_dir, "filters.cereal"), "wb") as f:
        f.write(np.array([64, 2420], np.int32).tobytes())
        f.write(np.ascontiguousarray(filt, np.float32).tobytes())


def _at_rate(x44, fs):
    """an independent float conversion of a 44.1 kHz clip to fs (scipy's polyphase FIR), rounded to int16"""
    from scipy.signal import resample_poly
    g = gcd(44100, fs)
    y = resample_poly(x44.astype(np.float64), fs // g, 44100 // g)
    return np.clip(np.round(y), -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory, torch_cuda):
    """44.1, 48 (mono and stereo), 16 and 96 kHz files, lengths repeated so that groups batch"""
    d = tmp_path_factory.mktemp("rates")
    files = []
    spec = [(44100, 1, 6.0), (48000, 1, 6.0), (48000, 2, 6.0), (16000, 1, 6.0), (96000, 1, 5.0), (48000, 1, 6.0),
            (44100, 1, 6.0), (16000, 1, 6.0), (96000, 1, 5.0), (48000, 1, 7.0)]
    for i, (fs, ch, sec) in enumerate(spec):
        x = _at_rate(synth.gen_clip(900 + i, sec), fs) if fs != 44100 else synth.gen_clip(900 + i, sec)
        p = str(d / f"c{i}_{fs}_{ch}.wav")
        if ch == 2:
            rng = np.random.default_rng(i)
            lr = np.stack([x, np.clip(x.astype(np.int32) + rng.integers(-50, 50, x.size), -32768, 32767).astype(np.int16)], 1)
            synth.write_wav(p, lr.ravel(), channels=2, rate=fs)
        else:
            synth.write_wav(p, x, rate=fs)
        files.append(p)
    return d, files


def _collector(cache, filters, resample):
    _write_filters(cache, filters)
    c = hpfw_amd.ParallelCollector(resample=resample)
    c.load(cache)
    return c


def test_collector_switch_off_refuses_48k(corpus, filters, tmp_path):
    _, files = corpus
    c = _collector(str(tmp_path / "cache"), filters, False)
    with pytest.raises(hpfw_amd.HpfwError, match="44100"):
        c.calc_hashprint(files[1])
    hps = c.calc_hashprints(files[:2])
    assert hps[0][0] is not None and hps[1][0] is None               # skipped, as before


def test_calc_hashprint_of_a_48k_file(corpus, filters, gpu, oracle, tmp_path):
    _, files = corpus
    c = _collector(str(tmp_path / "cache"), filters, True)
    pcm, fs = hpfw_amd.wav_read_any(files[1])
    assert fs == 48000
    got = c.calc_hashprint(files[1])
    via_gpu = gpu.extract(gpu.resample(pcm, fs))[0]
    y = ref.resample(pcm, fs)
    want = oracle.Plan(y.size).extract(filters, y)
    assert np.array_equal(got, via_gpu) and np.array_equal(got, want)
    # 44.1 kHz files: the same hashprints with the switch on and off
    off = _collector(str(tmp_path / "cache_off"), filters, False)
    assert np.array_equal(c.calc_hashprint(files[0]), off.calc_hashprint(files[0]))
    a = c.calc_hashprints([files[0], files[6]])
    b = off.calc_hashprints([files[0], files[6]])
    assert all(np.array_equal(x[0], y[0]) for x, y in zip(a, b))


def test_prepare_and_calc_hashprints_on_a_mixed_corpus(corpus, filters, tmp_path, monkeypatch):
    _, files = corpus
    c = _collector(str(tmp_path / "cache"), filters, True)
    single = [c.calc_hashprint(f) for f in files]
    batch = c.calc_hashprints(files)
    assert [os.path.splitext(os.path.basename(f))[0] for f in files] == [n for _, n in batch]
    for i, (hp, _) in enumerate(batch):
        assert hp is not None and np.array_equal(hp, single[i]), i
    monkeypatch.setenv("HPFW_PREPARE_KEEP_FILTERS", "1")
    prep = c.prepare(files)
    assert [n for _, n in prep] == [n for _, n in batch]
    for i, (hp, _) in enumerate(prep):
        assert np.array_equal(hp, single[i]), i
    # the spectrogram cache holds the 44.1 kHz clips' spectrograms: a new collector on the same cache brings the files
    # of the first call back from it, with the same hashprints
    c2 = _collector(str(tmp_path / "cache"), filters, True)
    back = dict((n, hp) for hp, n in c2.prepare([files[0]]))
    for i, f in enumerate(files):
        assert np.array_equal(back[os.path.splitext(os.path.basename(f))[0]], single[i]), i


def test_multi_gpu_group_on_one_device(corpus, filters, tmp_path, monkeypatch):
    _, files = corpus
    monkeypatch.setenv("HPFW_PREPARE_KEEP_FILTERS", "1")
    monkeypatch.setenv("HPFW_NO_SPECTRO_CACHE", "1")
    c = _collector(str(tmp_path / "one"), filters, True)
    want = c.prepare(files)
    _write_filters(str(tmp_path / "grp"), filters)
    g = multi.GpuGroup([0])
    g.set_resample(True)                                             # before the group makes its collectors
    g.load(str(tmp_path / "grp"))
    got = g.prepare(files)
    assert [n for _, n in got] == [n for _, n in want]
    assert all(np.array_equal(a, b) for (a, _), (b, _) in zip(got, want))
    assert np.array_equal(g.calc_hashprint(files[3]), want[3][0])
    g.close()


def test_live_identification_of_queries_at_other_rates(torch_cuda, tmp_path, capsys):
    """16 x 30 s clips indexed at 44.1 kHz; 5 s slices converted to 48, 16 and 96 kHz by an independent float resampler
    find their clip, at the 44.1 kHz slice's offset within one column"""
    lib_dir = tmp_path / "lib"
    lib_dir.mkdir()
    clips = [synth.gen_clip(1200 + i, 30.0) for i in range(16)]
    names = []
    for i, x in enumerate(clips):
        p = str(lib_dir / f"track{i:02d}.wav")
        synth.write_wav(p, x)
        names.append(p)
    li = hpfw_amd.LiveSongIdentification(cache=str(tmp_path / "cache"), resample=True)
    li.index(names)
    qdir = tmp_path / "q"
    qdir.mkdir()
    cases = [(3, 4.0), (7, 11.5), (12, 20.0)]
    for ci, start in cases:
        at = int(start * 44100)
        x = clips[ci][at:at + 5 * 44100]
        q44 = str(qdir / f"track{ci:02d}_q44100.wav")
        synth.write_wav(q44, x)
        (hit44,) = li.top([q44], 1)
        assert hit44[1][0][1] == f"track{ci:02d}"
        off44 = hit44[1][0][2]
        hp44 = li.collector.calc_hashprint(q44)
        for fs in (48000, 16000, 96000):
            q = str(qdir / f"track{ci:02d}_q{fs}.wav")
            synth.write_wav(q, _at_rate(x, fs), rate=fs)
            (hit,) = li.top([q], 1)
            assert hit[1], (ci, fs)
            dist, name, off = hit[1][0]
            assert name == f"track{ci:02d}" and abs(off - off44) <= 1, (ci, fs, hit, off44)
            hp = li.collector.calc_hashprint(q)
            m = min(hp.size, hp44.size)
            agree = 1 - np.unpackbits((hp[:m] ^ hp44[:m]).view(np.uint8)).mean()
            print(f"track{ci:02d} at {fs} Hz: offset {off} (44.1 kHz: {off44}), bit agreement {agree:.3f}")
    li._gpu.close()


def test_audio_combiner_on_recordings_at_mixed_rates(torch_cuda, tmp_path, capsys):
    src = synth.gen_clip(78, 120.0).astype(np.float64)
    starts_s = [0.0, 18.0, 40.0, 55.0]
    rates = [44100, 48000, 32000, 22050]
    n = 52 * 44100
    files, starts = [], []
    for i, (s, fs) in enumerate(zip(starts_s, rates)):
        at = int(round(s * 44100 / 441)) * 441
        seg = src[at:at + n]
        rng = np.random.default_rng([synth.SEED, 600 + i])
        seg = seg + np.sqrt(float(np.mean(seg ** 2)) / 1e4) * rng.standard_normal(seg.size)
        x = np.clip(np.round(seg), -32768, 32767).astype(np.int16)
        p = str(tmp_path / f"rec{i}.wav")
        synth.write_wav(p, _at_rate(x, fs) if fs != 44100 else x, rate=fs)
        files.append(p)
        starts.append(at)
    with pytest.raises(hpfw_amd.HpfwError):
        off = hpfw_amd.AudioCombiner()
        try:
            off.prepare(files[1:2])                                   # switch off: 44.1 kHz only, as before
        finally:
            off.close()
    comb = hpfw_amd.AudioCombiner(resample=True)
    res = comb.combine(files)
    capsys.readouterr()
    overlap = lambda a, b: min(starts[a], starts[b]) + n - max(starts[a], starts[b])
    for qi in range(len(files)):
        w = res[qi]
        assert w.rec is not None and overlap(qi, w.rec) > 0, (qi, w)
        assert abs(w.offset - (starts[w.rec] - starts[qi]) // 441) <= 25, (qi, w)
    comb.close()


FACADE = r"""
#include <cstdio>
#include <hpfw/gpu/gpu_collector.h>
int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    hpfw::GpuCollector c;
    c.set_cache_dir(argv[1]);
    c.load();
    c.set_resample(true);
    for (uint64_t v : c.calc_hashprint(argv[2])) std::printf("%016llx\n", (unsigned long long)v);
    return 0;
}
"""


def test_cpp_facade_with_the_switch(corpus, filters, tmp_path):
    _, files = corpus
    cache = str(tmp_path / "cache") + "/"
    want = _collector(cache, filters, True).calc_hashprint(files[1])
    src = tmp_path / "facade.cpp"
    src.write_text(FACADE)
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    exe = str(tmp_path / "facade")
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", lib_dir,
                        "-lhpfw_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, cache, files[1]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.array([int(v, 16) for v in r.stdout.split()], np.uint64)
    assert np.array_equal(got, want)
