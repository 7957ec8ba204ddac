"""Sample-accurate offsets on the GPU (hpfw_amd/csrc/k_xcorr.hip, hpfw_gpu_xcorr_pcm16*): the exact cross-correlation
against numpy int64 (tests/xcorr_ref.py) on both kernels, the accumulator bound, the peak rule, invalid arguments, the
device entry point, the Mel front end's kept-frame map against the oracle, and AudioCombiner.refine / layout from WAV
files cut off the 441-sample grid, in Python and in the C++ example."""
import os
import subprocess

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, synth

import xcorr_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = synth.SR


@pytest.fixture
def xg(torch_cuda):
    g = hpfw_amd.Gpu(0)
    yield g
    g.close()


@pytest.fixture(params=["mfma", "valu"])
def xcorr_path(request, monkeypatch):
    """the matrix-core kernel (default) and the plain integer kernel (HPFW_XCORR=valu, read at every call)"""
    if request.param == "valu":
        monkeypatch.setenv("HPFW_XCORR", "valu")
    else:
        monkeypatch.delenv("HPFW_XCORR", raising=False)
    return request.param


def _job(a_off, a_len, b_off, b_len, p, q, length, radius):
    return (a_off, a_len, b_off, b_len, p, q, length, radius, 0)


def _jobs(rows):
    return np.array(rows, _lib.XCORR_JOB_DTYPE)


def _peak_row(pk):
    return int(pk["lag"]), int(pk["r"]), int(pk["energy_a"]), int(pk["energy_b"])


# ---- 1. exact against numpy ----------------------------------------------------------------------------------------------
A_OFF, A_LEN, B_OFF, B_LEN, N_PCM = 1000, 90000, 95000, 80000, 180000


def _p_of(case, length, radius):
    """p so that a[p - radius .. p + radius + length) lies inside a, hangs over its start or its end, or misses it"""
    if case == "inside":
        return radius + 7
    if case == "start":
        return -(length // 2 + 1)
    if case == "end":
        return A_LEN - length // 2 - 1
    if case == "before":
        return -(radius + length + 5)
    return A_LEN + radius + 5                     # "after"


# every len and every radius of the issue, every position of a: a dozen ragged jobs for one call
RAGGED = [(1, 0, "inside", 0), (31, 1, "start", 17), (32, 511, "end", B_LEN - 32), (33, 512, "inside", 3),
          (1023, 513, "start", 40001), (4097, 1024, "end", 1), (70001, 1500, "inside", 9999), (4097, 4096, "start", 75000),
          (1, 4096, "after", B_LEN - 1), (33, 1024, "before", 0), (1023, 0, "end", 12), (70001, 1, "start", 0),
          (32, 1500, "end", 7), (1023, 4096, "inside", 555)]


@pytest.fixture(scope="module")
def ragged_case():
    """(pcm, jobs, per job the reference r and peak), computed once"""
    rng = np.random.default_rng(2101)
    pcm = rng.integers(-32768, 32768, size=N_PCM).astype(np.int16)
    # the extremes, alone and in runs that meet each other in some lag
    pcm[rng.integers(0, N_PCM, size=300)] = -32768
    pcm[rng.integers(0, N_PCM, size=300)] = 32767
    pcm[A_OFF + 500:A_OFF + 900] = -32768
    pcm[B_OFF + 10100:B_OFF + 10500] = -32768
    pcm[A_OFF + 30000:A_OFF + 30200] = 32767
    pcm[A_OFF:A_OFF + 40] = -32768
    pcm[A_OFF + A_LEN - 40:A_OFF + A_LEN] = 32767
    rows = [_job(A_OFF, A_LEN, B_OFF, B_LEN, _p_of(c, n, rad), q, n, rad) for n, rad, c, q in RAGGED]
    a, b = pcm[A_OFF:A_OFF + A_LEN], pcm[B_OFF:B_OFF + B_LEN]
    want_r = [xcorr_ref.xcorr(a, b, row[4], row[5], row[6], row[7]) for row in rows]
    want_pk = [xcorr_ref.peak(a, b, row[4], row[5], row[6], row[7], r) for row, r in zip(rows, want_r)]
    return pcm, _jobs(rows), want_r, want_pk


def test_exact_against_numpy(xg, ragged_case, xcorr_path):
    pcm, jobs, want_r, want_pk = ragged_case
    assert {n for n, _, _, _ in RAGGED} == {1, 31, 32, 33, 1023, 4097, 70001}
    assert {r for _, r, _, _ in RAGGED} == {0, 1, 511, 512, 513, 1024, 1500, 4096}
    assert not want_r[8].any() and not want_r[9].any()             # a entirely outside: all zeros
    peaks, r = xg.xcorr(pcm, jobs, want_r=True)
    for i in range(jobs.size):
        assert np.array_equal(r[i], want_r[i]), (xcorr_path, i, RAGGED[i])
        assert _peak_row(peaks[i]) == want_pk[i], (xcorr_path, i, RAGGED[i])
    only_peaks = xg.xcorr(pcm, jobs)                                # no r kept by the caller
    assert np.array_equal(only_peaks, peaks)


def test_two_paths_agree_and_repeat(xg, ragged_case, monkeypatch):
    pcm, jobs, _, _ = ragged_case
    monkeypatch.delenv("HPFW_XCORR", raising=False)
    pk_m, r_m = xg.xcorr(pcm, jobs, want_r=True)
    pk_m2, r_m2 = xg.xcorr(pcm, jobs, want_r=True)
    monkeypatch.setenv("HPFW_XCORR", "valu")
    pk_v, r_v = xg.xcorr(pcm, jobs, want_r=True)
    assert np.array_equal(pk_m, pk_v) and np.array_equal(pk_m, pk_m2)
    assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(r_m, r_v, r_m2))


# ---- 2. the accumulator bound ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length,radius", [(1 << 18, 32), (1 << 22, 1)])
def test_accumulator_bound(xg, xcorr_path, length, radius):
    """every product is 2^30 and every digit product the largest there is: past the 2^17 samples an int32 sum of top-digit
    products lasts"""
    pcm = np.full(length + 2 * radius, -32768, np.int16)
    jobs = _jobs([_job(0, length, 0, length, 0, 0, length, radius),                      # a hangs over at every lag but 0
                  _job(0, length + 2 * radius, 0, length, radius, 0, length, radius)])    # a inside at every lag
    peaks, r = xg.xcorr(pcm, jobs, want_r=True)
    lags = np.arange(-radius, radius + 1, dtype=np.int64)
    assert np.array_equal(r[0], (1 << 30) * (length - np.abs(lags)))
    assert np.array_equal(r[1], np.full(lags.size, (1 << 30) * length, np.int64))
    assert _peak_row(peaks[0]) == (0, (1 << 30) * length, (1 << 30) * length, (1 << 30) * length)
    assert _peak_row(peaks[1]) == (0, (1 << 30) * length, (1 << 30) * length, (1 << 30) * length)
    if length == 1 << 22:
        assert int(r[1][0]) == 1 << 52


# ---- 3. the peak rule ----------------------------------------------------------------------------------------------------------
def test_peak_rule_ties(xg, xcorr_path):
    n = 40000
    pcm = np.zeros(n, np.int16)
    a_off, a_len, b_off, b_len = 0, 20000, 20000, 20000
    rows, want = [], []
    # b = one impulse; impulses of a at chosen lags give |r| ties by construction
    pcm[b_off + 100] = 100
    base = 5000
    for at, v in ((base - 5, 7), (base + 5, 7), (base + 9, -7)):
        pcm[a_off + at] = v
    rows.append(_job(a_off, a_len, b_off, b_len, base - 100, 0, 256, 16))          # b[100] meets a[p + l + 100]
    want.append((-5, 700))                                                          # |l| 5 before 9, then the negative lag
    base2 = 9000
    for at, v in ((base2 + 3, -7), (base2 - 5, 7), (base2 + 5, 7)):
        pcm[a_off + at] = v
    rows.append(_job(a_off, a_len, b_off, b_len, base2 - 100, 0, 256, 16))
    want.append((3, -700))                                                          # the smaller |l| wins, positive as it is
    # periodic operands (period 8): inside a, r repeats every 8 lags over three tiles
    per = np.array([900, -300, 50, 7, -1200, 333, 20, -5], np.int16)
    p_off = 12000
    pcm[a_off + p_off:a_off + p_off + 6400] = np.tile(per, 800)
    pcm[b_off + 4000:b_off + 4000 + 1024] = np.tile(per, 128)
    rows.append(_job(a_off, a_len, b_off, b_len, p_off + 2400, 4000, 1024, 1030))  # in phase at lag 0
    rows.append(_job(a_off, a_len, b_off, b_len, p_off + 2402, 4000, 1024, 1030))  # in phase at lags -2, 6, -10, ...
    jobs = _jobs(rows)
    peaks, r = xg.xcorr(pcm, jobs, want_r=True)
    for i in (0, 1):
        assert (int(peaks[i]["lag"]), int(peaks[i]["r"])) == want[i]
    a, b = pcm[a_off:a_off + a_len], pcm[b_off:b_off + b_len]
    for i in (2, 3):
        ref = xcorr_ref.xcorr(a, b, rows[i][4], rows[i][5], rows[i][6], rows[i][7])
        assert np.array_equal(r[i], ref)
        top = np.abs(ref).max()
        assert (np.abs(ref) == top).sum() >= 200                   # the tie is real, and spans the tiles
        assert _peak_row(peaks[i]) == xcorr_ref.peak(a, b, rows[i][4], rows[i][5], rows[i][6], rows[i][7], ref)
    assert int(peaks[2]["lag"]) == 0 and int(peaks[3]["lag"]) == -2


def test_inverted_pair_scores_minus_one(xg, xcorr_path):
    """b = -a.  The score is r / (sqrt(energy_a) sqrt(energy_b)) in float64, which is -1 exactly when the two square roots
    are exact: the energy here is a perfect square, 1024 (300^2 + 400^2) = 16000^2"""
    a = np.tile(np.array([300, -400], np.int16), 1024)
    rng = np.random.default_rng(5)
    a = a * rng.choice(np.array([-1, 1], np.int16), size=a.size)       # signs at random: no second lag ties
    pcm = np.concatenate([a, -a]).astype(np.int16)
    jobs = _jobs([_job(0, a.size, a.size, a.size, 0, 0, a.size, 64)])
    pk = xg.xcorr(pcm, jobs)[0]
    assert _peak_row(pk) == (0, -16000 ** 2, 16000 ** 2, 16000 ** 2)
    assert xcorr_ref.score(pk["r"], pk["energy_a"], pk["energy_b"]) == -1.0
    assert hpfw_amd.combiner.xcorr_score(pk["r"], pk["energy_a"], pk["energy_b"]) == -1.0
    assert pk["r"] < 0                                                  # inverted


# ---- 4. invalid arguments --------------------------------------------------------------------------------------------------
def test_invalid_arguments(xg):
    pcm = np.arange(-500, 500, dtype=np.int16)
    good = _job(0, 600, 400, 600, 10, 5, 200, 8)
    bad = {"len 0": _job(0, 600, 400, 600, 10, 5, 0, 8),
           "len negative": _job(0, 600, 400, 600, 10, 5, -3, 8),
           "len above 2^22": _job(0, 600, 400, 600, 10, 5, (1 << 22) + 1, 8),
           "radius negative": _job(0, 600, 400, 600, 10, 5, 200, -1),
           "radius above 4096": _job(0, 600, 400, 600, 10, 5, 200, 4097),
           "q negative": _job(0, 600, 400, 600, 10, -1, 200, 8),
           "q + len beyond b": _job(0, 600, 400, 600, 10, 401, 200, 8),
           "a beyond the buffer": _job(500, 501, 400, 600, 10, 5, 200, 8),
           "b beyond the buffer": _job(0, 600, 400, 601, 10, 5, 200, 8),
           "a_off negative": _job(-1, 600, 400, 600, 10, 5, 200, 8),
           "b_len negative": _job(0, 600, 400, -600, 10, 5, 200, 8),
           "a_off beyond the buffer": _job(1001, 0, 400, 600, 10, 5, 200, 8)}
    want = xg.xcorr(pcm, _jobs([good]))
    for name, row in bad.items():
        for rows in ([row], [good, row]):                                           # alone, and behind a valid job
            with pytest.raises(hpfw_amd.HpfwError) as e:
                xg.xcorr(pcm, _jobs(rows))
            assert e.value.status == _lib.E_INVALID, name
        assert np.array_equal(xg.xcorr(pcm, _jobs([good])), want), name             # the handle still works
    # null pointers
    L, h = _lib.lib(), xg._h
    jobs, peaks = _jobs([good]), np.zeros(1, _lib.XCORR_PEAK_DTYPE)
    hp = _lib._hp
    assert L.hpfw_gpu_xcorr_pcm16_host(None, hp(pcm), pcm.size, hp(jobs), 1, None, hp(peaks)) == _lib.E_INVALID
    assert L.hpfw_gpu_xcorr_pcm16_host(h, None, pcm.size, hp(jobs), 1, None, hp(peaks)) == _lib.E_INVALID
    assert L.hpfw_gpu_xcorr_pcm16_host(h, hp(pcm), pcm.size, None, 1, None, hp(peaks)) == _lib.E_INVALID
    assert L.hpfw_gpu_xcorr_pcm16_host(h, hp(pcm), pcm.size, hp(jobs), 1, None, None) == _lib.E_INVALID
    assert L.hpfw_gpu_xcorr_pcm16_host(h, hp(pcm), pcm.size, hp(jobs), -1, None, hp(peaks)) == _lib.E_INVALID
    assert L.hpfw_gpu_xcorr_pcm16(h, None, hp(jobs), 1, None, None, None) == _lib.E_INVALID
    assert L.hpfw_gpu_xcorr_pcm16(None, None, hp(jobs), 1, None, None, None) == _lib.E_INVALID
    assert L.hpfw_gpu_xcorr_pcm16_host(h, hp(pcm), pcm.size, hp(jobs), 0, None, None) == 0      # no job: nothing to do
    assert np.array_equal(xg.xcorr(pcm, _jobs([good])), want)
    a, b = pcm[:600], pcm[400:]
    assert _peak_row(want[0]) == xcorr_ref.peak(a, b, 10, 5, 200, 8)


# ---- 5. the device entry point -----------------------------------------------------------------------------------------------
def test_device_entry_point_on_a_stream(xg, torch_cuda, ragged_case):
    torch = torch_cuda
    pcm, jobs, want_r, want_pk = ragged_case
    jobs = jobs[[3, 5, 8, 4, 0]]
    n_lags = int((2 * jobs["radius"].astype(np.int64) + 1).sum())
    d_pcm = torch.from_numpy(pcm).cuda()
    d_r = torch.full((n_lags,), -1, dtype=torch.int64, device="cuda")
    d_peaks = torch.zeros(jobs.size * _lib.XCORR_PEAK_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_peaks2 = torch.zeros_like(d_peaks)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        xg.xcorr_dev(d_pcm.data_ptr(), jobs, d_r.data_ptr(), d_peaks.data_ptr(), side.cuda_stream)
        xg.xcorr_dev(d_pcm.data_ptr(), jobs, 0, d_peaks2.data_ptr(), side.cuda_stream)
    side.synchronize()
    host_pk, host_r = xg.xcorr(pcm, jobs, want_r=True)
    assert np.array_equal(d_r.cpu().numpy(), np.concatenate(host_r))
    assert np.array_equal(d_peaks.cpu().numpy().view(_lib.XCORR_PEAK_DTYPE), host_pk)
    assert np.array_equal(d_peaks2.cpu().numpy().view(_lib.XCORR_PEAK_DTYPE), host_pk)
    assert [_peak_row(p) for p in host_pk] == [want_pk[i] for i in (3, 5, 8, 4, 0)]


# ---- 6. the kept-frame map -----------------------------------------------------------------------------------------------------
def test_kept_frames_equal_the_oracle_mask(xg, oracle):
    n = int(7.5 * SR) + 123
    rng = np.random.default_rng(6)
    tone = synth.gen_clip(5, 8.0)
    c0 = np.zeros(n, np.int16)
    c0[int(1.5 * SR):int(3.5 * SR)] = tone[:2 * SR]                 # 1.5 s of leading zeros, then 2 s of signal
    z0 = int(3.5 * SR)                                              # 2.5 s of zeros with two isolated clusters
    at473, at474 = z0 + 441 * 30 + 17, z0 + 441 * 60 + 300
    c0[at473:at473 + 3] = [21, 4, 4]                                # 441 + 16 + 16 = 473: ten frames see it, all dropped
    c0[at474:at474 + 4] = [21, 5, 2, 2]                             # 441 + 25 + 4 + 4 = 474: ten frames, all kept
    c0[int(6.0 * SR):] = tone[3 * SR:3 * SR + n - int(6.0 * SR)]
    c1 = rng.integers(-3000, 3000, size=n).astype(np.int16)
    c1[2 * SR:3 * SR] = 0
    got = xg.mel_kept_frames(np.stack([c0, c1]))
    mel = oracle.Mel()
    for clip, g in zip((c0, c1), got):
        keep = mel.power(clip)[1]
        assert g.dtype == np.int32 and np.array_equal(g, np.flatnonzero(keep))
    f473, f474 = at473 // 441, at474 // 441                        # a frame that holds the whole cluster
    for f, kept in ((f473, False), (f474, True)):
        lo, hi = 441 * f - 2205, 441 * f + 2205
        assert int((c0[lo:hi].astype(np.int64) ** 2).sum()) == (474 if kept else 473)
        assert (f in got[0]) == kept
    assert got[0][0] > 1.5 * SR / 441 - 6 and not mel.power(c0)[1][:140].any()
    # the columns of the Mel spectrogram are these frames
    assert [s.shape[1] for s in xg.mel_spectrogram(np.stack([c0, c1]))] == [g.size for g in got]
    assert got[0].size < hpfw_amd.lib().hpfw_gpu_mel_frames(n) - 200
    with pytest.raises(hpfw_amd.HpfwError):
        frames = np.zeros((1, 10), np.int32)
        cnt = np.zeros(1, np.int32)
        _lib.check(_lib.lib().hpfw_gpu_mel_kept_frames_pcm16_host(xg._h, _lib._hp(c0), n, 1, _lib._hp(frames), 10, _lib._hp(cnt)))


# ---- 7. end to end from WAV files cut off the 441-sample grid ----------------------------------------------------------------
CUTS = [0, 7 * SR + 123, 15 * SR + 440, 22 * SR + 1, 30 * SR + 221]     # no multiple of 441 but the first
SNR_DB = [40, 30, 20, 10, 25]
GAIN = [1.0, 1.0, -0.5, 1.0, 1.0]
SILENCE = [0, 0, 0, int(1.5 * SR), 0]                                   # digital silence in front of the recording
REC_LEN = 25 * SR
# layout's thresholds.  min_score: two noisy copies of one signal at SNR s1, s2 correlate at 1 / sqrt((1 + 1/s1) (1 + 1/s2)),
# 0.95 for the worst pair here (10 and 20 dB), and a wrong alignment at a small fraction of that: half way.  min_peak: ten
# seconds of overlap are a thousand columns; a few tens of votes on one offset are already no accident among 65 536 hashes.
MIN_PEAK, MIN_SCORE = 20, 0.5


@pytest.fixture(scope="module")
def event(tmp_path_factory):
    """five 25 s recordings of one 60 s source: (files in name order, the planted start of every file on the source's clock)"""
    d = tmp_path_factory.mktemp("event")
    src = synth.gen_clip(77, 60.0).astype(np.float64)
    files, starts = [], []
    for i, cut in enumerate(CUTS):
        seg = src[cut:cut + REC_LEN]
        assert seg.size == REC_LEN
        rng = np.random.default_rng([synth.SEED, 900 + i])
        noise = np.sqrt(float(np.mean(seg ** 2)) / 10 ** (SNR_DB[i] / 10)) * rng.standard_normal(seg.size)
        x = np.clip(np.round(GAIN[i] * (seg + noise)), -32768, 32767).astype(np.int16)
        x = np.concatenate([np.zeros(SILENCE[i], np.int16), x])
        path = str(d / f"rec{i}.wav")
        synth.write_wav(path, x)
        files.append(path)
        starts.append(cut - SILENCE[i])
    return files, starts


def _refined_event(files):
    comb = hpfw_amd.AudioCombiner(keep_audio=True)
    comb.build(comb.prepare(files))
    hits = [comb.align(comb._hp[i], 8, exclude=i) for i in range(len(files))]
    fine = [comb.refine(i, hits[i]) for i in range(len(files))]
    lay = comb.layout(MIN_PEAK, MIN_SCORE)
    return comb, hits, fine, lay


def test_end_to_end_offsets_to_the_sample(torch_cuda, event):
    files, starts = event
    comb, hits, fine, lay = _refined_event(files)
    n = len(files)
    overlap = lambda i, j: min(CUTS[i], CUTS[j]) + REC_LEN - max(CUTS[i], CUTS[j])
    pairs = [(i, j) for i in range(n) for j in range(n) if i != j and overlap(i, j) >= 10 * SR]
    assert len(pairs) == 12                                            # six pairs, each from both sides
    for i, j in pairs:
        planted = starts[j] - starts[i]                                # query[n + planted] = recording[n]
        by_rec = {h.rec: (h, f) for h, f in zip(hits[i], fine[i])}
        assert j in by_rec, (i, j, hits[i])
        h, f = by_rec[j]
        xq, fq = comb._audio[files[i]]
        xr, fr = comb._audio[files[j]]
        geo = hpfw_amd.combiner.refine_geometry(comb._hp[i].size, comb._hp[j].size, fq, fr, xq.size, xr.size, h.offset, 1 << 18)
        print(f"pair {i} {j}: planted {planted} column offset {h.offset} peak {h.peak} coarse {geo and geo[0]} "
              f"refined {f.offset_samples} inverted {f.inverted} score {f.score:.4f}")
        assert geo is not None and abs(geo[0] - planted) <= 441, (i, j, geo, planted, h)
        assert f.offset_samples == planted, (i, j, f, planted)
        assert f.inverted == ((GAIN[i] < 0) != (GAIN[j] < 0)), (i, j, f)
        assert f.name == files[j] and f.rec == j and f.peak == h.peak and abs(f.score) > MIN_SCORE
    # the silence in front of recording 3 moved its columns: without the kept-frame map its offsets would be 150 columns off
    assert comb._audio[files[3]][1][0] >= 145
    # one event, every recording where it was cut, every other edge consistent with the tree
    assert len(lay) == 1, lay
    assert lay[0].members == tuple(range(n))
    assert lay[0].starts == tuple(s - min(starts) for s in starts)
    assert lay[0].inverted == tuple(g < 0 for g in GAIN)
    assert len(lay[0].residuals) >= 2 and all(res == 0 for _, _, res in lay[0].residuals), lay[0].residuals
    # a second combiner gives identical results
    comb2, hits2, fine2, lay2 = _refined_event(files)
    assert hits2 == hits and fine2 == fine and lay2 == lay
    # a shorter segment and a smaller radius find the same offsets
    for i, j in pairs[:4]:
        h = next(h for h in hits[i] if h.rec == j)
        assert comb.refine(files[i], [h], seg_len=1 << 15, radius=512)[0].offset_samples == starts[j] - starts[i]
    # refine needs the audio
    plain = hpfw_amd.AudioCombiner()
    with pytest.raises(ValueError):
        plain.refine(0, [])
    for c in (comb, comb2, plain):
        c.close()


# ---- 8. the C++ example -------------------------------------------------------------------------------------------------------
def test_cpp_example_prints_the_python_values(torch_cuda, event, tmp_path, capsys):
    files, _ = event
    comb = hpfw_amd.AudioCombiner(keep_audio=True)
    comb.combine(files)
    printed = capsys.readouterr().out
    lines = []
    for i, f in enumerate(files):
        fine = comb.refine(f, comb.align(comb._hp[i], 1, exclude=i))
        lines.append(f"{fine[0].name} {fine[0].offset_samples} {int(fine[0].inverted)} {fine[0].score:.17g}" if fine else " 0 0 0")
    comb.close()
    assert all(l != " 0 0 0" for l in lines)
    exe = tmp_path / "combine"
    cmd = ["g++", "-std=c++20", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "combine.cpp"),
           "-o", str(exe), "-L", os.path.dirname(_lib.LIB_PATH), "-lhpfw_gpu",
           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), "--samples", os.path.dirname(files[0])], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    # the lines of `combine <directory>` first, byte for byte, then one line per file
    assert r.stdout == printed + "\n".join(lines) + "\n"
    r = subprocess.run([str(exe), "--samples"], capture_output=True, text=True)
    assert r.returncode == 2
