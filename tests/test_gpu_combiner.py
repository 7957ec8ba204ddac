"""AudioCombiner on the GPU (hpfw_amd/csrc/k_combiner.hip, hpfw_gpu_combiner_*): the inverted index against a numpy
stable argsort, find against the loop-for-loop restatement of combiner.h:90-132 (tests/combiner_ref.py), align against
numpy per-diagonal counts, chunked passes under a small workspace, a realistic corpus of Mel hashprints, and the whole
path from WAV files through the Python class and the C++ example."""
import os
import subprocess

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, synth

from combiner_ref import NONE, RefIndex, events_per_query, expected_topk, mel_corpus, numpy_peaks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def cg(torch_cuda):
    g = hpfw_amd.Gpu(0)
    yield g
    g.close()


def _rows(res):
    return [(int(r["rec"]), int(r["cnt"]), int(r["confidence"]), int(r["offset"])) for r in res]


def _index_want(recs):
    allv = np.concatenate([np.asarray(r, np.uint16) for r in recs]) if recs else np.zeros(0, np.uint16)
    rec_of = np.repeat(np.arange(len(recs)), [len(r) for r in recs])
    off_of = np.concatenate([np.arange(len(r)) for r in recs]) if recs else np.zeros(0, np.int64)
    order = np.argsort(allv, kind="stable")
    vs = np.searchsorted(allv[order], np.arange(65537), "left")
    return vs, rec_of[order], off_of[order]


def _check_align(g, queries, recs, k, exclude):
    got = g.combiner_align(queries, k, exclude)
    for qi, q in enumerate(queries):
        pk = numpy_peaks(q, recs, exclude[qi])
        want = expected_topk(pk, k)
        assert [(int(h["rec"]), int(h["peak"]), int(h["offset"])) for h in got[qi]] == want, qi
    return got


def _random_recordings(rng, n, lo, hi, alphabet=65536):
    return [rng.integers(0, alphabet, size=int(rng.integers(lo, hi + 1))).astype(np.uint16) for _ in range(n)]


def test_index_equals_stable_argsort(cg):
    rng = np.random.default_rng(11)
    recs = _random_recordings(rng, 9, 0, 3000, alphabet=4096)
    recs[2] = np.zeros(0, np.uint16)
    recs[5] = np.array([4095], np.uint16)
    recs[7] = np.full(500, 0xFFFF, np.uint16)
    cg.combiner_add(recs)
    assert cg.combiner_size() == 9
    vs, rec, off = cg.combiner_get()
    wvs, wrec, woff = _index_want(recs)
    assert np.array_equal(vs, wvs) and np.array_equal(rec, wrec) and np.array_equal(off, woff)
    cg.combiner_clear()                                  # two appends = one add
    cg.combiner_add(recs[:4])
    cg.combiner_add(recs[4:])
    vs2, rec2, off2 = cg.combiner_get()
    assert np.array_equal(vs2, wvs) and np.array_equal(rec2, wrec) and np.array_equal(off2, woff)
    cg.combiner_clear()
    vs3, rec3, _ = cg.combiner_get()
    assert rec3.size == 0 and not vs3.any()


def test_find_against_restatement(cg):
    rng = np.random.default_rng(12)
    recs = _random_recordings(rng, 12, 1, 2500, alphabet=2048)      # a small alphabet: many chance events
    recs[3] = recs[1].copy()                                         # a recording repeated: ties, leadership switches
    recs[6] = np.zeros(0, np.uint16)
    queries, exclude = [], []
    for i, (src, at, n) in enumerate([(0, 100, 800), (1, 0, 1200), (4, 700, 300), (8, 10, 1500), (9, 0, 1)]):
        q = recs[src][at:at + n].copy()
        flips = rng.random(q.size) < 0.2                             # bit flips
        q[flips] ^= (np.uint16(1) << rng.integers(0, 11, size=int(flips.sum())).astype(np.uint16))
        queries.append(q)
        exclude.append(-1)
    queries.append(recs[5].copy())
    exclude.append(5)                                                # self-exclusion
    queries.append(recs[1].copy())
    exclude.append(1)                                                # its twin (3) must win
    queries.append(np.full(40, 3000, np.uint16))                     # a value nowhere in the index: no event
    exclude.append(-1)
    queries.append(np.zeros(0, np.uint16))                           # an empty query
    exclude.append(-1)
    cg.combiner_add(recs)
    got = _rows(cg.combiner_find(queries, exclude))
    ref = RefIndex(recs)
    want = [ref.find(q, e) for q, e in zip(queries, exclude)]
    assert got == want
    assert got[-2] == (NONE, 0, 0, 0) and got[-1] == (NONE, 0, 0, 0)
    assert got[6][0] == 3
    # an empty index
    cg.combiner_clear()
    assert _rows(cg.combiner_find(queries[:3])) == [(NONE, 0, 0, 0)] * 3
    assert (cg.combiner_align(queries[:3], 4)["rec"] == NONE).all()


def test_align_against_numpy(cg):
    rng = np.random.default_rng(13)
    recs = _random_recordings(rng, 10, 50, 2000, alphabet=1024)
    x = rng.integers(0, 65536, size=60).astype(np.uint16)
    recs[4] = np.concatenate([x, x])                 # a query equal to x matches at d = 0 and d = -60: the smaller wins
    queries = [x, recs[2][100:900], recs[7], np.zeros(0, np.uint16), rng.integers(0, 1024, size=700).astype(np.uint16)]
    exclude = [-1, -1, 7, -1, 2]
    cg.combiner_add(recs)
    got = _check_align(cg, queries, recs, 6, exclude)
    assert got[0][0]["rec"] == 4 and got[0][0]["peak"] == 60 and got[0][0]["offset"] == -60
    assert (got[3]["rec"] == NONE).all()
    got64 = _check_align(cg, queries, recs, 64, exclude)             # k above the recordings: padded
    assert (got64[:, 10:]["rec"] == NONE).all()
    assert 7 not in got64[2]["rec"]


def test_skewed_hashes_in_chunks(cg, monkeypatch):
    """a large share of 0xFFFF (constant stretches) and a query whose events take many chunks of a small workspace"""
    rng = np.random.default_rng(14)
    recs = _random_recordings(rng, 4, 2500, 3500, alphabet=8192)
    for r in recs:
        r[rng.random(r.size) < 0.3] = 0xFFFF
    q = rng.integers(0, 8192, size=5000).astype(np.uint16)
    q[rng.random(q.size) < 0.3] = 0xFFFF
    q[1000:2000] = recs[2][500:1500]
    queries = [q, recs[1][:3000], q[::-1].copy()]
    cg.combiner_add(recs)
    ref = RefIndex(recs)
    want = [ref.find(x) for x in queries]
    monkeypatch.delenv("HPFW_COMBINER_WORKSPACE_MB", raising=False)
    base_find, base_align = _rows(cg.combiner_find(queries)), cg.combiner_align(queries, 4)
    monkeypatch.setenv("HPFW_COMBINER_WORKSPACE_MB", "1")            # ~2.3 M events per query: dozens of chunks
    small_find, small_align = _rows(cg.combiner_find(queries)), cg.combiner_align(queries, 4)
    assert base_find == want and small_find == want
    assert np.array_equal(base_align, small_align)
    _check_align(cg, queries, recs, 4, [-1, -1, -1])
    with pytest.raises(hpfw_amd.HpfwError, match="exceeds the workspace"):
        cg.combiner_find([np.zeros(100000, np.uint16)])              # 4 x 99 999 + N bins > 1 MiB


def test_realistic_corpus_all_vs_all(cg, monkeypatch):
    monkeypatch.delenv("HPFW_COMBINER_WORKSPACE_MB", raising=False)
    recs = mel_corpus(cg)
    assert len(recs) == 64 and all(r.size > 5000 for r in recs)
    cg.combiner_add(recs)
    ex = list(range(64))
    res = _rows(cg.combiner_find(recs, ex))
    ref = RefIndex(recs)
    events = events_per_query(recs, recs, ex)
    checked = [qi for qi in (0, 1, 33, 62) if events[qi] <= 4_000_000][:3]   # the restatement on a subset
    assert len(checked) >= 2, events
    for qi in checked:
        assert res[qi] == ref.find(recs[qi], qi), qi
    aligned = _check_align(cg, recs, recs, 8, ex)
    again = _rows(cg.combiner_find(recs, ex))                       # deterministic
    assert again == res
    # several passes of a few queries each: a 32 MiB workspace takes queries while their bins stay within 16 MiB
    bins = [len(recs) * (r.size - 1) + sum(x.size for x in recs) for r in recs]
    assert max(bins) * 4 < 32 << 20 and sum(bins) * 4 > 8 * (16 << 20)   # every query fits, at least 8 passes
    monkeypatch.setenv("HPFW_COMBINER_WORKSPACE_MB", "32")
    assert _rows(cg.combiner_find(recs, ex)) == res
    assert np.array_equal(cg.combiner_align(recs, 8, ex), aligned)


def test_passes_bounded_by_the_number_of_recordings(cg):
    """20 000 recordings: a pass takes at most 2^24 / 20 000 = 838 queries (its peak table), so 900 queries take two"""
    rng = np.random.default_rng(15)
    recs = _random_recordings(rng, 20000, 0, 3, alphabet=4096)
    queries, exclude = [], []
    for i in range(900):
        j = int(rng.integers(0, len(recs)))
        q = np.concatenate([recs[j], rng.integers(0, 4096, size=int(rng.integers(0, 6))).astype(np.uint16)])
        queries.append(q)
        exclude.append(j if i % 3 == 0 else -1)
    cg.combiner_add(recs)
    got = _rows(cg.combiner_find(queries, exclude))
    ref = RefIndex(recs)
    assert got == [ref.find(q, e) for q, e in zip(queries, exclude)]
    aligned = cg.combiner_align(queries, 5, exclude)
    parts = np.concatenate([cg.combiner_align(queries[a:a + 100], 5, exclude[a:a + 100]) for a in range(0, 900, 100)])
    assert np.array_equal(aligned, parts)
    for qi in (0, 1, 899):
        want = expected_topk(numpy_peaks(queries[qi], recs, exclude[qi]), 5)
        assert [(int(h["rec"]), int(h["peak"]), int(h["offset"])) for h in aligned[qi]] == want, qi


def test_device_entry_points_on_a_stream(cg, torch_cuda):
    """_add_device, _find_device, _align_device on a side stream, with offsets that do not start at 0"""
    torch = torch_cuda
    rng = np.random.default_rng(16)
    recs = _random_recordings(rng, 7, 100, 1500, alphabet=1024)
    recs[2] = np.zeros(0, np.uint16)
    db = np.concatenate([rng.integers(0, 65536, size=37).astype(np.uint16)] + recs)
    db_off = 37 + np.concatenate([[0], np.cumsum([r.size for r in recs])]).astype(np.int64)
    queries = [recs[1][50:400], recs[4][:200], np.zeros(0, np.uint16), recs[0], recs[6][::-1].copy()]
    exclude = [-1, 4, -1, 0, -1]
    qs = np.concatenate([rng.integers(0, 65536, size=11).astype(np.uint16)] + queries)
    q_off = 11 + np.concatenate([[0], np.cumsum([q.size for q in queries])]).astype(np.int64)
    k = 4
    d_db = torch.from_numpy(db.view(np.int16)).cuda()
    d_q = torch.from_numpy(qs.view(np.int16)).cuda()
    d_find = torch.zeros(len(queries) * _lib.COMBINE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_align = torch.zeros(len(queries) * k * _lib.ALIGN_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cg.combiner_add_dev(d_db.data_ptr(), db_off, side.cuda_stream)
        cg.combiner_find_dev(d_q.data_ptr(), q_off, exclude, d_find.data_ptr(), side.cuda_stream)
        cg.combiner_align_dev(d_q.data_ptr(), q_off, exclude, k, d_align.data_ptr(), side.cuda_stream)
    side.synchronize()
    vs, rec, off = cg.combiner_get()
    wvs, wrec, woff = _index_want(recs)
    assert np.array_equal(vs, wvs) and np.array_equal(rec, wrec) and np.array_equal(off, woff)
    ref = RefIndex(recs)
    assert _rows(d_find.cpu().numpy().view(_lib.COMBINE_DTYPE)) == [ref.find(q, e) for q, e in zip(queries, exclude)]
    got = d_align.cpu().numpy().view(_lib.ALIGN_DTYPE).reshape(len(queries), k)
    for qi, q in enumerate(queries):
        want = expected_topk(numpy_peaks(q, recs, exclude[qi]), k)
        assert [(int(h["rec"]), int(h["peak"]), int(h["offset"])) for h in got[qi]] == want, qi
    assert np.array_equal(got, cg.combiner_align(queries, k, exclude))  # the host entry point agrees


def _write_recordings(tmp_path):
    """6 recordings cut from one 150 s source at multiples of 441 samples, light noise each, one of them stereo"""
    src = synth.gen_clip(77, 150.0).astype(np.float64)
    starts_s = [0.0, 18.0, 40.0, 62.0, 80.0, 95.0]
    n = 52 * synth.SR
    files, starts = [], []
    for i, s in enumerate(starts_s):
        at = int(round(s * synth.SR / 441)) * 441
        seg = src[at:at + n]
        rng = np.random.default_rng([synth.SEED, 500 + i])
        p = float(np.mean(seg ** 2))
        seg = seg + np.sqrt(p / 10 ** (40 / 10)) * rng.standard_normal(seg.size)
        x = np.clip(np.round(seg), -32768, 32767).astype(np.int16)
        path = str(tmp_path / f"rec{i}.wav")
        if i == 3:
            lr = np.stack([x, x], 1)
            synth.write_wav(path, lr.ravel(), channels=2)
        else:
            synth.write_wav(path, x)
        files.append(path)
        starts.append(at)
    return files, starts


def test_end_to_end_from_audio(torch_cuda, tmp_path, capsys):
    files, starts = _write_recordings(tmp_path)
    comb = hpfw_amd.AudioCombiner()
    res = comb.combine(files)
    printed = capsys.readouterr().out
    hps = comb._hp
    n = [h.size for h in hps]
    # the printed lines: the restatement on the same hashprints
    ref = RefIndex(hps)
    lines = []
    for i, f in enumerate(files):
        r = ref.find(hps[i], i)
        lines += [f"FINDING {f}", f"{files[r[0]] if r[0] != NONE else ''} {r[1]} {r[2]} {r[3]}", ""]
    assert printed == "\n".join(lines) + "\n"
    overlap = lambda a, b: min(starts[a] + 52 * synth.SR, starts[b] + 52 * synth.SR) - max(starts[a], starts[b])
    for qi in range(len(files)):
        hits = comb.align(hps[qi], 8, exclude=qi)
        by_rec = {h.rec: h for h in hits}
        partners = [j for j in range(len(files)) if j != qi and overlap(qi, j) >= 20 * synth.SR]
        assert partners
        for j in partners:
            assert j in by_rec and by_rec[j].offset == (starts[j] - starts[qi]) // 441, (qi, j, by_rec.get(j))
        # find's winner: an overlapping recording near its true offset.  Not necessarily on it: the reference compares a
        # bin's count with the result's confidence (combiner.h:117), not with its cnt, so the result follows the last
        # event whose bin exceeds a small confidence, and the diagonals next to the true one collect many events too
        # (a 0.25 s note of the synthetic source is 25 frames of similar spectra)
        w = res[qi]
        assert w.rec is not None and overlap(qi, w.rec) > 0 and abs(w.offset - (starts[w.rec] - starts[qi]) // 441) <= 25, (qi, w)
    # the C++ example on the same directory prints the same lines
    exe = tmp_path / "combine"
    cmd = ["g++", "-std=c++20", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "combine.cpp"),
           "-o", str(exe), "-L", os.path.dirname(_lib.LIB_PATH), "-lhpfw_gpu",
           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout == printed
    # determinism: a second combiner gives the same results
    comb2 = hpfw_amd.AudioCombiner()
    assert comb2.combine(files) == res
    capsys.readouterr()
    with pytest.raises(ValueError):
        comb2.build([("a", hps[0]), ("a", hps[1])])
    comb.close()
    comb2.close()
    assert min(n) > 4000


def test_empty_wav_among_the_recordings(torch_cuda, tmp_path, capsys):
    """a file of 0 samples: no covariance, no hashprints, no match -- in Python and in the C++ example"""
    src = synth.gen_clip(78, 60.0)
    files = [str(tmp_path / f"{name}.wav") for name in ("a", "b", "c")]
    synth.write_wav(files[0], src[:25 * synth.SR])
    synth.write_wav(files[1], np.zeros(0, np.int16))
    synth.write_wav(files[2], src[1000 * 441:1000 * 441 + 25 * synth.SR])
    comb = hpfw_amd.AudioCombiner()
    res = comb.combine(files)
    printed = capsys.readouterr().out
    comb.close()
    assert res[1].rec is None and (res[1].cnt, res[1].confidence, res[1].offset) == (0, 0, 0)
    assert printed.splitlines()[3:5] == [f"FINDING {files[1]}", " 0 0 0"]
    assert res[0].rec == 2 and res[2].rec == 0
    exe = tmp_path / "combine"
    cmd = ["g++", "-std=c++20", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "combine.cpp"),
           "-o", str(exe), "-L", os.path.dirname(_lib.LIB_PATH), "-lhpfw_gpu",
           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout == printed
