"""Clock drift between recorders and the event rendered, end to end on the MI355X: four recordings of
one 90 s piece on clocks 0, +60, -250 and +400 ppm apart (tests/drift_corpus.py) through AudioCombiner.layout_drift and
render.  The chain of this file run with the references alone -- tests/xcorr_ref.py and tests/warp_ref.py in place of the
kernels, the column offsets taken from the truth -- meets both conditions below on this corpus: drifts within 0.11 ppm of the
truth (the bound is 0.64 ppm), every anchor used, starts within 0.3 samples."""
import os
import subprocess

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, synth
from hpfw_amd.combiner import Component

import drift_corpus as dc
import warp_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# as in the single-offset layout's test: two noisy copies of one signal 20 dB above their noise correlate at 0.99, a wrong
# alignment at a small fraction of that; ten seconds of overlap are a thousand columns and a few tens of votes no accident
MIN_PEAK, MIN_SCORE = 20, 0.5
ANCHOR_LEN, ANCHOR_HOP = 1 << 16, 1 << 18
# the votes of a pair 650 ppm apart spread over the five column offsets its 2 150 samples of slide cross, and the offset that
# wins may belong to either end of the overlap: up to 2.5 columns (1 100 samples) from the lag at the centre, where the first
# anchor looks.  Twice the default radius covers that and the half column of the grid.
RADIUS = 2048
# |score| of every rendered track against the rate-1 member's over their common support, as the restatement renders this
# corpus on the CPU (tracks 1, 2, 3 against track 0); the floor of each is 0.01 below, for the integer-lag residue
REF_SCORE = (0.9820, 0.9893, 0.9900)


@pytest.fixture(scope="module")
def event(torch_cuda, tmp_path_factory):
    """(the combiner with the four recordings indexed, their files, the layout with its details, the rendered tracks)"""
    d = tmp_path_factory.mktemp("drift")
    files = []
    for k, x in enumerate(dc.recordings()):
        files.append(str(d / f"rec{k}.wav"))
        synth.write_wav(files[-1], x)
    comb = hpfw_amd.AudioCombiner(keep_audio=True)
    comb.build(comb.prepare(files))
    comps, pairs = comb.layout_drift(MIN_PEAK, MIN_SCORE, anchor_len=ANCHOR_LEN, anchor_hop=ANCHOR_HOP, radius=RADIUS, details=True)
    tracks = comb.render(comps[0], tracks=True) if len(comps) == 1 else None
    yield comb, files, comps, pairs, tracks
    comb.close()


def test_a_single_offset_per_pair_does_not_fit(event):
    """the slide of these clocks over the recordings is 1 000 to 2 150 samples: layout() with one offset per pair must show
    it, as edges it rejects or as residuals between the edges it keeps -- so the chain of anchors is needed here"""
    comb = event[0]
    lay = comb.layout(MIN_PEAK, MIN_SCORE)
    print(lay)
    whole = len(lay) == 1 and lay[0].members == (0, 1, 2, 3) and len(lay[0].residuals) == 3
    assert not whole or any(abs(res) > 2 for _, _, res in lay[0].residuals)


def test_layout_drift_finds_every_clock(event):
    comb, files, comps, pairs, _ = event
    assert sorted((min(qi, h.rec), max(qi, h.rec)) for qi, h, _ in pairs) == [(i, j) for i in range(4) for j in range(i + 1, 4)]
    spans = []
    for qi, h, at in pairs:
        offset, drift = dc.pair_truth(qi, h.rec)
        span = max(at) - min(at) if at else 0
        print(f"pair {qi} {h.rec}: offset {h.offset:.3f} (truth {offset:.3f}) drift {h.drift_ppm:.4f} ppm (truth {drift * 1e6:.4f}) "
              f"score {h.score:.4f} anchors {h.anchors} used {h.used} rms {h.rms:.3f} span {span}")
        assert h.used >= 3 and span >= 2 * ANCHOR_HOP
        # every lag is right to +-1, so the line's slope to 2 samples over the span of the anchors it used
        assert abs(h.drift_ppm * 1e-6 - drift) <= 2.0 / span, (qi, h)
        # a condition, not a tolerance: the line must rest on the anchors placed, not on the few that happen to agree
        assert h.used >= 0.8 * h.anchors, (qi, h)
        assert h.inverted == ((dc.GAIN[qi] < 0) != (dc.GAIN[h.rec] < 0)) and h.score >= MIN_SCORE and h.name == files[h.rec]
        # the offset is the line at sample 0: a lag's +-1 and the slope's bound over the half span from the anchors' middle
        assert h.anchors >= 10 and abs(h.offset - offset) <= 1.0 + (2.0 / span) * max(abs(min(at)), abs(max(at)))
        spans.append(span)
    assert len(comps) == 1, comps
    c = comps[0]
    starts, rates = dc.component_truth()
    print(c, starts, rates)
    assert c.members == (0, 1, 2, 3) and c.inverted == tuple(g < 0 for g in dc.GAIN) and len(c.residuals) == 3
    assert np.abs(np.array(c.rates) - rates).max() <= 2.0 / min(spans)
    assert np.abs(np.array(c.starts) - starts).max() <= 2.0
    # the edges the tree did not use agree with it: an edge against a path of at most three, each within the bounds above
    for i, j, samples, ppm in c.residuals:
        assert abs(samples) <= 4 * 2.0 and abs(ppm) * 1e-6 <= 4 * 2.0 / min(spans), c.residuals
    # refine_drift alone gives the pair's hit
    qi, h, _ = pairs[0]
    again = comb.refine_drift(files[qi], [a for a in comb.align(comb._hp[qi], 8, exclude=qi) if a.rec == h.rec], MIN_SCORE, ANCHOR_LEN, ANCHOR_HOP,
                              RADIUS)
    assert again == [h]
    plain = hpfw_amd.AudioCombiner()
    with pytest.raises(ValueError):
        plain.refine_drift(0, [], MIN_SCORE)
    with pytest.raises(ValueError):
        plain.render(Component((0,), (0,), (False,), ()))
    plain.close()


def _score(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(a @ b) / np.sqrt(float(a @ a) * float(b @ b))


def test_rendered_tracks_line_up(event, tmp_path):
    comb, files, comps, _, tracks = event
    c = comps[0]
    assert tracks is not None and tracks.shape[0] == 4 and tracks.dtype == np.int16
    ends = [s + r * comb._audio[f][0].size for s, r, f in zip(c.starts, c.rates, files)]
    assert tracks.shape[1] == int(np.ceil(max(ends)))
    for k in (1, 2, 3):
        lo, hi = int(np.ceil(max(c.starts[0], c.starts[k]))) + 64, int(min(ends[0], ends[k])) - 64
        got = _score(tracks[0][lo:hi], tracks[k][lo:hi])
        print(f"track {k} against track 0 over {lo} .. {hi}: {got:.4f} (the restatement on the CPU: {REF_SCORE[k - 1]})")
        assert got >= REF_SCORE[k - 1] - 0.01                         # (positive: the default gains undo the inversion)
    # the rendered tracks as recordings of their own: every pair refines to lag 0, no polarity left
    out = []
    for k in range(4):
        out.append(str(tmp_path / f"track{k}.wav"))
        _lib.wav_write(out[-1], tracks[k])
    again = hpfw_amd.AudioCombiner(keep_audio=True)
    again.build(again.prepare(out))
    seen = set()
    for i in range(4):
        for f in again.refine(i, again.align(again._hp[i], 8, exclude=i)):
            assert f.offset_samples == 0 and not f.inverted and f.score >= MIN_SCORE, (i, f)
            seen.add((i, f.rec))
    assert len(seen) == 12
    again.close()


def test_rendered_mix_is_the_restatement(event):
    """render(component) against warp_ref.mix of the same maps, bit for bit.  The restatement is evaluated through m0 on
    windows -- the first outputs, where each member starts, a seam of the chunks, the last outputs -- which keeps the test at
    a second; the whole length is compared between two chunkings and with the gains given"""
    comb, files, comps, _, _ = event
    c = comps[0]
    pcm = [comb._audio[f][0] for f in files]
    maps = [_lib.time_map_q40(s, r - 1.0) for s, r in zip(c.starts, c.rates)]
    gains = [-(1 << 13) if inv else 1 << 13 for inv in c.inverted]
    mix = comb.render(c)
    n_out = mix.size
    win = 1 << 16
    for m0 in sorted({0, n_out - win, (1 << 20) - win // 2} | {max(0, int(s) - win // 2) for s in c.starts}):
        assert np.array_equal(mix[m0:m0 + win], warp_ref.mix(pcm, maps, gains, m0, win)), m0
    assert np.array_equal(comb.render(c, chunk=1 << 20), mix) and np.array_equal(comb.render(c, gains=gains, chunk=(1 << 21) + 12345), mix)
    assert mix.any() and np.abs(mix[n_out // 2:n_out // 2 + win].astype(np.int32)).max() > 1000
    with pytest.raises(ValueError):
        comb.render(c, gains=[1, 2])


def test_a_plain_component_renders_shifted_copies(event):
    """a Component of layout(): rates 1 and integer starts.  In tracks mode a member with a positive gain is a bit-exact copy"""
    comb, files, _, _, _ = event
    c = Component((0, 2), (1000, 0), (False, True), ())
    x0, x2 = comb._audio[files[0]][0], comb._audio[files[2]][0]
    tracks = comb.render(c, tracks=True, chunk=1 << 21)
    assert tracks.shape == (2, max(1000 + x0.size, x2.size))
    assert np.array_equal(tracks[0][1000:1000 + x0.size], x0) and not tracks[0][:1000].any() and not tracks[0][1000 + x0.size:].any()
    assert np.array_equal(tracks[1][:x2.size], np.clip(-x2.astype(np.int32), -32768, 32767))   # the inverted member, negated
    mix = comb.render(c, gains=[1 << 15, 0])
    assert np.array_equal(mix[1000:1000 + x0.size], x0)               # gain 1.0 alone: the copy again


def test_cpp_example_writes_the_python_bytes(event, tmp_path):
    """examples/combine.cpp --samples --render --tracks: GpuAudioCombiner::layout_drift and render over the same C functions
    give the same placement and the same WAV files, byte for byte"""
    comb, files, comps, _, tracks = event
    c = comps[0]
    _lib.wav_write(str(tmp_path / "py_mix.wav"), comb.render(c))
    exe = tmp_path / "combine"
    cmd = ["g++", "-std=c++20", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "combine.cpp"),
           "-o", str(exe), "-L", os.path.dirname(_lib.LIB_PATH), "-lhpfw_gpu",
           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), "--samples", "--render", str(tmp_path / "cpp_mix.wav"), "--tracks", str(tmp_path / "cpp_tracks"),
                        "--min-peak", str(MIN_PEAK), "--min-score", str(MIN_SCORE), "--anchor-hop", str(ANCHOR_HOP), "--radius", str(RADIUS),
                        os.path.dirname(files[0])], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = " ".join(f"{m} : {s:.17g} {q:.17g}" for m, s, q in zip(c.members, c.starts, c.rates))
    assert r.stdout.splitlines()[-1] == line, r.stdout[-2000:]
    assert (tmp_path / "cpp_mix.wav").read_bytes() == (tmp_path / "py_mix.wav").read_bytes()
    for k in range(4):
        _lib.wav_write(str(tmp_path / "py_track.wav"), tracks[k])
        assert (tmp_path / "cpp_tracks" / f"track{k}.wav").read_bytes() == (tmp_path / "py_track.wav").read_bytes(), k
