"""Live feeds on the GPU: the windows cut out of rings that wrap, sample for sample and hashprint for
hashprint against the windows of the concatenated feed copied out on the host; a push that does not fit; a feed that
reconnects; and LiveStreams against LiveSongIdentification.timeline() on the concerts of tests/test_gpu_timeline.py."""
import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, synth

import timeline_ref as ref

pytestmark = pytest.mark.gpu
SHIFTS, TEMPOS = [-2, 0, 2], [0.96, 1.0, 1.04]
SECONDS = (7.0, 5.3, 1.5)                     # the last feed never completes a window of 2 s


def _feeds():
    return [synth.gen_clip(700 + i, 30.0)[:int(round(s * synth.SR))] for i, s in enumerate(SECONDS)]


def _direct(gpu, w, tempos, shifts):
    if tempos is not None:
        return gpu.extract_tempo(w, tempos, shifts)
    return gpu.extract_transposed(w, shifts) if shifts is not None else gpu.extract(w)


def _expected(gpu, feeds, win, hop, tempos=None, shifts=None):
    """per feed (windows int16 [n_w][win], their hashprints) from the feed as one recording"""
    out = []
    for x in feeds:
        w = ref.windows_of(x, win, hop)
        out.append((w, _direct(gpu, w, tempos, shifts) if w.shape[0] else None))
    return out


def _drive(gpu, torch, feeds, win, hop, form, seed, tempos=None, shifts=None, capacity=None, max_chunk=5000):
    """pushes the feeds in seeded random chunks of 0 .. max_chunk samples, differing between the feeds of one push, and
    extracts after every push: on odd pushes one window at a time until none is ready, on even pushes all at once.
    Returns per feed ([window numbers], [clips], [hashprints]) and the number of times each ring wrapped."""
    rng = np.random.default_rng(seed)
    capacity = win + 5000 if capacity is None else capacity
    s = gpu.streams(len(feeds), win, hop, capacity, tempos, shifts)
    got = [([], [], []) for _ in feeds]
    try:
        assert (s.capacity, s.n_streams, s.win, s.hop) == (capacity, len(feeds), win, hop)
        at = [0] * len(feeds)
        push = 0
        while any(a < x.size for a, x in zip(at, feeds)):
            sizes = [int(min(rng.integers(0, max_chunk + 1), x.size - a)) for a, x in zip(at, feeds)]
            if push % 5 == 0:
                k = push // 5 % len(feeds)
                sizes[k] = min(push // 5 % 2, feeds[k].size - at[k])            # (sizes 0 and 1 occur for certain)
            chunks = [x[a:a + n] for a, x, n in zip(at, feeds, sizes)]
            assert (s.room() >= max_chunk).all()
            if form == "host":
                ready = s.push([c if c.size else None for c in chunks])
            else:
                flat = torch.from_numpy(np.concatenate(chunks + [np.zeros(1, np.int16)])).cuda()
                ready = s.push_dev(flat.data_ptr(), sizes)
                torch.cuda.synchronize()
            at = [a + n for a, n in zip(at, sizes)]
            n_i, e_i = s.info()
            assert list(n_i) == at
            assert ready == sum(_lib.window_count(a, win, hop) - int(e) for a, e in zip(at, e_i)) == s.ready()
            while ready:
                cap = 1 if push % 2 else ready
                if form == "host":
                    which, hp, clips = s.extract(cap, clips=True)
                else:
                    shape = s._hp_shape(cap)
                    d_hp = torch.zeros(shape, dtype=torch.int64, device="cuda")
                    d_clips = torch.zeros((cap, win), dtype=torch.int16, device="cuda")
                    which = s.extract_dev(cap, d_hp.data_ptr(), d_clips.data_ptr())
                    torch.cuda.synchronize()
                    hp, clips = d_hp.cpu().numpy().view(np.uint64), d_clips.cpu().numpy()
                assert which.size == cap and hp.shape[0] == cap
                order = [(int(w["feed"]), int(w["window"])) for w in which]
                assert order == sorted(order)
                for j, (f, w) in enumerate(order):
                    got[f][0].append(w)
                    got[f][1].append(clips[j].copy())
                    got[f][2].append(hp[j].copy())
                ready -= cap
                assert s.ready() == ready                                        # the windows beyond cap stay ready
            push += 1
        assert s.extract()[0].size == 0
        wraps = [int(n) // capacity for n in s.info()[0]]
    finally:
        s.close()
    return got, wraps


def _same(got, want, what):
    for f, ((wins, clips, hps), (w_want, hp_want)) in enumerate(zip(got, want)):
        assert wins == list(range(w_want.shape[0])), (what, f, wins)
        if wins:
            assert np.array_equal(np.stack(clips), w_want), (what, f)
            assert np.array_equal(np.stack(hps), hp_want), (what, f)


@pytest.mark.parametrize("win", [88200, 88201])
def test_stream_windows_are_exact(gpu, torch_cuda, win):
    """three feeds of 7.0, 5.3 and 1.5 s in rings of win + 5000 samples, a 7-smooth and a chirp-z window length (an even and an
    odd stride of the gathered clips), an even, an odd and a full-window hop: clips and hashprints of every window equal those
    of the feed taken as one recording, from host and from device pointers, with shifts, tempos and both, in projection mode
    0, and with one extraction in several passes"""
    feeds = _feeds()
    assert _lib.supported_length(win) == win
    for hop in (44100, 9973, win):
        want = _expected(gpu, feeds, win, hop)
        assert want[0][0].shape[0] >= 3 and want[1][0].shape[0] >= 2 and want[2][0].shape[0] == 0
        for form in ("host", "device"):
            got, wraps = _drive(gpu, torch_cuda, feeds, win, hop, form, seed=hop % 1000 + (form == "host"))
            assert wraps[0] >= 3 and wraps[1] >= 2, wraps
            _same(got, want, (win, hop, form))
    hop = 9973
    for tempos, shifts in ((None, SHIFTS), (TEMPOS, None), (TEMPOS, SHIFTS)):
        got, _ = _drive(gpu, torch_cuda, feeds, win, hop, "host" if shifts is None else "device", seed=5, tempos=tempos, shifts=shifts)
        _same(got, _expected(gpu, feeds, win, hop, tempos, shifts), (win, tempos, shifts))
    # one extraction in several passes: rings that hold a whole feed, each feed in one chunk, the windows extracted 3 at a time
    want = _expected(gpu, feeds, win, hop)
    gpu.set_batch(3)
    try:
        s = gpu.streams(3, win, hop, 7 * synth.SR + 8)
        try:
            assert s.push(feeds) == want[0][0].shape[0] + want[1][0].shape[0] >= 30
            which, hp, clips = s.extract(clips=True)
            assert [(int(w["feed"]), int(w["window"])) for w in which] == [(f, w) for f in range(2) for w in range(want[f][0].shape[0])]
            assert np.array_equal(clips, np.concatenate([want[0][0], want[1][0]]))
            assert np.array_equal(hp, np.concatenate([want[0][1], want[1][1]]))
        finally:
            s.close()
    finally:
        gpu.set_batch(0)
    gpu.set_projection(0)
    try:
        got, _ = _drive(gpu, torch_cuda, feeds, win, hop, "host", seed=6)
        _same(got, _expected(gpu, feeds, win, hop), (win, "projection 0"))
        for kw in (dict(shifts=SHIFTS), dict(tempos=TEMPOS)):
            with pytest.raises(hpfw_amd.HpfwError, match="projection mode 1"):
                gpu.streams(3, win, hop, **kw)
    finally:
        gpu.set_projection(1)


def test_push_that_does_not_fit_changes_nothing(gpu):
    """an overfull chunk on one feed refuses the whole push: no feed receives anything, info and room are as before, and the
    windows that follow are those of the accepted pushes alone"""
    win, hop = 88200, 44100
    a, b = _feeds()[:2]
    s = gpu.streams(2, win, hop)                                                # capacity 0: two windows
    try:
        assert s.capacity == 2 * win
        assert s.push([a[:100000], b[:50000]]) == 1
        before = s.info()
        assert list(s.room()) == [2 * win - 100000, 2 * win - 50000]
        with pytest.raises(hpfw_amd.HpfwError, match="feed 1") as e:
            s.push([a[100000:100010], b[50000:50000 + 2 * win - 50000 + 1]])   # feed 0 would fit, feed 1 is one sample too long
        assert e.value.status == _lib.E_INVALID
        after = s.info()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert list(s.room()) == [2 * win - 100000, 2 * win - 50000] and s.ready() == 1
        with pytest.raises(hpfw_amd.HpfwError):
            s.push([a[:2 * win], None])                                          # the first feed named is the first that fails
        assert "feed 0" in str(hpfw_amd.lib().hpfw_gpu_last_error())
        assert s.push([a[100000:100010], b[50000:2 * win]]) == 1 + 3            # exactly full is accepted
        assert list(s.room()) == [2 * win - 100010, 0]
        which, hp, clips = s.extract(clips=True)
        assert [(int(w["feed"]), int(w["window"])) for w in which] == [(0, 0), (1, 0), (1, 1), (1, 2)]
        want = np.concatenate([ref.windows_of(a[:100010], win, hop), ref.windows_of(b[:2 * win], win, hop)])
        assert np.array_equal(clips, want) and np.array_equal(hp, gpu.extract(want))
        assert list(s.room()) == [2 * win - 100010 + hop, 3 * hop]               # handed-out windows free their hop
        assert s.extract()[0].size == 0
    finally:
        s.close()


def test_reset_restarts_one_feed(gpu):
    """a feed that reconnects starts again at sample 0 and window 0, wherever its ring stood; the other feed goes on"""
    win, hop = 88200, 9973
    a, b, c = (synth.gen_clip(710 + i, 30.0)[:n] for i, n in enumerate((4 * synth.SR, 130001, 3 * synth.SR)))
    s = gpu.streams(2, win, hop, win + 50001)
    got = ([], [])
    try:
        def take():
            which, hp, clips = s.extract(clips=True)
            for w, h, x in zip(which, hp, clips):
                got[int(w["feed"])].append((int(w["window"]), h.copy(), x.copy()))

        s.push([a[:100001], b[:100001]])
        take()
        s.push([a[100001:130002], b[100001:]])                                   # feed 1: windows 0 .. 4 complete, the ring part full
        s.reset(1)                                                               # ... and dropped with what was ready
        assert list(s.info()[0]) == [130002, 0] and list(s.info()[1]) == [2, 0] and s.room()[1] == s.capacity
        with pytest.raises(hpfw_amd.HpfwError):
            s.reset(2)
        take()                                                                   # feed 0's three windows alone
        assert [len(g) for g in got] == [5, 2]
        at_a, at_c = 130002, 0
        while at_a < a.size or at_c < c.size:
            s.push([a[at_a:at_a + 40000], c[at_c:at_c + 50000]])
            at_a, at_c = min(at_a + 40000, a.size), min(at_c + 50000, c.size)
            take()
    finally:
        s.close()
    first = ref.windows_of(b[:100001], win, hop)
    want_1 = np.concatenate([first, ref.windows_of(c, win, hop)])
    assert [w for w, _, _ in got[1]] == list(range(first.shape[0])) + list(range(want_1.shape[0] - first.shape[0]))
    assert np.array_equal(np.stack([x for _, _, x in got[1]]), want_1)
    assert np.array_equal(np.stack([h for _, h, _ in got[1]]), gpu.extract(want_1))
    want_0 = ref.windows_of(a, win, hop)
    assert [w for w, _, _ in got[0]] == list(range(want_0.shape[0]))
    assert np.array_equal(np.stack([x for _, _, x in got[0]]), want_0)
    assert np.array_equal(np.stack([h for _, h, _ in got[0]]), gpu.extract(want_0))


# ---- end to end ---------------------------------------------------------------------------------------------------------------
N_SONGS = 20


def _lsi(filters, devices=None):
    """an identifier whose collector holds the filter fixture and whose index holds the 20 songs hashed under it, as
    tests/test_gpu_timeline.py builds it"""
    lsi = hpfw_amd.LiveSongIdentification(devices=devices)
    ext = lsi.collector.gpu()
    ext.set_filters(filters)
    hp = ext.extract(np.stack([synth.gen_clip(i, 30.0) for i in range(N_SONGS)]))
    lsi.build([(hp[i], f"song{i:02d}") for i in range(N_SONGS)])
    return lsi


@pytest.mark.parametrize("case", ["concert_a", "concert_b_variants", "concert_a_sharded"])
def test_streams_equal_the_timeline(tmp_path, filters, torch_cuda, case):
    """feed 0: the concert in random chunks of up to 3 s; feed 1: the same concert in chunks of 0.5 s, started 7 pushes later;
    feed 2: white noise.  For feeds 0 and 1 the segments and per-window rows of all pushes plus finish() equal
    timeline(windows=True) of the concert's file tuple for tuple, feed 2 yields no segment, and every segment comes out of the
    push that delivers its closing window: the first strong window behind its last one, or window last + max_gap + 1"""
    x = ref.concert_b() if "concert_b" in case else ref.concert_a()
    kw = dict(tempos=TEMPOS, shifts=SHIFTS) if "variants" in case else {}
    path = str(tmp_path / "concert.wav")
    synth.write_wav(path, x)
    noise = np.clip(np.round(3000.0 * np.random.default_rng(8).standard_normal(x.size)), -32768, 32767).astype(np.int16)
    lsi = _lsi(filters, devices=[0, 0] if "sharded" in case else None)
    try:
        want_segs, want_wins = lsi.timeline(path, min_score=10, windows=True, **kw)
        with pytest.raises(hpfw_amd.HpfwError, match="44.1 kHz") as e:
            lsi.streams(3, min_score=10, rate=48000)
        assert e.value.status == _lib.E_UNSUPPORTED
        assert len(want_segs) >= 2 and len(want_wins) == _lib.window_count(x.size, 220500, 110250)
        rng = np.random.default_rng(9)
        segs, wins, delivered, returned = {0: [], 1: [], 2: []}, {0: [], 1: [], 2: []}, {}, {}
        with lsi.streams(3, min_score=10, windows=True, **kw) as live:
            at, push = [0, 0, 0], 0
            while at[0] < x.size or at[1] < x.size:
                n0 = int(rng.integers(0, 3 * synth.SR + 1))
                n1 = 0 if push < 7 else synth.SR // 2
                chunks = {0: x[at[0]:at[0] + n0], 2: noise[at[2]:at[2] + n0]}
                if n1:
                    chunks[1] = x[at[1]:at[1] + n1]
                at = [min(at[0] + n0, x.size), min(at[1] + n1, x.size), min(at[2] + n0, x.size)]
                new, rows = live.push(chunks)
                for f, w, row in rows:
                    assert w == len(wins[f])
                    wins[f].append(row)
                    delivered[f, w] = push
                for f, sg in new:
                    returned[f, len(segs[f])] = push
                    segs[f].append(sg)
                now = live.open()
                assert now[2] is None and len(now) == 3
                push += 1
            mid = {f: len(s) for f, s in segs.items()}
            for f, sg in live.finish():
                segs[f].append(sg)
            assert live.open() == [None, None, None] and live.finish() == []
        n_w = len(want_wins)
        strong = [w for w, row in enumerate(want_wins) if row[0] is not None and row[4] >= 10]
        for f in (0, 1):
            assert segs[f] == want_segs, (case, f, segs[f], want_segs)
            assert len(wins[f]) == n_w
            for w, (g, t) in enumerate(zip(wins[f], want_wins)):
                assert g == t or (g[0] is None and t[0] is None), (case, f, w, g, t)
            for i, sg in enumerate(want_segs):
                last = int(round((sg[1] - 5.0) / 2.5))
                closer = min([w for w in strong if w > last][:1] + [last + 1 + 1])           # max_gap = 1
                if closer < n_w:
                    assert returned[f, i] == delivered[f, closer], (case, f, i, closer)
                else:
                    assert i >= mid[f]                                                      # only finish() can release it
        assert segs[2] == [] and len(wins[2]) == n_w
    finally:
        lsi._gpu.close()
