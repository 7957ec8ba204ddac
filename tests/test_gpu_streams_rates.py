"""Live feeds at other rates than 44.1 kHz on the GPU: the rings of feeds at seven rates, pushed in chunks of
0, 1, fewer than T and a few thousand samples, against the offline conversion of the whole feed (tests/resample_ref.py with the
library's table) sample for sample and hashprint for hashprint; both clamps; a push that does not fit; a feed that reconnects;
and LiveStreams at 48 kHz against LiveSongIdentification.timeline() of the same audio as a 48 kHz file."""
from math import gcd

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, synth

import resample_ref as rs
import timeline_ref as ref

pytestmark = pytest.mark.gpu
SHIFTS, TEMPOS = [-2, 0, 2], [0.96, 1.0, 1.04]
RATES = [48000, 44100, 32000, 96000, 44056, 22050, 8000]      # 44 056 Hz: the table that does not fit the LDS
SECONDS = (7.0, 5.3, 7.0, 5.3, 7.0, 1.5, 7.0)                 # the sixth feed never completes a window of 2 s
_TAPS = {}


def _taps(fs):
    """the library's own table: a 1-LSB difference between the C and the numpy design is not a kernel error"""
    if fs not in _TAPS:
        _TAPS[fs] = hpfw_amd.resample_table(fs)[2]
    return _TAPS[fs]


def _h(fs):
    return 0 if fs == 44100 else rs.half_taps(fs)


def emitted(n, fs):
    if fs == 44100:
        return n
    L, M = rs.ratio(fs)
    H = rs.half_taps(fs)
    return 0 if n <= H else -(-(n - H) * L // M)


def _whole(x, fs):
    """the feed at 44.1 kHz as the offline resampler gives it for everything pushed"""
    return x.copy() if fs == 44100 else rs.resample(x, fs, _taps(fs))


def _at_rate(x44, fs):
    """an independent float conversion of a 44.1 kHz clip to fs (scipy's polyphase FIR), rounded to int16"""
    if fs == 44100:
        return x44
    from scipy.signal import resample_poly
    g = gcd(44100, fs)
    return np.clip(np.round(resample_poly(x44.astype(np.float64), fs // g, 44100 // g)), -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def feeds():
    """[(rate, the feed at its rate, the feed converted as one clip)], computed once and left unchanged"""
    out = []
    for i, (fs, s) in enumerate(zip(RATES, SECONDS)):
        x = _at_rate(synth.gen_clip(700 + i, 30.0)[:int(round(s * synth.SR))], fs)
        out.append((fs, x, _whole(x, fs)))
        for a in out[-1][1:]:
            a.setflags(write=False)
    return out


def _direct(gpu, w, tempos, shifts):
    if tempos is not None:
        return gpu.extract_tempo(w, tempos, shifts)
    return gpu.extract_transposed(w, shifts) if shifts is not None else gpu.extract(w)


def _drive(gpu, torch, feeds, win, hop, form, seed, tempos=None, shifts=None, max_chunk=5000, slow=0):
    """pushes the feeds in seeded random chunks of 0 .. round(max_chunk fs / 44100) input samples, differing between the feeds of
    one push (sizes 0 and 1 forced on one feed every fifth push; feed `slow` fed one sample at a time for 3 T pushes from push 10
    on), and extracts after every push, alternately one window at a time and all at once.  After every push emitted() is the
    formula.  Returns per feed ([window numbers], [clips], [hashprints]) and how often each ring wrapped."""
    rng = np.random.default_rng(seed)
    capacity = win + 5000
    rates = [fs for fs, _, _ in feeds]
    xs = [x for _, x, _ in feeds]
    s = gpu.streams(len(feeds), win, hop, capacity, tempos, shifts, rates=rates)
    got = [([], [], []) for _ in feeds]
    try:
        assert list(s.rates) == rates and (s.capacity, s.n_streams, s.win, s.hop) == (capacity, len(feeds), win, hop)
        at = [0] * len(feeds)
        push = 0
        one_by_one = range(10, 10 + 6 * _h(rates[slow]))
        while any(a < x.size for a, x in zip(at, xs)):
            sizes = [int(min(rng.integers(0, int(round(max_chunk * fs / 44100)) + 1), x.size - a)) for a, x, fs in zip(at, xs, rates)]
            if push % 5 == 0:
                k = push // 5 % len(feeds)
                sizes[k] = min(push // 5 % 2, xs[k].size - at[k])                # (sizes 0 and 1 occur for certain)
            if push in one_by_one:
                sizes[slow] = min(1, xs[slow].size - at[slow])
            chunks = [x[a:a + n] for a, x, n in zip(at, xs, sizes)]
            assert (s.room() >= np.array(sizes)).all()
            if form == "host":
                ready = s.push([c if c.size else None for c in chunks])
            else:
                flat = torch.from_numpy(np.concatenate(chunks + [np.zeros(1, np.int16)])).cuda()
                ready = s.push_dev(flat.data_ptr(), sizes)
                torch.cuda.synchronize()
            at = [a + n for a, n in zip(at, sizes)]
            n_i, e_i = s.info()
            assert list(n_i) == at                                               # received stays "samples pushed"
            em = [emitted(a, fs) for a, fs in zip(at, rates)]
            assert list(s.emitted()) == em, (push, at)
            assert ready == sum(_lib.window_count(m, win, hop) - int(e) for m, e in zip(em, e_i)) == s.ready()
            while ready:
                cap = 1 if push % 2 else ready
                if form == "host":
                    which, hp, clips = s.extract(cap, clips=True)
                else:
                    d_hp = torch.zeros(s._hp_shape(cap), dtype=torch.int64, device="cuda")
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
                assert s.ready() == ready
            push += 1
        assert s.extract()[0].size == 0
        wraps = [int(m) // capacity for m in s.emitted()]
    finally:
        s.close()
    return got, wraps


def _expected(gpu, feeds, win, hop, tempos=None, shifts=None):
    """per feed (windows int16 [n_w][win], their hashprints) of the converted feed cut at what it has emitted"""
    out = []
    for fs, x, y in feeds:
        w = ref.windows_of(y[:emitted(x.size, fs)], win, hop)
        out.append((w, _direct(gpu, w, tempos, shifts) if w.shape[0] else None))
    return out


def _same(got, want, what):
    for f, ((wins, clips, hps), (w_want, hp_want)) in enumerate(zip(got, want)):
        assert wins == list(range(w_want.shape[0])), (what, f, wins)
        if wins:
            diff = np.stack(clips) != w_want
            assert not diff.any(), (what, f, int(diff.sum()), np.argwhere(diff)[:4].tolist())
            assert np.array_equal(np.stack(hps), hp_want), (what, f)


@pytest.mark.parametrize("win", [88200, 88201])
def test_rings_hold_the_offline_conversion(gpu, torch_cuda, feeds, win):
    """seven feeds at 48, 44.1, 32, 96, 44.056, 22.05 and 8 kHz in rings of win + 5000 samples that all wrap: the clips of every
    window equal the windows of the feed converted as one clip, the hashprints those of gpu.extract on them, from host and from
    device pointers, with shifts and tempos together, and in projection mode 0; the 44.1 kHz feed equals its input"""
    assert _lib.supported_length(win) == win
    assert np.array_equal(feeds[1][1], feeds[1][2])
    for hop in (44100, 9973):
        want = _expected(gpu, feeds, win, hop)
        assert [w.shape[0] >= 2 for w, _ in want] == [True, True, True, True, True, False, True]
        assert np.array_equal(want[1][0], ref.windows_of(feeds[1][1], win, hop))       # the 44.1 kHz feed: its input windows
        for k, form in enumerate(("host", "device")):
            slow = (0, 3, 4, 6)[(2 * (hop == 9973) + k + win) % 4]                     # 48, 96, 44.056 and 8 kHz in turn
            got, wraps = _drive(gpu, torch_cuda, feeds, win, hop, form, seed=hop % 1000 + k, slow=slow)
            assert all(n >= 2 for i, n in enumerate(wraps) if i != 5), wraps
            _same(got, want, (win, hop, form))
    hop = 9973
    got, _ = _drive(gpu, torch_cuda, feeds, win, hop, "device", seed=5, tempos=TEMPOS, shifts=SHIFTS, slow=2)
    _same(got, _expected(gpu, feeds, win, hop, TEMPOS, SHIFTS), (win, "variants"))
    gpu.set_projection(0)
    try:
        got, _ = _drive(gpu, torch_cuda, feeds, win, hop, "host", seed=6, slow=6)
        _same(got, _expected(gpu, feeds, win, hop), (win, "projection 0"))
    finally:
        gpu.set_projection(1)


def _square():
    """alternating blocks of +-32768 ... 32767 at 48 kHz: the filter's overshoot at every edge passes both ends of int16"""
    t = np.arange(110411)
    return np.where((t // 48) % 2 == 0, 32767, -32768).astype(np.int16)


def test_both_clamps_occur(gpu):
    """a full-scale square wave at 48 kHz pushed in chunks smaller than H: the ring holds the clamped values of the restatement"""
    fs, win, hop = 48000, 88200, 9973
    H = rs.half_taps(fs)
    x = _square()
    y = _whole(x, fs)
    assert (y == 32767).any() and (y == -32768).any()
    acc_free = rs.resample(x // 2, fs, _taps(fs)).astype(np.int64) * 2               # (half scale does not clamp: the full one must)
    assert (acc_free > 32767).any() and (acc_free < -32768).any()
    s = gpu.streams(1, win, hop, win + 5000, rates=fs)
    clips = []
    try:
        rng = np.random.default_rng(3)
        at = 0
        while at < x.size:
            n = int(rng.integers(1, H))
            if s.push([x[at:at + n]]):
                clips += list(s.extract(clips=True)[2])
            at += n
        assert list(s.emitted()) == [emitted(x.size, fs)]
    finally:
        s.close()
    want = ref.windows_of(y[:emitted(x.size, fs)], win, hop)
    assert want.shape[0] >= 2 and np.array_equal(np.stack(clips), want)
    assert (want == 32767).any() and (want == -32768).any()


def test_refused_push_moves_nothing_and_reset_forgets_the_history(gpu, feeds):
    """a push beyond room() is refused as a whole with the feed named: nothing was appended and no history moved, so the pushes
    that follow still give the bits of the whole feed; a feed reset in mid-stream then gives the windows of the new signal alone"""
    win, hop = 88200, 44100
    (fa, a, ya), (fb, b, yb) = feeds[0], feeds[2]                                     # 48 kHz, 32 kHz
    c = _at_rate(synth.gen_clip(720, 30.0)[:4 * synth.SR], fb)
    s = gpu.streams(2, win, hop, rates=[fa, fb])                                      # capacity 0: two windows
    got = ([], [])
    try:
        def take():
            which, hp, clips = s.extract(clips=True)
            for w, x in zip(which, clips):
                got[int(w["feed"])].append((int(w["window"]), x.copy()))

        L, M = rs.ratio(fb)
        assert list(s.room()) == [_h(f) + 2 * win * rs.ratio(f)[1] // rs.ratio(f)[0] for f in (fa, fb)]
        s.push([a[:50001], b[:30001]])
        before, room = (s.info(), s.emitted()), s.room()
        assert list(room) == [_h(f) + 2 * win * rs.ratio(f)[1] // rs.ratio(f)[0] - n for f, n in ((fa, 50001), (fb, 30001))]
        with pytest.raises(hpfw_amd.HpfwError, match="feed 1") as e:
            s.push([a[50001:50011], b[30001:30001 + int(room[1]) + 1]])               # feed 0 would fit, feed 1 is one sample too long
        assert e.value.status == _lib.E_INVALID
        after = (s.info(), s.emitted())
        assert all(np.array_equal(p, q) for p, q in zip(before[0] + (before[1],), after[0] + (after[1],)))
        assert np.array_equal(s.room(), room)
        assert s.push([a[50001:50011], b[30001:30001 + int(room[1])]]) >= 1           # exactly full is accepted
        assert s.room()[1] == 0 and s.emitted()[1] <= 2 * win < emitted(30001 + int(room[1]) + 1, fb)
        take()
        at_a, at_b = 50011, 30001 + int(room[1])
        while at_a < 4 * fa:
            s.push([a[at_a:at_a + 30000], b[at_b:at_b + 20000]])
            at_a, at_b = at_a + 30000, min(at_b + 20000, b.size)
            take()
        n_b = len(got[1])
        s.reset(1)                                                                    # in mid-stream: the ring part full, a history in place
        assert list(s.info()[0]) == [at_a, 0] and s.emitted()[1] == 0 and s.room()[1] == _h(fb) + 2 * win * M // L
        for at_c in range(0, c.size, 7001):
            s.push([None, c[at_c:at_c + 7001]])
            take()
    finally:
        s.close()
    want_a = ref.windows_of(ya[:emitted(at_a, fa)], win, hop)
    assert [w for w, _ in got[0]] == list(range(want_a.shape[0])) and np.array_equal(np.stack([x for _, x in got[0]]), want_a)
    want_b = ref.windows_of(yb[:emitted(at_b, fb)], win, hop)
    yc = _whole(c, fb)
    assert np.count_nonzero(yc[:_h(fb)]) > 0                                          # the outputs that read in front of the feed's start
    want_c = ref.windows_of(yc[:emitted(c.size, fb)], win, hop)
    assert n_b == want_b.shape[0] >= 2 and want_c.shape[0] >= 2
    assert [w for w, _ in got[1]] == list(range(n_b)) + list(range(want_c.shape[0]))
    assert np.array_equal(np.stack([x for _, x in got[1]]), np.concatenate([want_b, want_c]))


# ---- end to end ---------------------------------------------------------------------------------------------------------------
N_SONGS = 20


def _lsi(filters, devices=None, resample=True):
    lsi = hpfw_amd.LiveSongIdentification(devices=devices, resample=resample)
    ext = lsi.collector.gpu()
    ext.set_filters(filters)
    hp = ext.extract(np.stack([synth.gen_clip(i, 30.0) for i in range(N_SONGS)]))
    lsi.build([(hp[i], f"song{i:02d}") for i in range(N_SONGS)])
    return lsi


@pytest.fixture(scope="module")
def concert_48k(tmp_path_factory):
    x = _at_rate(ref.concert_a(), 48000)
    path = str(tmp_path_factory.mktemp("live48") / "concert_a_48k.wav")
    synth.write_wav(path, x, rate=48000)
    return path, x


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one_index", "sharded"])
def test_48k_feeds_equal_the_timeline_of_the_48k_file(concert_48k, filters, torch_cuda, devices):
    """feed 0: the 48 kHz concert in random chunks of up to 3 s, then H zeros; feed 1: the same in chunks of 0.5 s, started 7
    pushes later, then H zeros; feed 2: white noise at 44.1 kHz.  Segments and per-window rows of feeds 0 and 1 equal
    timeline(windows=True) of the 48 kHz file under resample=True tuple for tuple; feed 2 yields nothing"""
    path, x = concert_48k
    fs = 48000
    noise = np.clip(np.round(3000.0 * np.random.default_rng(8).standard_normal(x.size)), -32768, 32767).astype(np.int16)
    lsi = _lsi(filters, devices)
    try:
        want_segs, want_wins = lsi.timeline(path, min_score=10, windows=True)
        assert len(want_segs) >= 2 and len(want_wins) == _lib.window_count(rs.out_length(x.size, fs), 220500, 110250)
        rng = np.random.default_rng(9)
        segs, wins = {0: [], 1: [], 2: []}, {0: [], 1: [], 2: []}
        with lsi.streams(3, min_score=10, windows=True, rate=[fs, fs, 44100]) as live:
            assert live.rates == [fs, fs, 44100] and [live.tail(f) for f in range(3)] == [rs.half_taps(fs)] * 2 + [0]
            tail = np.zeros(live.tail(0), np.int16)
            at, push, tails = [0, 0, 0], 0, [False, False]
            while not all(tails):
                n0 = int(rng.integers(0, 3 * fs + 1))
                n1 = 0 if push < 7 else fs // 2
                chunks = {2: noise[at[2]:at[2] + n0 * 441 // 480]}
                for f, n in ((0, n0), (1, n1)):
                    if at[f] < x.size:
                        chunks[f] = x[at[f]:at[f] + n]
                    elif not tails[f]:
                        chunks[f], tails[f] = tail, True
                at = [min(at[0] + n0, x.size), min(at[1] + n1, x.size), min(at[2] + n0 * 441 // 480, x.size)]
                new, rows = live.push(chunks)
                for f, w, row in rows:
                    assert w == len(wins[f])
                    wins[f].append(row)
                for f, sg in new:
                    segs[f].append(sg)
                push += 1
            for f, sg in live.finish():
                segs[f].append(sg)
        for f in (0, 1):
            assert segs[f] == want_segs, (f, segs[f], want_segs)
            assert len(wins[f]) == len(want_wins)
            for w, (g, t) in enumerate(zip(wins[f], want_wins)):
                assert g == t or (g[0] is None and t[0] is None), (f, w, g, t)
        assert segs[2] == [] and len(wins[2]) >= 2
    finally:
        lsi._gpu.close()


def test_without_the_switch_the_rate_is_refused(filters, torch_cuda):
    lsi = _lsi(filters, resample=False)
    try:
        for rate in (48000, [48000, 48000, 44100]):
            with pytest.raises(hpfw_amd.HpfwError, match="44.1 kHz") as e:
                lsi.streams(3, min_score=10, rate=rate)
            assert e.value.status == _lib.E_UNSUPPORTED and "48000 Hz" in str(e.value)
        with lsi.streams(3, min_score=10, rate=[44100] * 3) as live:                  # 44.1 kHz feeds need no switch
            assert live.rates == [44100] * 3
        with pytest.raises(hpfw_amd.HpfwError) as e:
            lsi.collector.gpu().streams(2, 88200, 44100, rates=[48000, 7999])
        assert e.value.status == _lib.E_UNSUPPORTED and "feed 1" in str(e.value)
    finally:
        lsi._gpu.close()
