"""The time warp and the fused mix on the MI355X (k_warp.hip): bitwise against the numpy restatement of
tests/warp_ref.py -- every output length, source length, placement, step, fraction and output origin the contract names at
least once -- the mix against the mix of materialised tracks, chunked rendering, a side stream, and every invalid argument."""
import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib

import warp_ref as ref

pytestmark = pytest.mark.gpu

T = ref.T
PPM12 = 13194140                                                     # 12 ppm in 2^-40 per sample
F_MAX = (1 << 40) - 1
M_FAR = (1 << 31) - 6000


@pytest.fixture(scope="module")
def wg(torch_cuda):
    g = hpfw_amd.Gpu(0)
    yield g
    g.close()


def _noise(seed, n):
    return np.random.default_rng(seed).integers(-32768, 32768, size=n).astype(np.int16)


def _tracks(rows):
    """rows of (src_off, src_len, i0, f0, d, gain)"""
    t = np.zeros(len(rows), _lib.WARP_TRACK_DTYPE)
    for k, r in enumerate(rows):
        t[k] = tuple(int(v) for v in r) + (0,)
    return t


def _check(wg, src, i0, f0, d, m0, n_out, gain=1):
    got = wg.warp(src, _tracks([(0, src.size, i0, f0, d, gain)]), m0, n_out)
    want = ref.warp(src, i0, f0, d, m0, n_out, gain)
    assert got.shape == (1, n_out)
    assert np.array_equal(got[0], want), (src.size, i0, f0, d, m0, n_out, int(np.count_nonzero(got[0] != want)))
    return got[0]


def test_table_on_the_device_is_the_library_table(wg):
    """d = 0 reads one row for all outputs: every 64th row through a fixed fraction"""
    x = _noise(1, 300)
    taps = _lib.warp_table()
    for p in range(0, ref.P, 64):
        f0 = p << 28
        got = wg.warp(x, _tracks([(0, x.size, 0, f0, 0, 1)]), 0, 300)[0]
        assert np.array_equal(got, ref.warp(x, 0, f0, 0, 0, 300, 1, taps)), p


@pytest.mark.parametrize("n_out", (1, 255, 256, 2047, 2049, 6000))
def test_output_lengths(wg, n_out):
    """a tile is 2048 outputs: below, at and above one tile, and a ragged third tile; the source crosses the output's end"""
    src = _noise([2, n_out], 4097)
    for d, f0 in ((PPM12, 1), (-(1 << 30), F_MAX), (1 << 30, 0)):
        _check(wg, src, -3, f0, d, 0, n_out)


@pytest.mark.parametrize("src_len", (1, T - 1, 4097, 70001))
def test_source_lengths_and_placements(wg, src_len):
    """the track before, inside, across either end of and wholly outside the outputs 0 .. 5999"""
    src = _noise([3, src_len], src_len)
    n_out = 6000
    # source sample j lands on output j - i0
    places = {"across the start": src_len // 2, "inside": -1000, "across the end": -(n_out - src_len // 2 - 1),
              "outside, after": -(n_out + 100), "outside, before": src_len + T + 5}
    for (what, i0), (d, f0) in zip(places.items(), ((-1, 1), (PPM12, F_MAX), (-PPM12, 0), (1 << 30, 1), (-(1 << 30), F_MAX))):
        got = _check(wg, src, i0, f0, d, 0, n_out)
        if what.startswith("outside"):
            assert not got.any(), what
        elif src_len > T:
            assert got.any(), what


def test_every_step_and_fraction(wg):
    src = _noise(4, 4097)
    for d in (0, 1, -1, PPM12, -PPM12, 1 << 30, -(1 << 30)):
        for f0 in (0, 1, F_MAX):
            _check(wg, src, -50, f0, d, 0, 2049)


def test_negative_step_crossing_zero(wg):
    """u = f0 + m d goes from positive through 0 to negative: the shift is a floor, the phase wraps to the top rows"""
    src = _noise(5, 4097)
    for d, f0 in ((-1, 1), (-PPM12, 100 * PPM12 + 5), (-(1 << 30), (1 << 30) * 3 + 7), (-(1 << 30), 0)):
        u = f0 + np.arange(2049, dtype=np.int64) * d
        assert (u < 0).any() and u[0] >= 0
        _check(wg, src, 10, f0, d, 0, 2049)


@pytest.mark.parametrize("d", (1 << 30, -(1 << 30)))
def test_far_outputs(wg, d):
    """m0 = 2^31 - 6000: m d is near 2^61, the position near 2^31 +- 2^21"""
    src = _noise(6, 70001)
    m_mid = M_FAR + 3000
    i0 = -(m_mid + ((m_mid * d) >> 40)) + 30000                       # the middle output reads sample 30000
    for f0 in (0, F_MAX):
        got = _check(wg, src, i0, f0, d, M_FAR, 6000)
        assert got.any()
    _check(wg, src, 0, 1, d, 0, 6000)                                 # and m0 = 0 at the same step


def test_source_at_an_odd_offset(wg):
    buf = _noise(7, 9000)
    for off in (1, 3, 7, 8, 4099):
        for d in (0, PPM12, -(1 << 30)):
            got = wg.warp(buf, _tracks([(off, 4097, -5, 1, d, 1)]), 0, 4200)[0]
            assert np.array_equal(got, ref.warp(buf[off:off + 4097], -5, 1, d, 0, 4200)), (off, d)


def test_full_scale_squares_reach_both_rails(wg):
    t = np.arange(4097)
    for period in (7, 44):
        sq = np.where((t // period) % 2 == 0, 32767, -32768).astype(np.int16)
        got = _check(wg, sq, 0, 1 << 39, PPM12, 0, 4000)
        assert (got == 32767).any() and (got == -32768).any()
        raw = ref.raw(sq, 0, 1 << 39, PPM12, 0, 4000)
        assert raw.max() > 32767 and raw.min() < -32768              # the clamp worked on both sides


def test_negative_gain_negates_before_the_clamp(wg):
    src = np.full(200, -32768, np.int16)
    for g in (-1, -(1 << 15), -(1 << 17)):
        got = _check(wg, src, 0, 0, 0, 0, 200, g)
        assert (got[T:-T] == 32767).all()                              # +32768 clamps
    assert (_check(wg, src, 0, 0, 0, 0, 200, 5)[T:-T] == -32768).all()
    x = _noise(8, 3000)
    assert np.array_equal(_check(wg, x, 3, 12345, PPM12, 0, 3000, -7), np.clip(-ref.raw(x, 3, 12345, PPM12, 0, 3000), -32768, 32767))


def test_three_tracks_of_different_lengths_in_one_launch(wg):
    parts = [_noise([9, n], n) for n in (1, 4097, 70001)]
    buf = np.concatenate(parts)
    offs = np.concatenate([[0], np.cumsum([p.size for p in parts])])
    maps = ((5, 0, 0), (-100, 1, -PPM12), (-3000, F_MAX, 1 << 30))
    tr = _tracks([(offs[k], parts[k].size) + maps[k] + ((-1) ** k,) for k in range(3)])
    got = wg.warp(buf, tr, 0, 6000)
    for k in range(3):
        assert np.array_equal(got[k], ref.warp(parts[k], *maps[k], 0, 6000, (-1) ** k)), k


def test_identity_map_is_the_shifted_source(wg):
    x = _noise(10, 4097)
    for i0 in (0, 5, -5, 4000, -2100):
        got = wg.warp(x, _tracks([(0, x.size, i0, 0, 0, 1)]), 0, 6000)[0]
        m = np.arange(6000) + i0
        want = np.where((m >= 0) & (m < x.size), x[np.clip(m, 0, x.size - 1)], 0)
        assert np.array_equal(got, want), i0


def test_device_entry_points_on_a_side_stream(wg, torch_cuda):
    torch = torch_cuda
    parts = [_noise([11, n], n) for n in (4097, 5001)]
    pad = 3
    buf = np.concatenate([np.zeros(pad, np.int16)] + parts)
    maps = ((-7, 1, PPM12), (20, F_MAX, -(1 << 30)))
    tr = _tracks([(pad, 4097) + maps[0] + (1 << 14,), (pad + 4097, 5001) + maps[1] + (-(1 << 14),)])
    n_out = 4200
    d_pcm = torch.from_numpy(buf).cuda()
    d_out = torch.full((2 * n_out + 3,), 7, dtype=torch.int16, device="cuda")
    d_mix = torch.full((n_out + 3,), 7, dtype=torch.int16, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        wg.warp_dev(d_pcm.data_ptr(), buf.size, tr, 0, n_out, d_out.data_ptr(), side.cuda_stream)
        wg.mix_dev(d_pcm.data_ptr(), buf.size, tr, 0, n_out, d_mix.data_ptr(), side.cuda_stream)
        ev = torch.cuda.Event()
        ev.record(side)
    torch.cuda.current_stream().wait_event(ev)
    got, mix = d_out.cpu().numpy(), d_mix.cpu().numpy()
    assert np.array_equal(got[:n_out], ref.warp(parts[0], *maps[0], 0, n_out, 1))
    assert np.array_equal(got[n_out:2 * n_out], ref.warp(parts[1], *maps[1], 0, n_out, -1))
    assert np.array_equal(mix[:n_out], ref.mix(parts, maps, [1 << 14, -(1 << 14)], 0, n_out))
    assert (got[2 * n_out:] == 7).all() and (mix[n_out:] == 7).all()  # nothing written past the outputs


# ---- the fused mix -----------------------------------------------------------------------------------------------------
def _mix_case(n_tracks, gains, n_out, seed):
    """tracks of ragged lengths laid so that some tiles are met by all, some by a few and the last ones by none"""
    rng = np.random.default_rng(seed)
    parts = [_noise([seed, k], int(rng.integers(3000, 5000))) for k in range(n_tracks)]
    offs = np.concatenate([[0], np.cumsum([p.size for p in parts])])
    steps = (0, PPM12, -PPM12, 1 << 30, -(1 << 30), 1, -1, 5 * PPM12, -7 * PPM12)
    maps = [(-4096 - 100 * k, int(rng.integers(0, 1 << 40)), steps[k % len(steps)]) for k in range(n_tracks)]
    tr = _tracks([(offs[k], parts[k].size) + maps[k] + (gains[k],) for k in range(n_tracks)])
    return np.concatenate(parts), parts, maps, tr


@pytest.mark.parametrize("n_tracks", (1, 2, 9))
def test_mix_equals_the_mix_of_the_tracks(wg, n_tracks):
    big = (1 << 17, -(1 << 17), 0, 1, -1, 1 << 15, -12345, 3640, 1 << 17)
    n_out = 6 * 2048 + 77                                             # tile 0: no track; tile 2: all; later: some, then none
    for gains in (big[:n_tracks], big[::-1][:n_tracks], (1 << 17,) * n_tracks):
        buf, parts, maps, tr = _mix_case(n_tracks, gains, n_out, 12)
        mix = wg.mix(buf, tr, 0, n_out)
        plain = tr.copy()
        plain["gain"] = 1                                             # the tracks before their sign
        assert np.array_equal(mix, ref.mix_tracks(wg.warp(buf, plain, 0, n_out), gains))
        assert np.array_equal(mix, ref.mix(parts, maps, gains, 0, n_out))
        assert not mix[:4000].any() and not mix[-2048:].any()         # tiles no track meets are zeros
        if any(gains):
            assert mix.any()
    if n_tracks == 9:
        assert (mix == 32767).any() and (mix == -32768).any()         # nine full gains clip


def test_mix_in_chunks_equals_one_call(wg):
    gains = (20000, -20000, 9000, 1 << 15, -3000)
    buf, parts, maps, tr = _mix_case(5, gains, 0, 13)
    n_out = 3 * 4096 + 1000
    whole = wg.mix(buf, tr, 0, n_out)
    pieces = [wg.mix(buf, tr, m0, min(4096, n_out - m0)) for m0 in range(0, n_out, 4096)]
    assert np.array_equal(np.concatenate(pieces), whole)
    tracks = [wg.warp(buf, tr, m0, min(4096, n_out - m0)) for m0 in range(0, n_out, 4096)]
    assert np.array_equal(np.concatenate(tracks, axis=1), wg.warp(buf, tr, 0, n_out))
    assert np.array_equal(wg.mix(buf, tr[:0], 0, 3000), np.zeros(3000, np.int16))     # no track: silence


def test_far_mix(wg):
    src = _noise(14, 70001)
    d = 1 << 30
    m_mid = M_FAR + 3000
    maps = [(-(m_mid + ((m_mid * d) >> 40)) + 30000, 5, d), (-(m_mid + ((m_mid * -d) >> 40)) + 100, F_MAX, -d)]
    tr = _tracks([(0, src.size) + maps[0] + (1 << 15,), (1, 5000) + maps[1] + (-(1 << 15),)])
    got = wg.mix(src, tr, M_FAR, 6000)
    assert np.array_equal(got, ref.mix([src, src[1:5001]], maps, [1 << 15, -(1 << 15)], M_FAR, 6000)) and got.any()


# ---- invalid arguments -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", (False, True))
def test_every_invalid_argument_is_refused(wg, mix):
    buf = _noise(15, 1000)
    call = wg.mix if mix else wg.warp
    good = (0, 1000, 0, 0, 0, 1)
    call(buf, _tracks([good]), 0, 10)
    bad_tracks = {
        "range past the buffer": (1, 1000, 0, 0, 0, 1), "offset past the buffer": (1001, 0, 0, 0, 0, 1), "negative offset": (-1, 10, 0, 0, 0, 1),
        "negative length": (0, -1, 0, 0, 0, 1), "d above": (0, 1000, 0, 0, (1 << 30) + 1, 1), "d below": (0, 1000, 0, 0, -(1 << 30) - 1, 1),
        "f0 negative": (0, 1000, 0, -1, 0, 1), "f0 at 2^40": (0, 1000, 0, 1 << 40, 0, 1), "gain above": (0, 1000, 0, 0, 0, (1 << 17) + 1),
        "gain below": (0, 1000, 0, 0, 0, -(1 << 17) - 1), "i0 above": (0, 1000, (1 << 62) + 1, 0, 0, 1),
    }
    for what, row in bad_tracks.items():
        with pytest.raises(hpfw_amd.HpfwError) as e:
            call(buf, _tracks([good, row]), 0, 10)
        assert e.value.status == _lib.E_INVALID and "track 1" in str(e.value), what
    for m0, n_out in ((-1, 10), (0, -1), ((1 << 31) - 9, 10), (1 << 31, 1), (0, (1 << 31) + 1)):
        with pytest.raises(hpfw_amd.HpfwError) as e:
            call(buf, _tracks([good]), m0, n_out)
        assert e.value.status == _lib.E_INVALID, (m0, n_out)
    # the limits themselves are accepted
    ok = _tracks([(0, 1000, -(1 << 62), F_MAX, 1 << 30, 1 << 17), (1000, 0, 1 << 62, 0, -(1 << 30), -(1 << 17))])
    assert not call(buf, ok, (1 << 31) - 10, 10).any()
    L = hpfw_amd.lib()
    out = np.zeros(10, np.int16)
    tr = _tracks([good])
    p = lambda a: a.ctypes.data_as(__import__("ctypes").c_void_p)    # noqa: E731
    fn = L.hpfw_gpu_mix_pcm16_host if mix else L.hpfw_gpu_warp_pcm16_host
    assert fn(None, p(buf), 1000, p(tr), 1, 0, 10, p(out)) == _lib.E_INVALID
    assert fn(wg._h, None, 1000, p(tr), 1, 0, 10, p(out)) == _lib.E_INVALID
    assert fn(wg._h, p(buf), 1000, None, 1, 0, 10, p(out)) == _lib.E_INVALID
    assert fn(wg._h, p(buf), 1000, p(tr), 1, 0, 10, None) == _lib.E_INVALID
    assert fn(wg._h, p(buf), -1, p(tr), 1, 0, 10, p(out)) == _lib.E_INVALID
    assert fn(wg._h, p(buf), 1000, p(tr), -1, 0, 10, p(out)) == _lib.E_INVALID
