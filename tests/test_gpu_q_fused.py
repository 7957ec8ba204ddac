"""The six-product hashprint kernel that settles its open values itself (k_project_q.hip):
the default handle against a HPFW_Q_PRODUCTS=9 handle (the nine-product kernel) and the oracle.  Every case first shows on the CPU, with
q_products_ref.split, that its input reaches what it is about: bits that the list path has to flip, where in a tile they
lie, tiles above the cap with wrong signs of Dp, the three tile states in one launch.

The inputs: a dB spectrogram of uniform noise has a few open values in ten thousand; a stretch of 99 + j columns whose
quantised values differ by less than 128 (`one_digit`) leaves j hashprints whose Du has one digit in the whole window --
Dp is then the sum of a2 b0 alone, all 64 rows are open and in about one of a hundred the sign of Dp is wrong.
The seeds were searched on the CPU so that the assertions on the input hold."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q_products_ref as ref  # noqa: E402
import hpfw_amd  # noqa: E402
from hpfw_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

WINDOW = ref.CTX + ref.LAG - 1         # a hashprint reads columns n .. n + 99


def handle(env, filt):
    os.environ.update(env)
    try:
        g = hpfw_amd.Gpu(0)
    finally:
        for k in env:
            os.environ.pop(k, None)
    g.set_filters(filt)
    return g


@pytest.fixture(scope="module")
def pair(torch_cuda, filters):
    """(default: six products, the open values settled in the kernel; nine products)"""
    gs = [handle(env, filters) for env in ({}, {"HPFW_Q_PRODUCTS": "9"})]
    yield gs
    for g in gs:
        g.close()


def from_db(torch, g, s):
    n, _, c = s.shape
    d_s = torch.from_numpy(np.ascontiguousarray(s)).cuda()
    hp = torch.zeros((n, c - 99), dtype=torch.int64, device="cuda")
    g.hashprints_from_db_dev(d_s.data_ptr(), n, c, hp.data_ptr())
    torch.cuda.synchronize()
    return hp.cpu().numpy().view(np.uint64)


def all_agree(torch, pair, oracle, filt, s):
    """hashprints of the default handle, equal to those of the nine-product handle and of the oracle"""
    got = from_db(torch, pair[0], s)
    assert np.array_equal(got, from_db(torch, pair[1], s)), "nine products"
    for i in range(s.shape[0]):
        assert np.array_equal(got[i], oracle.hashprints_from_db(filt, s[i])), i
    return got


def one_digit(rng, shape):
    """dB values around -40 dB whose quantised values differ by less than 128: every difference has one digit"""
    return ((-40 * 98304 + rng.integers(0, 128, shape)) / 98304.0).astype(np.float32)


def stretch(rng, s, a, j):
    """columns a .. a + 98 + j of s [121][c] become a one-digit stretch: hashprints a .. a + j - 1 lie wholly inside"""
    s[:, a:a + WINDOW + j] = one_digit(rng, (121, WINDOW + j))


def cpu_view(oracle, filt, s):
    """per clip (open [64][n], wrong [64][n], counts per tile, zero-slab flags per tile) and the launch's (listed, redone);
    wrong: open values where the sign of Dp is not the sign of D -- the bits the kernel has to flip"""
    clips, listed, redone = [], 0, 0
    for i in range(s.shape[0]):
        d, dp, _, _, is_open, du = ref.split(oracle, filt, s[i])
        wrong = is_open & ((dp >= 0) != (d >= 0))
        starts = range(0, is_open.shape[1], ref.TILE)
        counts = [int(is_open[:, n0:n0 + ref.TILE].sum()) for n0 in starts]
        zero = [not du[:, n0:n0 + ref.TILE + ref.CTX - 1].any() for n0 in starts]
        a, b = ref.tile_states(is_open, du)
        listed, redone = listed + a, redone + b
        clips.append((is_open, wrong, counts, zero))
    return clips, listed, redone


def check_counts(pair, s, listed, redone):
    tiles = s.shape[0] * ((s.shape[2] - 99 + ref.TILE - 1) // ref.TILE)
    assert pair[0].debug_q_products() == (tiles, listed, redone)


# clips per width: about one listed value in a hundred has to be flipped; a stretch of one hashprint opens 64 values and the
# noise around it a few more, so that a tile stays below the cap
LIST_CLIPS = {100: 24, 227: 24, 228: 24, 355: 12}
LIST_SEEDS = {100: 1, 227: 0, 228: 1, 355: 0}


def list_path_input(c, seed):
    """every tile of every clip gets one stretch of one hashprint, 64 open values; stretches keep so far apart that no
    hashprint's window lies in two of them (c = 228: the stretch of the one-hashprint tile in every second clip only)"""
    rng = np.random.default_rng(seed)
    n = LIST_CLIPS[c]
    s = rng.uniform(-80, 0, (n, 121, c)).astype(np.float32)
    for i in range(n):
        if c == 100:
            stretch(rng, s[i], 0, 1)
        elif c == 227:
            stretch(rng, s[i], int(rng.integers(0, 128)), 1)
        elif c == 228:
            if i % 2:
                stretch(rng, s[i], 128, 1)
            else:
                stretch(rng, s[i], int(rng.integers(0, 128)), 1)
        else:
            stretch(rng, s[i], int(rng.integers(0, 11)), 1)
            stretch(rng, s[i], int(rng.integers(200, 256)), 1)
    return s


@pytest.mark.parametrize("c", (100, 227, 228, 355))
def test_list_path_flips_bits(torch_cuda, pair, oracle, filters, c):
    s = list_path_input(c, LIST_SEEDS[c])
    clips, listed, redone = cpu_view(oracle, filters, s)
    counts = [k for _, _, cn, _ in clips for k in cn]
    assert redone == 0 and max(counts) <= ref.CAP and sum(1 for k in counts if k >= 1) >= len(clips)
    assert sum(int(w.sum()) for _, w, _, _ in clips) >= 8               # bits that stand wrong after the six products
    all_agree(torch_cuda, pair, oracle, filters, s)
    check_counts(pair, s, listed, redone)


PLACE_CLIPS, PLACE_SEED = 36, 0
ABOVE_SEED, MIXED_SEED = 3, 0


def placement_input(seed):
    """c = 228, clips in turn: all 64 rows of hashprint 0 open (the first group of 16 of the full tile), of hashprint 127
    (its last group), of hashprint 128 (the last tile of the clip, one hashprint: n_tiles = 1)"""
    rng = np.random.default_rng(seed)
    s = rng.uniform(-80, 0, (PLACE_CLIPS, 121, 228)).astype(np.float32)
    for i in range(PLACE_CLIPS):
        stretch(rng, s[i], (0, 127, 128)[i % 3], 1)
    return s


def test_placement_of_open_values_in_a_tile(torch_cuda, pair, oracle, filters):
    s = placement_input(PLACE_SEED)
    clips, listed, redone = cpu_view(oracle, filters, s)
    assert redone == 0
    wrong = np.stack([w for _, w, _, _ in clips])                       # [clip][row][n]
    is_open = np.stack([o for o, _, _, _ in clips])
    for w in range(4):                                                  # flips in the rows of all four waves
        assert wrong[:, 16 * w:16 * w + 16].any(), w
    assert wrong[:, :, 0:16].any() and wrong[:, :, 112:128].any()       # the first and the last group of a full tile
    assert wrong[:, :, 128].any()                                       # the partial tile
    # two open values of one hashprint in rows of waves 0 and 1 (one 32-bit word of `parts`), one of them to flip; and of waves 2 and 3
    for lo in (0, 32):
        both = is_open[:, lo:lo + 16].any(axis=1) & is_open[:, lo + 16:lo + 32].any(axis=1) & wrong[:, lo:lo + 32].any(axis=1)
        assert both.any(), lo
    # ... and a word in which two bits flip
    assert (wrong[:, 0:32].sum(axis=1) >= 2).any() or (wrong[:, 32:64].sum(axis=1) >= 2).any()
    all_agree(torch_cuda, pair, oracle, filters, s)
    check_counts(pair, s, listed, redone)


def test_above_the_cap_in_a_partial_and_in_a_full_tile(torch_cuda, pair, oracle, filters):
    """one-digit Du everywhere, c = 240: 141 hashprints, a full tile and a last tile of 13 (n_tiles = 1) -- the widths 100,
    227, 228 and 355 have no partial tile of three or more hashprints, and a tile goes above the cap only from three on.
    Then 99 + 3 columns at c = 355: three hashprints, up to 192 open values in a full tile of otherwise uniform noise"""
    rng = np.random.default_rng(3)
    s = one_digit(rng, (2, 121, 240))
    clips, listed, redone = cpu_view(oracle, filters, s)
    assert redone == 4 and listed == 0
    for _, wrong, counts, _ in clips:
        assert min(counts) > ref.CAP and wrong[:, :128].any() and wrong[:, 128:].any()
    all_agree(torch_cuda, pair, oracle, filters, s)
    check_counts(pair, s, listed, redone)

    rng = np.random.default_rng(ABOVE_SEED)
    s = rng.uniform(-80, 0, (2, 121, 355)).astype(np.float32)
    stretch(rng, s[0], 30, 3)
    stretch(rng, s[1], 150, 3)
    clips, listed, redone = cpu_view(oracle, filters, s)
    assert redone == 2 and clips[0][2][0] > ref.CAP and clips[1][2][1] > ref.CAP
    assert clips[0][1][:, 30:33].any() and clips[1][1][:, 150:153].any()           # a wrong sign of Dp in each redone tile
    all_agree(torch_cuda, pair, oracle, filters, s)
    check_counts(pair, s, listed, redone)



def test_zero_listed_and_redone_tiles_in_one_clip(torch_cuda, pair, oracle, filters):
    """c = 483, three full tiles: the -80 dB floor under the first (Du = 0 in its slab), noise under the second, one-digit
    Du from column 255 on: the last hashprint of the second tile and all of the third"""
    rng = np.random.default_rng(MIXED_SEED)
    s = rng.uniform(-80, 0, (2, 121, 483)).astype(np.float32)
    s[:, :, :128 + ref.CTX - 1 + ref.LAG] = -80.0
    s[:, :, 255:] = one_digit(rng, (2, 121, 483 - 255))
    clips, listed, redone = cpu_view(oracle, filters, s)
    for _, wrong, counts, zero in clips:
        assert zero == [True, False, False] and 1 <= counts[1] <= ref.CAP < counts[2]
        assert wrong[:, 256:].any()
    assert sum(int(w[:, 128:256].sum()) for _, w, _, _ in clips) >= 1
    got = all_agree(torch_cuda, pair, oracle, filters, s)
    assert (got[:, :128] == np.uint64(2 ** 64 - 1)).all()
    check_counts(pair, s, listed, redone)


def test_full_dynamic_range_from_the_spectrogram(torch_cuda, pair, oracle, filters):
    """uniform -80 .. 0 dB without a reference level: differences up to 80 dB, all three digits of Du in use"""
    rng = np.random.default_rng(21)
    s = rng.uniform(-80, 0, (3, 121, 355)).astype(np.float32)
    u = oracle.quantise_db(s).astype(np.int64)
    du = u[:, :, :-ref.LAG] - u[:, :, ref.LAG:]
    assert np.abs(du).max() > 75 * 98304 and all(np.abs(d).max() >= 100 for d in ref.digits(du))
    clips, listed, redone = cpu_view(oracle, filters, s)
    all_agree(torch_cuda, pair, oracle, filters, s)
    check_counts(pair, s, listed, redone)


def test_end_to_end_from_pcm(torch_cuda, pair, oracle, filters):
    """2 s of synthetic audio through extract: the kernel's FROM_T instance, the reference level riding on the staging"""
    clip = synth.gen_clip(71, 2.0)[None]
    want = oracle.Plan(clip.shape[1]).extract(filters, clip[0])
    for g in pair:
        assert np.array_equal(g.extract(clip)[0], want)
    assert pair[0].debug_q_products()[0] == (want.size + ref.TILE - 1) // ref.TILE
