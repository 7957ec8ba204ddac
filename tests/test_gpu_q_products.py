"""The six-product hashprint kernel and its fix-up launch (k_project_q.hip) against the oracle and
against a handle created with HPFW_Q_PRODUCTS=9 (the nine-product kernel): tile shapes, inputs that leave many signs
open, the three tile states through the debug counts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q_products_ref as ref  # noqa: E402
import hpfw_amd  # noqa: E402
from hpfw_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = (100, 227, 228, 355)          # 1 hashprint, one full tile, one hashprint behind a full tile, two full tiles


def handle(products, filt):
    os.environ["HPFW_Q_PRODUCTS"] = str(products)
    try:
        g = hpfw_amd.Gpu(0)
    finally:
        os.environ.pop("HPFW_Q_PRODUCTS", None)
    g.set_filters(filt)
    return g


@pytest.fixture(scope="module")
def pair(torch_cuda, filters):
    g6, g9 = handle(6, filters), handle(9, filters)
    yield g6, g9
    g6.close()
    g9.close()


def from_db(torch, g, s):
    n, _, c = s.shape
    d_s = torch.from_numpy(np.ascontiguousarray(s)).cuda()
    hp = torch.zeros((n, c - 99), dtype=torch.int64, device="cuda")
    g.hashprints_from_db_dev(d_s.data_ptr(), n, c, hp.data_ptr())
    torch.cuda.synchronize()
    return hp.cpu().numpy().view(np.uint64)


def both(torch, pair, oracle, filt, s):
    """hashprints of the six-product handle, checked against the nine-product handle and the oracle"""
    g6, g9 = pair
    got = from_db(torch, g6, s)
    assert np.array_equal(got, from_db(torch, g9, s))
    for i in range(s.shape[0]):
        assert np.array_equal(got[i], oracle.hashprints_from_db(filt, s[i])), i
    return got


def expected_states(oracle, filt, s):
    listed = redone = 0
    for i in range(s.shape[0]):
        _, _, _, _, is_open, du = ref.split(oracle, filt, s[i])
        a, b = ref.tile_states(is_open, du)
        listed, redone = listed + a, redone + b
    return listed, redone


@pytest.mark.parametrize("c", SHAPES)
def test_random_floor_and_small_differences(torch_cuda, pair, oracle, filters, c):
    rng = np.random.default_rng(c)
    tiles = 3 * ((c - 99 + 127) // 128)
    s = rng.uniform(-80, 0, (3, 121, c)).astype(np.float32)
    both(torch_cuda, pair, oracle, filters, s)
    assert pair[0].debug_q_products() == (tiles,) + expected_states(oracle, filters, s)
    # the -80 dB floor: Du = 0, every bit one
    got = both(torch_cuda, pair, oracle, filters, np.full((3, 121, c), -80.0, np.float32))
    assert (got == np.uint64(2 ** 64 - 1)).all()
    # differences below 128 / 98304 dB around -40 dB: Du has one digit, the low products decide most signs
    u = -40 * 98304 + rng.integers(0, 128, (3, 121, c))
    s = (u / 98304.0).astype(np.float32)
    assert np.array_equal(oracle.quantise_db(s), u)
    both(torch_cuda, pair, oracle, filters, s)
    listed, redone = expected_states(oracle, filters, s)
    assert pair[0].debug_q_products() == (tiles, listed, redone) and listed + redone > 0


@pytest.mark.parametrize("j", (1, 2, 3))
def test_listed_and_redone_tiles(torch_cuda, pair, oracle, filters, j):
    """a stretch of 99 + j equal columns: j hashprints of the first tile with Du = 0 in their whole window, all 64 rows
    open -- 64 j open values against a cap of 128: listed below and at the cap, the tile redone above it"""
    rng = np.random.default_rng(40 + j)
    s = rng.uniform(-80, 0, (2, 121, 355)).astype(np.float32)
    s[1, :, 30:30 + 99 + j] = s[1, :, 30:31]
    both(torch_cuda, pair, oracle, filters, s)
    _, _, _, lm, is_open, du = ref.split(oracle, filters, s[1])
    assert (lm > 0).all() and is_open[:, 30:30 + j].all()
    listed, redone = expected_states(oracle, filters, s)
    first = int(is_open[:, :128].sum())
    assert first >= 64 * j and (first > ref.CAP) == (redone >= 1)
    if j == 3:
        assert redone >= 1
    if j == 1:
        assert first <= ref.CAP and listed >= 64
    assert pair[0].debug_q_products() == (4, listed, redone)


def test_the_count_exactly_at_the_cap(torch_cuda, pair, oracle, filters):
    """two all-open hashprints and a remainder (Du = 0 or +/- 80 dB) that adds none: exactly 128 values, listed, none redone"""
    rng = np.random.default_rng(14)
    s = rng.choice(np.array([-80.0, 0.0], np.float32), (1, 121, 227))
    s[0, :, 60:60 + 99 + 2] = -3.0
    both(torch_cuda, pair, oracle, filters, s)
    is_open = ref.split(oracle, filters, s[0])[4]
    assert int(is_open.sum()) == ref.CAP and is_open[:, 60:62].all()
    assert pair[0].debug_q_products() == (1, ref.CAP, 0)


def test_second_set_filters_and_more_than_one_pass(torch_cuda, oracle, filters):
    """the int32 table follows a second set_filters; 300 clips are more than one internal pass of 256"""
    rng = np.random.default_rng(5)
    f2 = (rng.standard_normal(2420 * 64) * 0.04).astype(np.float32)
    g6, g9 = handle(6, filters), handle(9, filters)
    try:
        g6.set_filters(f2)
        g9.set_filters(f2)
        s = rng.uniform(-80, 0, (2, 121, 228)).astype(np.float32)
        s[0, :, 100:] = s[0, :, 100:101]
        both(torch_cuda, (g6, g9), oracle, f2, s)
        u = -40 * 98304 + rng.integers(0, 128, (3, 121, 130))
        many = np.tile((u / 98304.0).astype(np.float32), (100, 1, 1))
        got = from_db(torch_cuda, g6, many)
        assert np.array_equal(got, from_db(torch_cuda, g9, many))
        for i in range(3):
            want = oracle.hashprints_from_db(f2, many[i])
            assert np.array_equal(got[i], want) and np.array_equal(got[297 + i], want)
        assert g6.debug_q_products()[0] == 300 - 256                          # the last launch: the second pass
    finally:
        g6.close()
        g9.close()


@pytest.mark.parametrize("sec", (2.0, 5.0))
def test_end_to_end(torch_cuda, pair, oracle, filters, sec):
    clip = synth.gen_clip(70, sec)[None]
    want = oracle.Plan(clip.shape[1]).extract(filters, clip[0])
    for g in pair:
        assert np.array_equal(g.extract(clip)[0], want)


def test_transposed_entry_point_is_unchanged(torch_cuda, pair, oracle, filters):
    torch = torch_cuda
    rng = np.random.default_rng(6)
    s = rng.uniform(-80, 0, (2, 121, 228)).astype(np.float32)
    s[1, :, 50:200] = -80.0
    shifts = np.array([0, 3, -2], np.int32)
    out = []
    for g in pair:
        d_s = torch.from_numpy(s).cuda()
        hp = torch.zeros((2, 3, 129), dtype=torch.int64, device="cuda")
        g.hashprints_from_db_transposed_dev(d_s.data_ptr(), 2, 228, shifts, hp.data_ptr())
        torch.cuda.synchronize()
        out.append(hp.cpu().numpy().view(np.uint64))
    assert np.array_equal(out[0], out[1])
    for i in range(2):
        assert np.array_equal(out[0][i, 0], oracle.hashprints_from_db(filters, s[i]))
