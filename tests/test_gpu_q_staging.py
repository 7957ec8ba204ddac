"""The hashprint kernel's slab staging by chains and its workgroup order (k_project_q.hip): the default
handle against q_products_ref and the oracle, from seeded dB spectrograms through hashprints_from_db (the six-product
kernel) and stage_delta_q (the nine-product kernel, D as int64).  Everything is integers: compared for equality."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q_products_ref as ref  # noqa: E402
import transpose_ref  # noqa: E402
import hpfw_amd  # noqa: E402
from hpfw_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(torch_cuda, filters):
    """a handle of its own with the default settings"""
    g = hpfw_amd.Gpu(0)
    g.set_filters(filters)
    yield g
    g.close()


def run(torch, g, s):
    """(hashprints uint64 [n][c - 99] of the six-product kernel, those of the nine-product kernel, D int64 [n][64][c - 99])"""
    n, _, c = s.shape
    d_s = torch.from_numpy(np.ascontiguousarray(s)).cuda()
    hp6 = torch.zeros((n, c - 99), dtype=torch.int64, device="cuda")
    hp9 = torch.zeros_like(hp6)
    d = torch.zeros((n, 64, c - 99), dtype=torch.int64, device="cuda")
    g.hashprints_from_db_dev(d_s.data_ptr(), n, c, hp6.data_ptr())
    g.stage_delta_q_dev(d_s.data_ptr(), n, c, d.data_ptr(), hp9.data_ptr())
    torch.cuda.synchronize()
    return hp6.cpu().numpy().view(np.uint64), hp9.cpu().numpy().view(np.uint64), d.cpu().numpy()


def check(torch, g, oracle, filt, s):
    """the handle equals the reference; returns the reference's (listed, redone)"""
    new = run(torch, g, s)
    listed = redone = 0
    for i in range(s.shape[0]):
        d, _, _, _, is_open, du = ref.split(oracle, filt, s[i])
        assert np.array_equal(new[2][i], d), i
        want = oracle.hashprints_from_db(filt, s[i])
        assert np.array_equal(new[0][i], want) and np.array_equal(new[1][i], want), i
        a, b = ref.tile_states(is_open, du)
        listed, redone = listed + a, redone + b
    tiles = s.shape[0] * ((s.shape[2] - 99 + ref.TILE - 1) // ref.TILE)
    d_s = torch.from_numpy(np.ascontiguousarray(s)).cuda()                          # (the handle's last six-product launch)
    hp = torch.zeros((s.shape[0], s.shape[2] - 99), dtype=torch.int64, device="cuda")
    g.hashprints_from_db_dev(d_s.data_ptr(), s.shape[0], s.shape[2], hp.data_ptr())
    assert g.debug_q_products() == (tiles, listed, redone)
    return listed, redone


@pytest.mark.parametrize("n_hp", (1, 15, 16, 17, 127, 128, 129, 144, 2320))
def test_widths(torch_cuda, g, oracle, filters, n_hp):
    """one tile, a short last tile (short tiles dispatched last), an exactly full last tile, the workload's shape"""
    c = n_hp + 99
    s = np.random.default_rng(1000 + n_hp).uniform(-80, 0, (2, 121, c)).astype(np.float32)
    check(torch_cuda, g, oracle, filters, s)


@pytest.mark.parametrize("floor", ("tile", "columns", "bin 120", "bin 0"))
def test_the_floor(torch_cuda, g, oracle, filters, floor):
    """c = 371: two full tiles and a short one of 16.  The -80 dB floor under a whole tile's slab (the all-zero shortcut),
    in the single columns c - 81, c - 80 and c - 1 (the last column with a partner, the first and the last without one),
    in the highest and in the lowest bin"""
    c = 371
    s = np.random.default_rng(7).uniform(-80, 0, (2, 121, c)).astype(np.float32)
    if floor == "tile":
        s[0, :, :ref.TILE + ref.CTX - 1 + ref.LAG] = -80.0
        s[1, :, 256:] = -80.0
    elif floor == "columns":
        s[0][:, [c - 81, c - 80, c - 1]] = -80.0
        s[1][:, c - 80] = -80.0
    else:
        s[:, 120 if floor == "bin 120" else 0, :] = -80.0
    new = run(torch_cuda, g, s)
    if floor == "tile":
        ones = np.uint64(2 ** 64 - 1)
        assert (new[0][0, :128] == ones).all() and (new[0][1, 256:] == ones).all()
    check(torch_cuda, g, oracle, filters, s)


def test_tiles_above_the_cap_are_redone_alike(torch_cuda, g, oracle, filters):
    """near-stationary input (every difference has one digit), c = 240: a full tile and a short one of 13, both above the
    cap -- the nine-product redo over the slab as the chains left it; then one such stretch in noise"""
    rng = np.random.default_rng(3)
    s = ((-40 * 98304 + rng.integers(0, 128, (2, 121, 240))) / 98304.0).astype(np.float32)
    assert check(torch_cuda, g, oracle, filters, s) == (0, 4)
    s = rng.uniform(-80, 0, (2, 121, 355)).astype(np.float32)
    s[0, :, 30:132] = ((-40 * 98304 + rng.integers(0, 128, (121, 102))) / 98304.0).astype(np.float32)
    assert check(torch_cuda, g, oracle, filters, s)[1] == 1


def test_transposed(torch_cuda, g, oracle, filters):
    """two shifted filter images over one slab (SHIFTED), a short last tile"""
    torch = torch_cuda
    c, shifts = 244, np.array([3, -2], np.int32)
    s = np.random.default_rng(6).uniform(-80, 0, (2, 121, c)).astype(np.float32)
    d_s = torch.from_numpy(s).cuda()
    hp = torch.zeros((2, 2, c - 99), dtype=torch.int64, device="cuda")
    g.hashprints_from_db_transposed_dev(d_s.data_ptr(), 2, c, shifts, hp.data_ptr())
    torch.cuda.synchronize()
    out = hp.cpu().numpy().view(np.uint64)
    for i in range(2):
        for j, sh in enumerate(shifts):
            assert np.array_equal(out[i, j], oracle.hashprints_from_db(filters, transpose_ref.shift_db(s[i], int(sh)))), (i, sh)


def test_end_to_end_from_pcm(torch_cuda, g, oracle, filters):
    """two 2 s clips through extract: the dB terms' instance (the reference level rides on the chains' loads)"""
    clips = np.stack([synth.gen_clip(81 + i, 2.0) for i in range(2)])
    plan = oracle.Plan(clips.shape[1])
    got = g.extract(clips)
    for i in range(2):
        assert np.array_equal(got[i], plan.extract(filters, clips[i])), i
