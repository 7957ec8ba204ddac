"""The hashprint kernel's slab staging by chains (k_project_q.hip) restated in numpy.

Du[col] = u[col] - u[col + 80], so a tile's 147 slab columns need u of the 227 columns n0 .. n0 + 226, which fall into 80
chains r, r + 80, r + 160 (the third only for r < 67).  A task = (half chunk qh: bins 8 qh .. 8 qh + 7, residue r) loads
and quantises its chain once, forms Du[r] and Du[r + 80] and stores two half units of three 8-byte digit planes, gathered
by byte permutes; 1280 tasks, five per thread.  Checked for every tile of clips of several widths:
  every byte of the slab's 147 columns is written exactly once, the spare columns 147 .. 159 only with zeros;
  every needed (bin, column) is loaded exactly once (loads outside the valid part go to index 0 and are not used);
  every load index lies inside the clip;
  the slab equals the digits of q_products_ref.
And the order of the workgroups: every logical tile once, the short last tiles behind all full ones."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q_products_ref as ref  # noqa: E402

THREADS, TASKS, HALVES, PITCH, UNIT, COLS = 256, 5, 16, 160, 48, ref.TILE + ref.CTX - 1
HEAVY = COLS - ref.LAG          # 67 residues whose chain holds two slab columns
WIDTHS = (100, 179, 180, 227, 228, 307, 2419)


def perm(s0, s1, sel):
    """v_perm_b32: byte i of the result is byte sel_i of the eight bytes {s1: 0..3, s0: 4..7}; selector 0x0c gives 0"""
    src = np.concatenate([s1.view(np.uint8).reshape(-1, 4), s0.view(np.uint8).reshape(-1, 4)], axis=1)
    out = np.zeros((src.shape[0], 4), np.uint8)
    for i in range(4):
        k = (sel >> (8 * i)) & 255
        assert k < 8 or k == 0x0c
        if k < 8:
            out[:, i] = src[:, k]
    return out.reshape(-1).view(np.uint32)


def planes(w):
    """w [n][4] words with digit j in byte j -> [n][3] plane words, element e's digit in byte e (q_planes)"""
    w = [np.ascontiguousarray(w[:, e]) for e in range(4)]
    t01, t23 = perm(w[1], w[0], 0x05010400), perm(w[3], w[2], 0x05010400)
    u01, u23 = perm(w[1], w[0], 0x0c0c0602), perm(w[3], w[2], 0x0c0c0602)
    return np.stack([perm(t23, t01, 0x05040100), perm(t23, t01, 0x07060302), perm(u23, u01, 0x05040100)], axis=1)


def digit_bytes(d):
    return ((d.astype(np.int64) + 0x808080) ^ 0x808080).astype(np.uint32) & np.uint32(0xFFFFFFFF)


def stage_tile(u, c, n0):
    """(slab bytes [8][160][48], writes per byte, loads per (bin, column) of the clip) of the tile at n0; u [121][c] int"""
    task = np.arange(THREADS * TASKS)                       # thread tid's tasks: tid + 256 i
    qh, r = task // ref.LAG, task % ref.LAG
    assert qh.max() == HALVES - 1 and len(set(zip(qh, r))) == HALVES * ref.LAG
    gc = n0 + r
    in0 = gc + ref.LAG < c
    in1 = (r < HEAVY) & (gc + 2 * ref.LAG < c)
    flat = u.reshape(-1).astype(np.int64)
    loads = np.zeros(ref.BINS * c, np.int64)
    wa = np.zeros((task.size, 8), np.uint32)
    wb = np.zeros((task.size, 8), np.uint32)
    for e in range(8):
        b = 8 * qh + e
        okb = b < ref.BINS
        at = b * c + gc
        i0 = np.where(in0 & okb, at, 0)
        i2 = np.where(in1 & okb, at + 2 * ref.LAG, 0)
        assert i0.min() >= 0 and (i0 + ref.LAG).max() < ref.BINS * c and i2.min() >= 0 and i2.max() < ref.BINS * c
        np.add.at(loads, i0[in0 & okb], 1)
        np.add.at(loads, i0[in0 & okb] + ref.LAG, 1)
        np.add.at(loads, i2[in1 & okb], 1)
        u0, u1, u2 = flat[i0], flat[i0 + ref.LAG], flat[i2]
        wa[:, e] = digit_bytes(np.where(in0 & okb, u0 - u1, 0))
        wb[:, e] = digit_bytes(np.where(in1 & okb, u1 - u2, 0))
    slab = np.zeros((8, PITCH, UNIT), np.uint8)
    writes = np.zeros((8, PITCH, UNIT), np.int64)
    for w, col in ((wa, r), (wb, r + ref.LAG)):
        lo, hi = planes(w[:, :4]), planes(w[:, 4:])
        for j in range(3):
            both = np.stack([lo[:, j], hi[:, j]], axis=1).copy().view(np.uint8).reshape(-1, 8)
            for k in range(8):
                at = (qh >> 1, col, 16 * j + 8 * (qh & 1) + k)
                slab[at] = both[:, k]
                np.add.at(writes, at, 1)
    return slab, writes, loads.reshape(ref.BINS, c)


def expected_slab(u, c, n0):
    du = np.zeros((128, COLS), np.int64)
    n = max(0, min(COLS, c - ref.LAG - n0))
    du[:ref.BINS, :n] = u[:, n0:n0 + n] - u[:, n0 + ref.LAG:n0 + ref.LAG + n]
    want = np.zeros((8, PITCH, UNIT), np.uint8)
    for j, d in enumerate(ref.digits(du)):
        want[:, :COLS, 16 * j:16 * j + 16] = d.astype(np.int8).view(np.uint8).reshape(8, 16, COLS).transpose(0, 2, 1)
    return want


@pytest.mark.parametrize("c", WIDTHS)
def test_chains_write_the_slab_once_from_single_loads(oracle, c):
    rng = np.random.default_rng(c)
    s = rng.uniform(-80, 0, (ref.BINS, c)).astype(np.float32)
    s[:, rng.integers(0, c, 5)] = -80.0
    u = oracle.quantise_db(s).astype(np.int64)
    nhp = c - 99
    for n0 in range(0, nhp, ref.TILE):
        slab, writes, loads = stage_tile(u, c, n0)
        assert (writes[:, :COLS] == 1).all(), n0
        assert (writes[:, COLS:] <= 1).all() and not slab[:, COLS:].any(), n0
        assert loads.max() == 1, n0
        need = np.zeros((ref.BINS, c), bool)                                    # the columns whose Du the slab holds, and their partners
        n = max(0, min(COLS, c - ref.LAG - n0))
        need[:, n0:n0 + n] = True
        need[:, n0 + ref.LAG:n0 + ref.LAG + n] = True
        assert np.array_equal(loads == 1, need), n0
        assert np.array_equal(slab, expected_slab(u, c, n0)), n0


def tile_of_workgroup(b, grid, nhp, tiles_x, n_clips):
    """q_tile_of_workgroup: the logical tile clip * tiles_x + tile of workgroup b, None for the grid's padding"""
    def round8(n):
        return 8 * ((n + 7) // 8)
    if nhp - (tiles_x - 1) * ref.TILE > ref.TILE - 16:                           # the last tile is no short one
        t = (b & 7) * (grid // 8) + (b >> 3)
        return t if t < tiles_x * n_clips else None
    full_x = tiles_x - 1
    n_full, grid_full = full_x * n_clips, round8(full_x * n_clips)
    if b < grid_full:
        j = (b & 7) * (grid_full // 8) + (b >> 3)
        return None if j >= n_full else (j // full_x) * tiles_x + j % full_x
    b -= grid_full
    j = (b & 7) * ((grid - grid_full) // 8) + (b >> 3)
    return j * tiles_x + full_x if j < n_clips else None


@pytest.mark.parametrize("nhp,n_clips", [(1, 1), (16, 3), (112, 9), (113, 9), (128, 5), (129, 1), (144, 7), (240, 4), (2320, 2), (2320, 37)])
def test_short_tiles_come_last_and_every_tile_once(nhp, n_clips):
    tiles_x = (nhp + ref.TILE - 1) // ref.TILE
    short = nhp - (tiles_x - 1) * ref.TILE <= ref.TILE - 16
    r8 = lambda n: 8 * ((n + 7) // 8)  # noqa: E731
    grid = r8((tiles_x - 1) * n_clips) + r8(n_clips) if short else r8(tiles_x * n_clips)
    ts = [tile_of_workgroup(b, grid, nhp, tiles_x, n_clips) for b in range(grid)]
    real = [t for t in ts if t is not None]
    assert sorted(real) == list(range(tiles_x * n_clips))
    is_last = [t % tiles_x == tiles_x - 1 for t in real]
    if short:
        assert is_last == sorted(is_last)                                        # all full tiles, then the short ones
    for x in range(8):                                                           # an XCD's full tiles: a contiguous run
        run = [t for b, t in enumerate(ts) if t is not None and b % 8 == x and not (short and t % tiles_x == tiles_x - 1)]
        if short:
            run = [t - t // tiles_x for t in run]                                # (numbered without the short tiles)
        assert run == list(range(run[0], run[0] + len(run))) if run else True
