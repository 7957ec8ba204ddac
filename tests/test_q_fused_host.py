"""The pairing of 16-byte units by which the fused six-product kernel settles an open value (k_project_q.hip,
q_value_from_digits), restated in numpy: the filter image as pack_filters_q lays it out, the slab of Du
digits as the staging lays it out, and over the 160 unit pairs the nine weighted dot products, which must be
q_products_ref.split's exact D."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q_products_ref as ref  # noqa: E402

STEPS, PITCH, CHUNKS = 2 * ref.CTX, 160, 8        # kQSteps, kQPitch, kQChunks
COLS = ref.TILE + ref.CTX - 1                     # 147 columns of a slab


def filter_image(fq):
    """[wave][step s = 2 t + p][digit][lane][16]: byte e of lane l = digit of fq[16 wave + (l & 15)][20 bin + t],
    bin = 64 p + 16 (l >> 4) + e, zero for bin >= 121"""
    dig = ref.digits(fq)
    img = np.zeros((4, STEPS, 3, 64, 16), np.int64)
    for w in range(4):
        for t in range(ref.CTX):
            for p in range(2):
                for l in range(64):
                    for e in range(16):
                        b = 64 * p + 16 * (l >> 4) + e
                        if b < ref.BINS:
                            for i in range(3):
                                img[w, 2 * t + p, i, l, e] = dig[i][16 * w + (l & 15), 20 * b + t]
    return img


def slab(du, n0):
    """[chunk][column (pitch 160)][digit][16]: byte e = digit of Du[16 chunk + e][n0 + column], zero for bins >= 121,
    for columns past the clip's Du and for the pitch's padding"""
    dig = ref.digits(du)
    s = np.zeros((CHUNKS, PITCH, 3, 16), np.int64)
    cols = min(COLS, du.shape[1] - n0)
    for q in range(CHUNKS):
        nb = min(16, ref.BINS - 16 * q)
        for j in range(3):
            s[q, :cols, j, :nb] = dig[j][16 * q:16 * q + nb, n0:n0 + cols].T
    return s


def value_from_digits(img, s, r, nl):
    """D of filter r and hashprint nl of the tile: 40 steps x 4 groups of unit pairs, nine digit products each"""
    acc = [0] * 5
    for step in range(STEPS):
        t, p = step >> 1, step & 1
        for g in range(4):
            assert nl + t <= 146
            for i in range(3):
                fu = img[r >> 4, step, i, (r & 15) + 16 * g]
                for j in range(3):
                    acc[i + j] += int(fu @ s[4 * p + g, nl + t, j])
    assert all(abs(a) < 2 ** 27 for a in acc)
    return sum(a << (8 * c) for c, a in enumerate(acc))


@pytest.mark.parametrize("c", (228, 355))
def test_unit_pairs_give_the_exact_sum(oracle, filters, c):
    rng = np.random.default_rng(c)
    db = rng.uniform(-80, 0, (121, c)).astype(np.float32)
    fq = oracle.quantise_filters(filters).astype(np.int64)
    d, _, _, _, _, du = ref.split(oracle, filters, db)
    img = filter_image(fq)
    nhp = c - 99
    for n0 in range(0, nhp, ref.TILE):
        s = slab(du, n0)
        last = min(ref.TILE, nhp - n0) - 1        # 127 in a full tile
        for r, nl in ((0, 0), (15, last), (16, last), (63, last), (63, 0), (37, last // 2)):
            assert value_from_digits(img, s, r, nl) == int(d[r, n0 + nl]), (n0, r, nl)


def test_padding_bytes_are_zero(oracle, filters):
    fq = oracle.quantise_filters(filters).astype(np.int64)
    img = filter_image(fq)
    assert not img[:, 1::2, :, 48:, 9:].any()      # bins 121 .. 127: p = 1, lanes 48 .. 63, bytes 9 .. 15
    assert np.abs(img).max() <= 128
