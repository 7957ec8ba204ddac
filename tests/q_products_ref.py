"""The six-product split of the fixed-point projection restated in numpy, for
test_q_products_host.py and test_gpu_q_products.py.

fq = a0 + 2^8 a1 + 2^16 a2 and Du = b0 + 2^8 b1 + 2^16 b2 in balanced digits (-128 .. 127); the digit products of equal
weight 2^(8c), c = i + j, share one sum A_c, and D = sum_c 2^(8c) A_c = 2^16 Dp + Dl with Dp = A_2 + 2^8 A_3 + 2^16 A_4 and
Dl = A_0 + 2^8 A_1.  Every digit sum stays below 3 * 2420 * 128 * 128 < 2^27, so float64 matrix products are exact."""
import numpy as np

CTX, LAG, BINS, NFILT = 20, 80, 121, 64
CAP = 128       # entries of a tile's segment (k_project_q.hip kQCap)
TILE = 128      # hashprints per tile


def digits(x):
    """the three balanced base-256 digits of int64 x (|x| < 2^23)"""
    x = np.asarray(x, np.int64)
    d0 = ((x + 128) & 255) - 128
    x1 = (x - d0) >> 8
    d1 = ((x1 + 128) & 255) - 128
    d2 = (x1 - d1) >> 8
    assert (np.abs(d2) <= 128).all()
    return d0, d1, d2


def frames(du):
    """Du [121][c - 80] -> X [2420][c - 99], X[20 b + t][i] = Du[b][i + t]"""
    n = du.shape[1] - (CTX - 1)
    w = np.lib.stride_tricks.sliding_window_view(du, CTX, axis=1)[:, :n, :]      # [b][i][t]
    return np.ascontiguousarray(w.transpose(0, 2, 1)).reshape(BINS * CTX, n)


def class_sums(fq, du):
    """A_0 .. A_4 as int64 [64][n]: one float64 matrix product per class, the pairs (i, j) of a class side by side"""
    a = digits(fq)
    b = digits(frames(du))
    out = []
    for c in range(5):
        pairs = [(i, c - i) for i in range(3) if 0 <= c - i < 3]
        left = np.concatenate([a[i] for i, _ in pairs], axis=1).astype(np.float64)
        right = np.concatenate([b[j] for _, j in pairs], axis=0).astype(np.float64)
        out.append(np.rint(left @ right).astype(np.int64))
    return out


def lmax(fq):
    """Lmax_r = 128 (S0_r + 256 (S0_r + S1_r)): |Dl| at most, the digits of Du taken as 128"""
    a0, a1, _ = digits(fq)
    s0, s1 = np.abs(a0).sum(axis=1), np.abs(a1).sum(axis=1)
    return 128 * (s0 + 256 * (s0 + s1))


def split(oracle, filt, db):
    """(D by classes, Dp, Dl, Lmax [64], open [64][n]) of one dB spectrogram [121][c]"""
    fq = oracle.quantise_filters(filt).astype(np.int64)
    u = oracle.quantise_db(db).astype(np.int64)
    du = u[:, :-LAG] - u[:, LAG:]
    acc = class_sums(fq, du)
    d = sum(acc[c] << (8 * c) for c in range(5))
    dp = acc[2] + (acc[3] << 8) + (acc[4] << 16)
    dl = acc[0] + (acc[1] << 8)
    lm = lmax(fq)
    is_open = (lm[:, None] > 0) & ((np.abs(dp) << 16) <= lm[:, None])
    return d, dp, dl, lm, is_open, du


def tile_states(is_open, du):
    """(listed values, redone tiles) of one clip as the six-product kernel reports them: a tile whose slab of Du is zero
    lists nothing, a tile with more than CAP open values is redone"""
    n = is_open.shape[1]
    listed = redone = 0
    for n0 in range(0, n, TILE):
        if not du[:, n0:n0 + TILE + CTX - 1].any():
            continue
        k = int(is_open[:, n0:n0 + TILE].sum())
        if k > CAP:
            redone += 1
        else:
            listed += k
    return listed, redone
