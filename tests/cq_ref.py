"""Plain restatements of the constant-Q stage (numpy and float64 only; nothing of the library or the oracle is used): the
band geometry, |c_j[3c]| from given forward bins, the planner's chirp-z classes with their split into global-memory
passes and LDS blocks, seeded forward bins, and the clip lengths at which the class sweep runs.

One class is all bands that share a chirp-z length p (plan.cpp chirpz_length: the smallest of 2^a, 3 2^a that holds
lg_j + C - 1 points).  Classes up to 16384 points run in LDS (k_cq.hip); larger ones peel `outer` radix-4 passes through
global memory around LDS blocks of len0 points (k_cq_big.hip)."""
import numpy as np

SR = 44100.0
FMIN, FMAX = 130.81, 4186.01
BPO = 24
MIN_WINDOW = 96
BINS = 121
P_MAX = 1 << 19             # the longest chirp-z transform the planner admits
LDS_MAX = 16384             # classes up to here run in LDS
BLOCK_MAX = 8192            # above: radix-4 passes are peeled until a block is at most this long

CONV_HANN_PERIODIC, CONV_LG_HALF_EVEN, CONV_FLOAT_GEOMETRY, CONV_NO_IFFT_SCALE = 1, 2, 4, 8

# shortest clip with a hashprint; 5 s (the only one of these with a 768-point class); 10 s; 45 s; 240 s; 900 s; the longest
# clip the forward split admits (8064 x 6720): together every class 256 .. 2^19, outer = 1, 2, 3, every len0, and
# len0 = 8192 at every outer (tests/test_cq_host.py)
LENGTHS = (54254, 220500, 441000, 1984500, 10584000, 39690000, 54190080)


def geometry(n, conventions=0):
    """(posit [121], lg [121]) of a clip of n samples: centre bin and window length of every band"""
    j = np.arange(BINS)
    if conventions & CONV_FLOAT_GEOMETRY:
        f32 = np.float32
        fftres = f32(SR) / f32(n)
        q = f32(2.0) ** (f32(1.0) / f32(BPO)) - f32(2.0) ** (f32(-1.0) / f32(BPO))
        f = f32(FMIN) * f32(2.0) ** (j.astype(np.float32) / f32(BPO))
        posit = np.floor(f / fftres).astype(np.int64)
        bw = (q * f / fftres).astype(np.float64)
    else:
        fftres = SR / n
        f = FMIN * 2.0 ** (j / BPO)
        posit = np.floor(f / fftres).astype(np.int64)
        bw = (2.0 ** (1.0 / BPO) - 2.0 ** (-1.0 / BPO)) * f / fftres
    rounded = np.rint(bw) if conventions & CONV_LG_HALF_EVEN else np.floor(bw + 0.5)
    return posit, np.maximum(rounded.astype(np.int64), MIN_WINDOW)


def extent(n, conventions=0):
    """(kmin, kmax, M, C): the bins [kmin, kmax) the bands read, the longest window and the spectrogram's columns"""
    posit, lg = geometry(n, conventions)
    start = posit - lg // 2
    m = int(lg.max())
    return int(start.min()), int((start + lg).max()), m, (m + 2) // 3


def cq_from_bins(x, kmin, n, bands=None):
    """|c_j[3c]| in float64, [len(bands)][C], from forward bins x [kmax - kmin] (complex) that start at bin kmin: per band
    the Hann-windowed slice, centre at index 0 of a length-M buffer, one length-M inverse transform, every third sample.
    bands: the rows wanted (default all 121)."""
    x = np.asarray(x)
    posit, lg = geometry(n)
    m = int(lg.max())
    cols = (m + 2) // 3
    bands = range(BINS) if bands is None else list(bands)
    out = np.zeros((len(bands), cols))
    for row, j in enumerate(bands):
        L = int(lg[j])
        win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(L) / (L - 1))
        idx = posit[j] - L // 2 + np.arange(L)
        assert idx[0] >= kmin and idx[-1] < kmin + x.shape[0], (j, int(idx[0]), int(idx[-1]), kmin, x.shape[0])
        prod = x[idx - kmin].astype(np.complex128) * win
        buf = np.zeros(m, np.complex128)
        half = L // 2
        buf[: L - half] = prod[half:]
        buf[m - half:] = prod[:half]
        out[row] = np.abs(np.fft.ifft(buf)[::3])[:cols]
    return out


def chirpz_length(need):
    """the smallest of 2^a, 3 2^a, at least 64, that is >= need"""
    p2, p3 = 64, 96
    while p2 < need:
        p2 *= 2
    while p3 < need:
        p3 *= 2
    return min(p2, p3)


def peel(p):
    """(outer, len0): radix-4 passes through global memory and the LDS block they leave"""
    outer, length = 0, p
    while p > LDS_MAX and length > BLOCK_MAX:
        length //= 4
        outer += 1
    return outer, length


def classes(n, conventions=0):
    """{p: (outer, len0, [bands])} of a clip of n samples, ascending in p"""
    _, lg = geometry(n, conventions)
    c = (int(lg.max()) + 2) // 3
    out = {}
    for j in range(BINS):
        p = chirpz_length(int(lg[j]) + c - 1)
        if p not in out:
            out[p] = peel(p) + ([],)
        out[p][2].append(j)
    return dict(sorted(out.items()))


def admitted():
    """every chirp-z length the planner admits from 256 on: 2^a and 3 2^a up to 2^19"""
    out = set()
    a = 256
    while a <= P_MAX:
        out.add(a)
        if 3 * a // 2 <= P_MAX:
            out.add(3 * a // 2)
        a *= 2
    return out


def bins(n, nk, seed):
    """float32 [nk][2]: standard-normal forward bins, seeded, with one spike of 3.0e4 at the first (+, Re) and the last
    (-, Im) element of the widest band's slice"""
    x = np.random.default_rng(seed).standard_normal((nk, 2)).astype(np.float32)
    posit, lg = geometry(n)
    start = posit - lg // 2
    j = int(lg.argmax())
    kmin = int(start.min())
    assert nk == int((start + lg).max()) - kmin
    x[start[j] - kmin, 0] = 3.0e4
    x[start[j] + lg[j] - 1 - kmin, 1] = -3.0e4
    return x


def first_and_last_bands(n):
    """the first and the last band of every class of a clip of n samples, ascending"""
    return sorted({b for _, _, bands in classes(n).values() for b in (bands[0], bands[-1])})
