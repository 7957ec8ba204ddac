"""Plain restatements of the chirp-z forward transform's shape (numpy and float64 only, nothing of the library
or the oracle is used): which convolution length a clip length takes, which rows of the last stage hold consumed bins, which
instance of the last stage's kernel runs them -- and the clip lengths at which the sweep of those classes runs, with its clips.

A clip of n samples whose length has a prime factor above 7 is transformed by a cyclic convolution of length L = n1 * 6300 >=
n + (kmax - kmin) - 1 with n1 = 16 a, the smallest that fits.  The kernels' shapes follow from a and from the rows k1 of 6300
bins that the constant-Q bands read:
  first stage   length-a transforms in tiles of 16 outputs, operands fetched four steps ahead (a % 4, a % 16, a <= 16 or above)
  last stage    the consumed rows k1lo .. k1lo + k1n - 1 in `need` row tiles of 32 (16 complex rows each), nt2 <= 3 per wave,
                n_tiles2 / nt2 groups of them (the last with n_tiles2 - need tiles of zeros); the n1 residues in n_blocks
                register sets of `step` in {16, 15, 14}, two sets in turn (an odd n_blocks walks one set past n1)
  tables        slack = L - (n + (kmax - kmin) - 1): at 0 the two halves of the lag table touch"""
import collections
import functools

import numpy as np

import cq_ref

N2 = 6300                   # the row transform of every chirp-z length
SHORTEST = 54254            # the shortest clip with a hashprint (C = 100 spectrogram columns)
A_FIRSTS = tuple(range(1, 18)) + (32, 33)       # every a up to one past a full tile of 16, and the next tile edge
A_EXACT = (1, 4, 16)        # exact fits (slack 0): the smallest a, a multiple of the prefetch depth, a full tile
A_CLASSES = 59              # last-stage classes are swept for every a up to here (clips of up to two minutes)
K1N_EDGES = (16, 17, 32, 33, 48, 49)            # consumed rows that fill a row tile exactly, or leave one row in the next

Shape = collections.namedtuple("Shape", "a n1 L slack k1lo k1n need nt2 n_tiles2 step n_blocks")


def is_smooth(n):
    """whether n has no prime factor above 7 (such a length takes the mixed-radix transform unless forced)"""
    for p in (2, 3, 5, 7):
        while n % p == 0:
            n //= p
    return n == 1


def needed(n):
    """n + (kmax - kmin) - 1: the shortest convolution that keeps the consumed bins free of wrap-around.  Non-decreasing
    in n: a band's centre bin moves up by at most one per sample, its window never shrinks, so kmin rises by at most one
    and kmax never falls."""
    kmin, kmax, _, _ = cq_ref.extent(n)
    return n + (kmax - kmin) - 1


def a_of(n):
    return -(-needed(n) // (16 * N2))


def last_stage(n1, k1n):
    """(need, nt2, n_tiles2, step, n_blocks) of the last stage for n1 residues and k1n consumed rows"""
    need = (2 * k1n + 31) // 32
    nt2 = min(need, 3)
    n_tiles2 = -(-need // nt2) * nt2

    def padded(step):                                   # residues an even number of register sets walks
        return (-(-n1 // step) + 1) // 2 * 2 * step
    step = min((16, 15, 14), key=lambda s: (padded(s), -s))
    return need, nt2, n_tiles2, step, -(-n1 // step)


def shape(n):
    """the Shape of a clip of n samples that takes (or is forced into) the chirp-z forward transform"""
    kmin, kmax, _, _ = cq_ref.extent(n)
    need_l = n + (kmax - kmin) - 1
    a = -(-need_l // (16 * N2))
    n1 = 16 * a
    k1lo = kmin // N2
    k1n = (kmax - 1) // N2 - k1lo + 1
    return Shape(a, n1, n1 * N2, n1 * N2 - need_l, k1lo, k1n, *last_stage(n1, k1n))


def last_stage_class(s):
    """what selects the last stage's code path: (step, n_blocks odd, nt2, tile groups, tiles of zeros in the last group)"""
    return s.step, s.n_blocks & 1, s.nt2, s.n_tiles2 // s.nt2, s.n_tiles2 - s.need


@functools.lru_cache(maxsize=None)
def _first_n(a):
    """the smallest n >= SHORTEST with a_of(n) >= a (bisection: a_of is non-decreasing)"""
    lo, hi = SHORTEST, 16 * N2 * a              # needed(n) > n: a_of(hi) > a
    if a_of(lo) >= a:
        return lo
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if a_of(mid) >= a else (mid, hi)
    return hi


def first_length(a):
    """the smallest odd n with a prime factor above 7 whose convolution has n1 = 16 a (odd: the second clip of a batch then
    starts on a 2-byte boundary)"""
    n = _first_n(a)
    while n % 2 == 0 or is_smooth(n):
        n += 1
    assert a_of(n) == a
    return n


def last_length(a):
    """the largest n with a prime factor above 7 whose convolution has n1 = 16 a"""
    n = _first_n(a + 1) - 1
    while is_smooth(n):
        n -= 1
    assert a_of(n) == a
    return n


def extents(ns):
    """(kmin, kmax) of cq_ref.extent for an array of lengths at once (the same float64 operations, element by element)"""
    ns = np.asarray(ns, np.int64)
    f = cq_ref.FMIN * 2.0 ** (np.arange(cq_ref.BINS) / cq_ref.BPO)
    fftres = cq_ref.SR / ns[:, None]
    posit = np.floor(f / fftres).astype(np.int64)
    bw = (2.0 ** (1.0 / cq_ref.BPO) - 2.0 ** (-1.0 / cq_ref.BPO)) * f / fftres
    lg = np.maximum(np.floor(bw + 0.5).astype(np.int64), cq_ref.MIN_WINDOW)
    start = posit - lg // 2
    return start.min(axis=1), (start + lg).max(axis=1)


def _smooth_mask(ns):
    r = np.array(ns, np.int64)
    for p in (2, 3, 5, 7):
        while True:
            m = r % p == 0
            if not m.any():
                break
            r[m] //= p
    return r == 1


@functools.lru_cache(maxsize=None)
def class_firsts():
    """({last_stage_class: n}, {k1n: n}): the smallest odd n with a prime factor above 7, a <= A_CLASSES, of every class of
    the last stage that occurs there, and of every number of consumed rows"""
    by_class, by_k1n = {}, {}
    for a in range(1, A_CLASSES + 1):
        lo, hi = _first_n(a), _first_n(a + 1)
        ns = np.arange(lo | 1, hi, 2)
        ns = ns[~_smooth_mask(ns)]
        kmin, kmax = extents(ns)
        k1n = (kmax - 1) // N2 - kmin // N2 + 1
        for k in np.unique(k1n):
            n = int(ns[np.argmax(k1n == k)])
            by_k1n.setdefault(int(k), n)
            by_class.setdefault(last_stage_class(shape(n)), n)      # (the class changes with ceil(k1n / 16) only)
    return by_class, by_k1n


@functools.lru_cache(maxsize=None)
def sweep_lengths():
    """the lengths of the sweep: the first length of every a in A_FIRSTS, the exact fits (the last length of a in A_EXACT),
    the first length of every last-stage class up to a = A_CLASSES, the first length of every k1n in K1N_EDGES; a length is
    listed once, where it first appears"""
    by_class, by_k1n = class_firsts()
    out = [first_length(a) for a in A_FIRSTS] + [last_length(a) for a in A_EXACT]
    for n in sorted(by_class.values()) + [by_k1n[k] for k in K1N_EDGES]:
        if n not in out:
            out.append(n)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def forced_smooth_length():
    """(n, slack): the 7-smooth length with a <= 17 whose forced chirp-z convolution has the least slack (the smallest n on a tie)"""
    best = None
    for n in smooth_lengths(SHORTEST, _first_n(18) - 1):
        key = (shape(n).slack, n)
        if best is None or key < best:
            best = key
    return best[1], best[0]


def smooth_lengths(lo, hi):
    """every 7-smooth n in [lo, hi], ascending"""
    out = []
    p7 = 1
    while p7 <= hi:
        p5 = p7
        while p5 <= hi:
            p3 = p5
            while p3 <= hi:
                p2 = p3
                while p2 <= hi:
                    if p2 >= lo:
                        out.append(p2)
                    p2 *= 2
                p3 *= 3
            p5 *= 5
        p7 *= 7
    return sorted(out)


def noise_clip(n):
    """full-scale noise, seeded with n: uniform over all of int16"""
    return np.random.default_rng(n).integers(-32768, 32768, n).astype(np.int16)


def rail_clip(n):
    """seeded with n: every sample at one end of the int16 range, -32768 or 32767"""
    return np.where(np.random.default_rng(n + 1).integers(0, 2, n) == 1, 32767, -32768).astype(np.int16)


def float64_error(x, clip, kmin, kmax):
    """largest error of forward bins x [kmax - kmin][2] against the float64 transform of clip / 32768, over max |ref|"""
    ref = np.fft.rfft(np.asarray(clip, np.float64) / 32768.0)[kmin:kmax]
    x = np.asarray(x, np.float64)
    return float(np.abs(x[:, 0] + 1j * x[:, 1] - ref).max() / np.abs(ref).max())
