"""S6's column stage without a GPU, at every n1 <= 255 the planner reaches (tests/cols_ref.py): the split rule, the
oracle's forward bins against float64, the int32 pairing's headroom, and the library's own twiddle-digit images run
through a numpy restatement of the three matrix-core kernels' integer arithmetic (what tests/emu is to the LDS
transforms)."""
import numpy as np
import pytest

import cols_ref
import hpfw_amd

# first length per n1 (the order of n1), then even n1 with odd n2, then the LDS-staged kernel's chunk edges: frozen, so
# that a change of the planner's rule shows as a diff here and not as silently different coverage
SWEEP = (
    54432, 54675, 54880, 57624, 57344, 65625, 65536, 86400, 96040, 64827, 122880, 60025, 138240, 114688, 144060, 131072,
    84035, 184320, 240000, 201684, 218700, 245760, 117649, 280000, 276480, 229376, 360000, 354375, 262144, 336140, 368640,
    234375, 493920, 455625, 403368, 540000, 491520, 470596, 560000, 504210, 552960, 458752, 720000, 390625, 777924, 524288,
    759375, 672280, 737280, 352947, 937500, 1000000, 944784, 1037232, 420175, 1080000, 1063125, 983040, 941192, 1250000,
    1008420, 1105920, 917504, 1265625, 1481760, 1366875, 588245, 1562500, 1555848,
    61250, 71442, 236196, 600250, 1180980,
    1048576, 1620000, 1835008, 2812500)
N1_EVEN = (8, 10, 12, 14, 16, 18, 20, 24, 28, 30, 32, 36, 40, 42, 48, 50, 54, 56, 60, 64, 70, 72, 80, 84, 90, 96, 98, 100,
           108, 112, 120, 126, 128, 140, 144, 150, 160, 162, 168, 180, 192, 196, 200, 210, 216, 224)
N1_ODD = (9, 15, 21, 25, 27, 35, 45, 49, 63, 75, 81, 105, 125, 135, 147, 175, 189)
N1_STAGED = (225, 240, 243, 245, 250, 252)

# Forward bins against np.fft.rfft(clip / 32768) in float64, largest error over the clip's own max |ref|.  The oracle
# alone over the whole sweep, both clip kinds, measured 1.65e-7 at worst (234375 = 75 x 3125, the noise clip); the bar
# is twice that, rounded up to one digit -- and below the 2e-6 tests/test_oracle.py holds forward bins to.
FLOAT64_BAR = 4e-7


def test_sweep_is_the_frozen_list():
    first = cols_ref.first_lengths()
    assert tuple(first) == tuple(sorted(N1_EVEN + N1_ODD + N1_STAGED))
    assert cols_ref.sweep_lengths() == SWEEP
    for n1, n in first.items():
        assert cols_ref.split(n)[0] == n1 and n >= cols_ref.FIRST_LENGTH
    assert [cols_ref.split(n) for n in SWEEP[-9:]] == [(10, 6125), (14, 5103), (36, 6561), (98, 6125), (180, 6561),
                                                       (256, 4096), (270, 6000), (448, 4096), (450, 6250)]


@pytest.mark.parametrize("n", SWEEP)
def test_split_rule_and_oracle_against_float64(oracle, n):
    plan = oracle.Plan(n)
    assert (plan.n1, plan.n2) == cols_ref.split(n)
    t = hpfw_amd.plan_cols_tables(n)                           # the library's planner: the same split
    assert (t["n1"], t["n2"]) == cols_ref.split(n)
    for kind, clip in (("noise", cols_ref.noise_clip(n)), ("worst", cols_ref.worst_clip(n))):
        err = cols_ref.float64_error(plan.spectrum(clip), clip, plan.kmin, plan.kmax)
        print(f"n = {n} = {plan.n1} x {plan.n2}, {kind}: {err:.3g}")
        assert err < FLOAT64_BAR, (n, kind, err)


def test_paired_accumulators_stay_below_2_31():
    """acc_0 + 2^8 acc_1 and acc_2 + 2^8 acc_3 over ALL int16 columns, every row, Re and Im, at every reachable n1 <= 255:
    a condition, not a measurement.  Largest fraction of 2^31 reached: 0.451 at n1 = 210 (even <= 224; 0.43 at 224), 0.376 at
    175 (odd <= 224), 0.526 at 245 (225 .. 255) -- one bit to spare."""
    frac = {}
    for name, n1s in (("even <= 224", N1_EVEN), ("odd <= 224", N1_ODD), ("225 .. 255", N1_STAGED)):
        for n1 in n1s:
            v = np.abs(cols_ref.worst_case_table(n1)[1])
            assert v.max() < 2 ** 31, (n1, int(v.max()))
            frac[name] = max(frac.get(name, (0, 0)), (float(v.max()) / 2 ** 31, n1))
    for name, (f, n1) in frac.items():
        print(f"{name}: {f:.3f} of 2^31 at n1 = {n1}")
    # (the search itself: the pair of weight 2^16 reaches about n1 2^14 127 (1 + 2^8 / 2) / 2^31 ~ n1 / 500, so a search
    # that found nothing would show here)
    assert 0.40 < frac["even <= 224"][0] < 0.5 and 0.5 < frac["225 .. 255"][0] < 0.6


def test_mirrored_row_integers_stay_below_2_31():
    """the parity-split kernel forms E + O and E - O (Im: O - E) of the paired sums in int32, for the rows q1 <= n1 / 4 of
    every even n1 <= 224; per parity the paired sums themselves.  Largest fraction of 2^31: 0.451 at n1 = 210."""
    worst = (0.0, 0)
    for n1 in N1_EVEN:
        for q1 in range(n1 // 4 + 1):
            for part in range(2):
                for pair in range(2):
                    for sign in (1, -1):
                        col, v = cols_ref.worst_case_columns(n1, q1, part, pair, odd_sign=sign)
                        assert abs(v) < 2 ** 31, (n1, q1, part, pair, sign, v)
                        worst = max(worst, (abs(v) / 2 ** 31, n1))
                        # (E and O alone are sums over half of the same terms, each term at most its corner's value)
    print(f"E + O, E - O: {worst[0]:.3f} of 2^31 at n1 = {worst[1]}")
    assert 0.40 < worst[0] < 0.5


# ---- the library's tables, and the kernels' integer arithmetic on them -----------------------------------------------

def _image_rows(image):
    """[mt][ks][3][64 lanes][16] -> digits [3][32 mt rows][32 ks samples]: byte e of lane l is row 32 tile + (l & 31),
    k1 = 32 step + 16 (l >> 5) + e"""
    mt, ks = image.shape[:2]
    return image.reshape(mt, ks, 3, 2, 32, 16).transpose(2, 0, 4, 1, 3, 5).reshape(3, 32 * mt, 32 * ks).astype(np.int64)


def _image2_rows(image2, ks2):
    """[mt2][parity ks2 + s][3][64 lanes][16] -> digits [3][2 parities][16 mt2 rows][64 ks2 samples m]: byte e of lane l is
    row 16 tile + (l & 15), m = 64 s + 16 (l >> 4) + e, k1 = 2 m + parity"""
    mt2 = image2.shape[0]
    return (image2.reshape(mt2, 2, ks2, 3, 4, 16, 16).transpose(3, 1, 0, 5, 2, 4, 6)
            .reshape(3, 2, 16 * mt2, 64 * ks2).astype(np.int64))


def _int32(v):
    """the value as the kernel's int32 arithmetic holds it: asserted not to wrap"""
    assert np.abs(v).max() < 2 ** 31
    return v


def _paired(digits, lo, hi):
    """digits [3][rows][K] x sample digits [K][cols] -> (acc_0 + 2^8 acc_1, acc_2 + 2^8 acc_3): digit products of weight
    i + j (sample digit i, twiddle digit j) share an int32 accumulator, the pairs are formed in int32"""
    acc = [_int32(digits[0] @ lo), _int32(digits[1] @ lo + digits[0] @ hi), _int32(digits[2] @ lo + digits[1] @ hi),
           _int32(digits[2] @ hi)]
    return _int32(acc[0] + (acc[1] << 8)), _int32(acc[2] + (acc[3] << 8)), acc


def _columns(n1, n_noise=24):
    """int16 [n1][columns]: noise with the ends of the range, constant columns, and every worst-case column of n1"""
    rng = np.random.default_rng(n1)
    noise = rng.integers(-32768, 32768, (n1, n_noise)).astype(np.int16)
    noise[:, 0], noise[:, 1], noise[::2, 2], noise[1::2, 2] = 32767, -32768, 32767, -32768
    return np.concatenate([noise, cols_ref.worst_case_table(n1)[0].reshape(-1, n1).T], axis=1)


@pytest.mark.parametrize("n1", sorted(N1_EVEN + N1_ODD + N1_STAGED))
def test_library_column_tables_and_kernel_arithmetic(n1):
    t = hpfw_amd.plan_cols_tables(cols_ref.first_lengths()[n1])
    hq, h = n1 // 2 + 1, n1 // 2
    assert (t["n1"], t["hq"], t["mt"], t["ks"]) == (n1, hq, (2 * hq + 31) // 32, (n1 + 31) // 32)
    w = cols_ref.wq(n1)
    assert np.array_equal(t["wq"], w)
    tw = cols_ref.row_twiddles(w, np.arange(hq))                       # [hq][n1][2]
    corr = 128 * tw.sum(axis=1)                                        # [hq][2]
    assert np.array_equal(t["corr"], corr.astype(np.float64)) and np.abs(corr).max() < 2 ** 53
    # the un-split image: rows 2 q1 (Re), 2 q1 + 1 (Im); zero beyond the hq rows and the n1 samples
    rows = tw.transpose(0, 2, 1).reshape(2 * hq, n1)
    want = np.zeros((3, 32 * t["mt"], 32 * t["ks"]), np.int64)
    want[:, :2 * hq, :n1] = cols_ref.balanced_digits(rows)
    digits = _image_rows(t["image"])
    assert np.array_equal(digits, want)
    assert np.array_equal(want[0] + 256 * want[1] + 65536 * want[2], np.pad(rows, ((0, want.shape[1] - 2 * hq), (0, want.shape[2] - n1))))

    x = _columns(n1)
    exact = cols_ref.column_dft(w, x).reshape(2 * hq, -1)              # rows as the image's
    lo, hi = cols_ref.sample_digits(x)
    assert np.array_equal(256 * hi + lo + 128, x.astype(np.int64))
    pad = ((0, 32 * t["ks"] - n1), (0, 0))                             # samples past n1 meet zero digits: any value
    lo_p, hi_p = np.pad(lo, pad, constant_values=77), np.pad(hi, pad, constant_values=-99)
    # fwd_cols_q3_kernel and fwd_cols_q_kernel<SMALL>: G = 2^16 (acc_2 + 2^8 acc_3) + (acc_0 + 2^8 acc_1) + corr
    p_lo, p_hi, acc = _paired(digits, lo_p, hi_p)
    g = (p_hi * 65536 + p_lo)[:2 * hq] + corr.reshape(-1, 1)
    assert np.array_equal(g, exact)
    # fwd_cols_q_kernel<not SMALL>: sum_c acc_c 2^(8 c) + corr, no pairing
    g = sum(acc[c] << (8 * c) for c in range(4))[:2 * hq] + corr.reshape(-1, 1)
    assert np.array_equal(g, exact)
    assert np.abs(exact).max() < 2 ** 53                               # exact in the epilogue's double

    if n1 % 2 or n1 > cols_ref.REG_N1:
        assert t["image2"] is None
        return
    # fwd_cols_q4_kernel: the rows q1 <= h / 2 from E and O, the rows h - q1 from the same two sums
    assert t["image2"] is not None, "even n1 <= 224 takes the parity-split kernel"
    nq1 = h // 2 + 1
    assert (t["mt2"], t["ks2"]) == ((2 * nq1 + 15) // 16, (h + 63) // 64) and t["ks2"] <= 2
    want2 = np.zeros((3, 2, 16 * t["mt2"], 64 * t["ks2"]), np.int64)
    for par in range(2):
        want2[:, par, :2 * nq1, :h] = cols_ref.balanced_digits(rows[:2 * nq1, par::2])
    d2 = _image2_rows(t["image2"], t["ks2"])
    assert np.array_equal(d2, want2)
    pad = ((0, 64 * t["ks2"] - h), (0, 0))
    e_lo, e_hi, _ = _paired(d2[:, 0], np.pad(lo[0::2], pad, constant_values=77), np.pad(hi[0::2], pad, constant_values=-99))
    o_lo, o_hi, _ = _paired(d2[:, 1], np.pad(lo[1::2], pad, constant_values=77), np.pad(hi[1::2], pad, constant_values=-99))
    got = np.zeros_like(exact)
    written = np.zeros(2 * hq, bool)
    for q1 in range(nq1):
        for part in range(2):
            r = 2 * q1 + part
            got[r] = _int32(e_hi[r] + o_hi[r]) * 65536 + _int32(e_lo[r] + o_lo[r]) + corr[q1, part]
            written[r] = True
            if 2 * q1 < h:                                  # (h even: row h / 2 is reached by both formulas, written by the first)
                m_lo, m_hi = (o_lo[r] - e_lo[r], o_hi[r] - e_hi[r]) if part else (e_lo[r] - o_lo[r], e_hi[r] - o_hi[r])
                rm = 2 * (h - q1) + part
                assert not written[rm]
                got[rm] = _int32(m_hi) * 65536 + _int32(m_lo) + corr[h - q1, part]
                written[rm] = True
    assert written.all()
    assert np.array_equal(got, exact)
