"""S6's row stage without a GPU, at every row length n2 the planner reaches (tests/rows_ref.py): the frozen sweep, what
it covers of the run-time dispatcher (fused kinds, last groups, loader classes), the library's plan and the row kernel's
body in the SIMT emulation (tests/emu/emu_rows.cpp) against the oracle, and the oracle's forward bins against float64.
The GPU side is tests/test_gpu_rows_sweep.py."""
import os
import re
import subprocess

import pytest

import cols_ref
import rows_ref
from test_cols_host import FLOAT64_BAR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "emu", "emu_rows.cpp"), os.path.join(ROOT, "hpfw_amd", "csrc", "plan.cpp"),
           os.path.join(ROOT, "oracle", "hpfw_oracle.c")]
FLAGS = ["-std=c++17", "-DHPFW_SIMT_EMU", "-ffp-contract=off", "-mfma", "-mavx2"]
THREADS = 512               # the row kernel's workgroup

# (n, n2): the first length of every row length, in the order of n: frozen, so that a change of the planner's rule shows
# as a diff here and not as silently different coverage
ROW_SWEEP = (
    (54432, 6804), (54675, 6075), (54880, 5488), (55125, 6125), (55296, 6144), (55566, 6174), (56000, 5600), (56250, 6250),
    (56448, 6272), (56700, 6300), (57344, 4096), (57600, 6400), (57624, 4802), (58320, 6480), (58800, 5880), (59049, 6561),
    (59535, 6615), (60000, 6000), (60025, 2401), (60480, 6720), (60750, 6750), (61440, 5120), (62208, 5184), (63504, 5292),
    (64512, 5376), (64827, 3087), (65625, 4375), (68600, 4900), (69120, 5760), (69984, 5832), (70000, 5000), (70875, 4725),
    (71442, 5103), (72576, 6048), (72900, 4860), (73500, 5250), (77175, 5145), (78125, 3125), (83349, 3969), (84375, 5625),
    (85050, 5670), (86400, 4800), (214326, 4374))
# one long length per loader class (odd, 0, 2) with n1 > 255: narrow consumed windows, many mirrored rows, the LDS-staged
# column kernel in front
ROW_LONG = ((1361367, 3969), (1680700, 4900), (1786050, 5670))
# the lengths that bring the fused kinds (3, 2) and (4, 1), and (4, 1), (4, 3) as the last group
NEW_KINDS = (55296, 63504, 69120, 214326)

ALL_LENGTHS = tuple(n for n, _ in ROW_SWEEP + ROW_LONG)


def test_sweep_is_the_frozen_list():
    first = rows_ref.row_lengths()
    assert len(ROW_SWEEP) == 43
    assert tuple((n, n2) for n2, n in first.items()) == ROW_SWEEP
    assert [n for n, _ in ROW_SWEEP] == sorted(n for n, _ in ROW_SWEEP)
    for n, n2 in ROW_SWEEP + ROW_LONG:
        n1, got = cols_ref.split(n)
        assert got == n2 and n1 <= rows_ref.N1_MAX and n >= cols_ref.FIRST_LENGTH
    assert [cols_ref.split(n)[0] for n, _ in ROW_LONG] == [343, 343, 315]
    assert [rows_ref.loader_class(n2) for _, n2 in ROW_LONG] == ["odd", 0, 2]
    # [7, 7, 5, 5, 4, 3, 3] -> 7 3 7 3 5 4 5 -> (7, 3) (7, 3) (5, 4) (5, 1)
    assert rows_ref.pass_order(44100) == [7, 3, 7, 3, 5, 4, 5]
    assert rows_ref.groups(6300) == [(7, 3), (5, 3), (5, 4)] and rows_ref.seq(6300) == "7x3,5x3,5x4"


def test_sweep_covers_every_kind_the_planner_reaches():
    """every fused kind (r1, r2), every kind in the last position and every loader class met over ALL accepted 7-smooth
    lengths occurs in the sweep; the row lengths above 255 x 6826 bring nothing the 43 lack"""
    kinds, last, loaders, n2s = set(), set(), set(), set()
    walked = cols_ref.smooth_lengths(cols_ref.FIRST_LENGTH, rows_ref.N1_MAX * cols_ref.N2_MAX)
    assert len(walked) == 2482
    for n in walked:
        n1, n2 = cols_ref.split(n)
        if n1 > rows_ref.N1_MAX or n2 in n2s:
            continue
        n2s.add(n2)
        g = rows_ref.groups(n2)
        assert all(a * b <= rows_ref.MAX_POINTS and a in (2, 3, 4, 5, 7) and b in (1, 2, 3, 4, 5, 7) for a, b in g)
        kinds |= set(g)
        last.add(g[-1])
        loaders.add(rows_ref.loader_class(n2))
    assert n2s == {n2 for _, n2 in ROW_SWEEP} and (min(n2s), max(n2s)) == (2401, 6804)
    seqs = [rows_ref.groups(n2) for _, n2 in ROW_SWEEP]
    assert {k for g in seqs for k in g} == kinds and len(kinds) == 17
    assert {g[-1] for g in seqs} == last and len(last) == 11
    assert {rows_ref.loader_class(n2) for _, n2 in ROW_SWEEP} == loaders == {0, 2, "odd"}
    assert sorted(len(g) for g in seqs) == [3] * 27 + [4] * 16 and len({tuple(g) for g in seqs}) == 43
    assert [[rows_ref.loader_class(n2) for _, n2 in ROW_SWEEP].count(c) for c in (0, 2, "odd")] == [23, 7, 13]
    assert {(3, 2), (4, 1)} <= kinds and {(4, 1), (4, 3)} <= last
    # the long lengths and the four of the sanitized run: on row lengths of the sweep
    assert {n2 for _, n2 in ROW_LONG} <= n2s and set(NEW_KINDS) <= {n for n, _ in ROW_SWEEP}
    new = [rows_ref.groups(cols_ref.split(n)[1]) for n in NEW_KINDS]
    assert any((3, 2) in g for g in new) and any((4, 1) in g for g in new)
    assert {g[-1] for g in new} >= {(4, 1), (4, 3)}


def _build(exe, extra):
    r = subprocess.run(["g++", *extra, *FLAGS, "-o", str(exe), *SOURCES, "-lm", "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


@pytest.fixture(scope="module")
def emu_rows(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("emu") / "emu_rows", ["-O2"])


def _fields(stdout):
    return dict(re.findall(r"(\w+)=(\S+)", stdout))


@pytest.mark.parametrize("n", ALL_LENGTHS)
def test_library_plan_and_row_body_match_the_restatement(emu_rows, n):
    """the library's planner (plan.cpp, compiled into the emulator) splits and groups as cols_ref / rows_ref state it, and
    rows2_body with those groups, 512 emulated threads and bounds-checked LDS gives the oracle's bits"""
    r = subprocess.run([emu_rows, str(n), str(THREADS)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    f = _fields(r.stdout)
    assert f["mismatches"] == "0" and int(f["values"]) > 0, r.stdout
    n1, n2 = cols_ref.split(n)
    assert (int(f["n"]), int(f["n1"]), int(f["n2"])) == (n, n1, n2), r.stdout
    assert f["seq"] == rows_ref.seq(n2) and int(f["groups"]) == len(rows_ref.groups(n2)), r.stdout


@pytest.mark.parametrize("n", ALL_LENGTHS)
def test_oracle_against_float64(oracle, n):
    """the reference of the GPU sweep on its own: forward bins of both clips of the column sweep within the bar"""
    plan = oracle.Plan(n)
    assert (plan.n1, plan.n2) == cols_ref.split(n)
    for kind, clip in (("noise", cols_ref.noise_clip(n)), ("worst", cols_ref.worst_clip(n))):
        err = cols_ref.float64_error(plan.spectrum(clip), clip, plan.kmin, plan.kmax)
        print(f"n = {n} = {plan.n1} x {plan.n2}, {kind}: {err:.3g}")
        assert err < FLOAT64_BAR, (n, kind, err)


def test_sanitized_run_of_the_new_kinds(tmp_path):
    """the stand-alone emulator under AddressSanitizer and UBSan at the four lengths that bring (3, 2), (4, 1) and the last
    groups (4, 1), (4, 3)"""
    exe = _build(tmp_path / "emu_rows_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    for n in NEW_KINDS:
        r = subprocess.run([exe, str(n), str(THREADS)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr[-3000:]
        assert _fields(r.stdout)["mismatches"] == "0" and "runtime error" not in r.stderr, r.stdout + r.stderr[-3000:]
