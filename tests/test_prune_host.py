"""What the row transform leaves out (HPFW_PRUNE: last-group outputs that nothing reads), checked on the host:
tests/emu/emu_prune.cpp runs the pruned kernel body against the full one in the SIMT emulation, bit for bit, and the
plan's rule for picking the pruned row kernel.  The GPU side is tests/test_gpu_prune.py."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "emu", "emu_prune.cpp"), os.path.join(ROOT, "hpfw_amd", "csrc", "plan.cpp")]
FLAGS = ["-std=c++17", "-DHPFW_SIMT_EMU", "-ffp-contract=off", "-mfma", "-mavx2"]


def _build(exe, extra):
    r = subprocess.run(["g++", *extra, *FLAGS, "-o", str(exe), *SOURCES, "-lm", "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


@pytest.fixture(scope="module")
def full_run(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("emu") / "emu_prune", ["-O2"])
    r = subprocess.run([exe, "full"], capture_output=True, text=True)
    return r


def test_pruned_bodies_match_full_bit_for_bit(full_run):
    """rows: LastEdges against LastAll on the LDS positions the epilogue reads and on the stored bins, for the shortest and
    the longest clip with n2 = 6300 and the 30 s clip"""
    assert full_run.returncode == 0, full_run.stdout + full_run.stderr
    assert "mismatches=0" in full_run.stdout
    rows = re.findall(r"^rows n=(\d+) .* positions=(\d+)$", full_run.stdout, re.M)
    assert len(rows) == 3 and all(int(p) > 3000 for _, p in rows), full_run.stdout


def test_plan_rule_selects_pruned_or_full(full_run):
    """windows inside outputs {0, 1, 18, 19} take the pruned kernel, a q2w of 640 (output 2) and the others the full one"""
    assert full_run.returncode == 0, full_run.stdout + full_run.stderr
    rule = dict(((int(a), int(b)), c) for a, b, c in re.findall(r"^rule q2lo=(\d+) q2w=(\d+) mask=\S+ (\w+)$", full_run.stdout, re.M))
    assert rule[(18, 598)] == "pruned" and rule[(18, 640)] == "full" and rule[(0, 6300)] == "full", full_run.stdout
    assert sorted(rule.values()).count("pruned") == 5 and len(rule) == 10


def test_sanitized_quick_run(tmp_path):
    """the same stand-alone program under AddressSanitizer and UBSan: two rows of one geometry and the plan rule"""
    exe = _build(tmp_path / "emu_prune_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, "quick"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "mismatches=0" in r.stdout and "runtime error" not in r.stderr
