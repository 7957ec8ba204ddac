"""The plain arithmetic of the per-length table cache (hpfw_amd/csrc/plan_cache.h) without a GPU: which plans an incoming
plan evicts and where the device-wide wait falls, and the layout by which the constant-Q stage finds the forward bins with
its two magic divisors.  tests/emu/plan_cache_check.cpp, a program of its own under ASan and UBSan."""
import os
import re
import shutil
import subprocess

import cols_ref
import rows_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_cache_arithmetic_under_sanitizers(tmp_path):
    """evictions: 6000 random caches (zero budget, an incoming plan above the budget, an empty cache, all or no plans known
    idle) against get_plan's former loop -- the same victims in the same order, one wait at most and before the same victim,
    three quarters of the budget as the goal behind a wait, the cache empty when nothing else fits.  Layout: k / n1 and
    t / nq2 by their magic divisors, every band below 2^19 entries, g2_off the running sum -- for the first length of every
    n1 the planner chooses, the lengths of the column and the row sweep, 88 200, 132 300, 1 323 000 and the longest clip"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "plan_cache_check"
    src = [os.path.join(ROOT, "tests", "emu", "plan_cache_check.cpp"), os.path.join(ROOT, "hpfw_amd", "csrc", "plan.cpp")]
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *src, "-o", str(exe),
                        "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lengths = sorted(set(cols_ref.sweep_lengths()) | set(rows_ref.row_lengths().values()))
    r = subprocess.run([str(exe), *map(str, lengths)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "plan_cache_check evictions ok: 6000 caches" in r.stdout
    m = re.search(r"plan_cache_check layout ok: (\d+) lengths .* with (\d+) values of n1 up to (\d+);", r.stdout)
    assert m, r.stdout
    n1s = {cols_ref.split(n)[0] for n in lengths}
    assert int(m.group(1)) >= len(lengths) and int(m.group(2)) >= len(n1s) and int(m.group(3)) == rows_ref.N1_MAX
