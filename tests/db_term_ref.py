"""The host program of tests/emu/db_term_check.cpp for the tests: built once per session, its result line as a dict, and
the results recorded from its exhaustive mode (tests/golden/db_term_check.json)."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "db_term_check.cpp")
CAP = 1e-4          # the largest share of inputs for which the fast evaluation may run the specified sequence after all
LOWEST, MILLION, INF = 0x2EDBE6FF, 0x49742400, 0x7F800000   # the bit patterns of 1e-10f, 1e6f and +inf

_BUILT = {}


def build(tmp_path_factory, sanitize=False):
    """the program, compiled like tests/emu's others (no implicit fusing, the hardware's fused multiply-add)"""
    if sanitize not in _BUILT:
        exe = tmp_path_factory.mktemp("db_term") / ("check_san" if sanitize else "check")
        opt = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
        cmd = ["g++", *opt, "-std=c++17", "-DHPFW_SIMT_EMU", "-ffp-contract=off", "-mfma", "-o", str(exe), SRC, "-lpthread"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        _BUILT[sanitize] = str(exe)
    return _BUILT[sanitize]


def run(exe, *args):
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(kv.split("=", 1) for kv in r.stdout.split())


def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "db_term_check.json")) as f:
        return json.load(f)
