"""CPU tests of the transposed query: the entry points are declared and exported, bad arguments are
refused before any device is touched, and the numpy restatements of tests/transpose_ref.py hold."""
import ctypes
import os
import re

import numpy as np

import hpfw_amd
from hpfw_amd import _lib, synth

import transpose_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
SYMS = ("hpfw_gpu_extract_transposed_pcm16", "hpfw_gpu_extract_transposed_pcm16_host", "hpfw_gpu_hashprints_from_db_transposed",
        "hpfw_gpu_search_topk_transposed_device", "hpfw_gpu_search_topk_transposed")


def test_entry_points_are_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hpfw_gpu.h")).read(), flags=re.S)
    for sym in SYMS:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTS and hasattr(hpfw_amd.lib(), sym)
    assert "hpfw_shift_hit" in header
    assert _lib.SHIFT_HIT_DTYPE.itemsize == 16


def _shifts(vals):
    a = np.ascontiguousarray(vals, np.int32)
    return a, a.ctypes.data_as(ctypes.c_void_p), a.size


def test_bad_shifts_and_null_handle_are_invalid():
    L = hpfw_amd.lib()
    bad = [[], list(range(65)), [1, 2, 1], [121], [-121], [0, 200]]
    hp = np.zeros(8, np.uint64)
    for vals in bad:
        keep, p, n = _shifts(vals)
        assert L.hpfw_gpu_extract_transposed_pcm16(None, None, 0, 0, p, n, None, None) == E_INVALID, vals
        assert b"shifts" in L.hpfw_gpu_last_error(), vals
        assert L.hpfw_gpu_extract_transposed_pcm16_host(None, None, 0, 0, p, n, None) == E_INVALID
        assert L.hpfw_gpu_hashprints_from_db_transposed(None, None, 1, 200, p, n, None, None) == E_INVALID
    keep, p, n = _shifts([-120, 0, 120])                              # good shifts, null handle
    assert L.hpfw_gpu_extract_transposed_pcm16(None, None, 0, 0, p, n, None, None) == E_INVALID
    assert b"null handle" in L.hpfw_gpu_last_error()
    assert L.hpfw_gpu_extract_transposed_pcm16(None, None, 0, 0, None, 1, None, None) == E_INVALID
    off = np.zeros(3, np.int64)
    out = np.zeros(4, _lib.SHIFT_HIT_DTYPE)
    for n_shifts in (0, 65, 2):
        assert L.hpfw_gpu_search_topk_transposed(None, hp.ctypes.data_as(ctypes.c_void_p), off.ctypes.data_as(ctypes.c_void_p), 1,
                                                 n_shifts, 2, out.ctypes.data_as(ctypes.c_void_p)) == E_INVALID
        assert L.hpfw_gpu_search_topk_transposed_device(None, None, off.ctypes.data_as(ctypes.c_void_p), 1, n_shifts, 2,
                                                        None, None) == E_INVALID


def test_transposed_clip_at_factor_one_is_gen_clip():
    for cid, sec in ((0, 2.0), (7, 3.3)):
        assert np.array_equal(ref.gen_clip(cid, sec), synth.gen_clip(cid, sec))
    assert not np.array_equal(ref.gen_clip(0, 2.0, factor=2 ** (1 / 12)), synth.gen_clip(0, 2.0))


def test_shift_db():
    db = np.arange(121 * 3, dtype=np.float32).reshape(121, 3) - 500
    assert np.array_equal(ref.shift_db(db, 0), db)
    s2 = ref.shift_db(db, 2)
    assert np.array_equal(s2[:119], db[2:]) and (s2[119:] == -80).all()
    m3 = ref.shift_db(db, -3)
    assert np.array_equal(m3[3:], db[:118]) and (m3[:3] == -80).all()
    assert (ref.shift_db(db, 121) == -80).all() and (ref.shift_db(db, -120)[120] == db[0]).all()


def _topk(d, k):
    """exact top-k of one dist row [n_clips] (offset = clip for tracing), ascending (dist, clip), padded"""
    order = sorted(range(d.size), key=lambda c: (d[c], c))[:k]
    row = np.zeros(k, _lib.HIT_DTYPE)
    row["dist"], row["clip"] = 0xFFFFFFFF, 0xFFFFFFFF
    for t, c in enumerate(order):
        row[t] = (d[c], c, 1000 + c, 0)
    return row


def test_merge_restatement_equals_brute_force():
    """the union of per-shift top-k lists, per clip its best (dist, shift index), then the k best (dist, clip), against
    the minimum over the shifts of the full distance table -- with planted ties (two identical shifts, equal distances)"""
    rng = np.random.default_rng(11)
    for trial in range(200):
        n_clips, S, k = int(rng.integers(1, 12)), int(rng.integers(1, 6)), int(rng.integers(1, 8))
        d = rng.integers(0, 6, size=(S, n_clips))                       # small range: many ties
        if S > 1 and trial % 3 == 0:
            d[S - 1] = d[0]                                             # a duplicated shift
        lists = np.stack([_topk(d[s], k) for s in range(S)])[None]
        got = ref.merge_shifts(lists, k)[0]
        best = [(int(d[:, c].min()), c, int(np.argmin(d[:, c]))) for c in range(n_clips)]   # argmin: first shift
        want = sorted(best)[:k]
        want = [(dd, c, 1000 + c, si) for dd, c, si in want] + [(0xFFFFFFFF, 0xFFFFFFFF, 0, -1)] * (k - len(want))
        assert got == want, (trial, d, k)


FACADE = r"""
#include <hpfw/gpu/gpu_collector.h>
#include <hpfw/gpu/gpu_storage.h>
#include <hpfw/gpu/transposed.h>
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    hpfw::db::GpuStorage<hpfw::GpuCollector> storage;
    hpfw_gpu *h = nullptr;
    if (hpfw_gpu_create(0, &h) != 0) return 1;
    auto per_shift = hpfw::transposed_hashprints(h, argv[1], {-2, 0, 2});
    auto top = storage.find_topk_transposed(per_shift, 10);
    hpfw_gpu_destroy(h);
    return top.empty() ? 0 : top[0].shift_index;
}
"""


def test_transposed_facade_compiles_and_links(tmp_path):
    import subprocess
    src = tmp_path / "transposed.cpp"
    src.write_text(FACADE)
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(tmp_path / "transposed"), "-L", lib_dir, "-lhpfw_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "transposed")], capture_output=True, text=True)   # no argument: no device touched
    assert r.returncode == 2


def test_shift_lists_are_checked_in_python():
    assert _lib.check_shifts(np.array([-4, 0, 4])) == [-4, 0, 4]
    assert _lib.check_shifts(range(-120, -56)) == list(range(-120, -56))
    for bad in ([], [2, 2], [121], [-121], list(range(65))):
        try:
            _lib.check_shifts(bad)
        except ValueError:
            continue
        raise AssertionError(bad)


def test_library_errors_carry_their_status():
    L = hpfw_amd.lib()
    keep, p, n = _shifts([2, 2])
    try:
        _lib.check(L.hpfw_gpu_extract_transposed_pcm16(None, None, 0, 0, p, n, None, None))
    except hpfw_amd.HpfwError as e:
        assert e.status == _lib.E_INVALID and "shifts" in str(e)
    else:
        raise AssertionError("no error")
    try:
        _lib.wav_read("/nonexistent/file.wav")
    except hpfw_amd.HpfwError as e:
        assert e.status == _lib.E_IO
    else:
        raise AssertionError("no error")
