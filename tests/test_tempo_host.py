"""CPU tests of the tempo query: the entry points are declared and exported, bad tempo lists are
refused before any device is touched, the library's common length equals the restatement's, and the numpy restatements of
tests/tempo_ref.py hold."""
import ctypes
import os
import re

import numpy as np
import pytest

import hpfw_amd
from hpfw_amd import _lib, synth

import tempo_ref as ref
import transpose_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
SYMS = ("hpfw_gpu_tempo_columns", "hpfw_gpu_hashprints_from_db_tempo", "hpfw_gpu_extract_tempo_pcm16",
        "hpfw_gpu_extract_tempo_pcm16_host")
BAD = [[], [1.0] * 65, [float("nan")], [float("inf")], [0.0], [-1.0], [0.49], [2.01], [1.0, float("nan")], [1.0, 1.0000001]]


def test_entry_points_are_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hpfw_gpu.h")).read(), flags=re.S)
    for sym in SYMS:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTS and hasattr(hpfw_amd.lib(), sym)


def _arr(vals, dtype):
    a = np.ascontiguousarray(vals, dtype)
    return a, a.ctypes.data_as(ctypes.c_void_p), a.size


def _calls(L, tp, nt, sp, ns):
    """the four entry points with a NULL handle (and NULL buffers): every one must refuse before using them"""
    out = ctypes.c_int64()
    return {
        "extract": L.hpfw_gpu_extract_tempo_pcm16(None, None, 220500, 1, tp, nt, sp, ns, None, None),
        "extract_host": L.hpfw_gpu_extract_tempo_pcm16_host(None, None, 220500, 1, tp, nt, sp, ns, None),
        "from_db": L.hpfw_gpu_hashprints_from_db_tempo(None, None, 1, 403, tp, nt, sp, ns, None, None),
        "columns": L.hpfw_gpu_tempo_columns(403, tp, nt, ctypes.byref(out)) if ns == 0 else E_INVALID,
    }


def test_bad_tempo_lists_are_invalid():
    L = hpfw_amd.lib()
    for vals in BAD:
        keep, tp, nt = _arr(vals, np.float32)
        for name, rc in _calls(L, tp, nt, None, 0).items():
            assert rc == E_INVALID, (vals, name)
            assert b"tempos" in L.hpfw_gpu_last_error(), (vals, name)
    assert L.hpfw_gpu_tempo_columns(403, None, 1, None) == E_INVALID
    # 16 tempos x 5 shifts = 80 variants; a good tempo list with a bad shift list; shifts without a list
    keep, tp, nt = _arr(np.linspace(0.9, 1.1, 16), np.float32)
    keep_s, sp, ns = _arr([-4, -2, 0, 2, 4], np.int32)
    for name, rc in _calls(L, tp, nt, sp, ns).items():
        assert rc == E_INVALID, name
    keep, tp, nt = _arr([0.96, 1.0], np.float32)
    for shifts in ([2, 2], [121], list(range(65))):
        keep_s, sp, ns = _arr(shifts, np.int32)
        for name, rc in _calls(L, tp, nt, sp, ns).items():
            assert rc == E_INVALID, (shifts, name)
    for name, rc in _calls(L, tp, nt, None, 2).items():
        assert rc == E_INVALID, name
    # good lists, null handle
    keep_s, sp, ns = _arr([-2, 0, 2], np.int32)
    for s_args in ((None, 0), (sp, ns)):
        rc = _calls(L, tp, nt, *s_args)
        for name in ("extract", "extract_host", "from_db"):
            assert rc[name] == E_INVALID, name
            assert b"null handle" in L.hpfw_gpu_last_error()
    out = ctypes.c_int64()
    keep, tp, nt = _arr([0.5, 1.0, 2.0] + [1.0 + 0.01 * i for i in range(1, 62)], np.float32)   # 64 tempos: accepted
    assert L.hpfw_gpu_tempo_columns(403, tp, nt, ctypes.byref(out)) == 0 and out.value == (402 * 65536) // 131072 + 1


def test_tempo_columns_equal_the_restatement():
    L = hpfw_amd.lib()
    rng = np.random.default_rng(12)
    lists = [[1.0], [0.5], [2.0], [0.5, 1.0, 2.0], [0.92, 0.96, 1.0, 1.04, 1.08], [1.08, 2.0], [0.97], [1.5, 0.75],
             list(rng.uniform(0.5, 2.0, 7))]
    cs = np.unique(np.concatenate([np.arange(100, 1200), rng.integers(100, 90_001, 2000), [90_000, 89_999, 2420, 403]]))
    out = ctypes.c_int64()
    for tempos in lists:
        keep, tp, nt = _arr(tempos, np.float32)
        for c in cs:
            assert L.hpfw_gpu_tempo_columns(int(c), tp, nt, ctypes.byref(out)) == 0
            assert out.value == ref.tempo_columns(int(c), np.float32(tempos)), (tempos, c)
        assert _lib.tempo_columns(403, tempos) == ref.tempo_columns(403, np.float32(tempos))
    assert ref.tempo_columns(403, [0.92]) == 370 and ref.tempo_columns(403, [1.0]) == 403
    assert ref.tempo_step(1.0) == 65536 and ref.tempo_step(0.5) == 131072 and ref.tempo_step(2.0) == 32768


def _random_db(rng, c, rows=121):
    db = (-80 * rng.random((rows, c))).astype(np.float32)
    db[rng.random((rows, c)) < 0.2] = -80.0                                  # the floor, as the dB conversion leaves it
    db[rng.random((rows, c)) < 0.01] = 0.0
    return db


def test_scale_db_properties():
    rng = np.random.default_rng(3)
    for c in (100, 403, 1001, 2420):
        db = _random_db(rng, c)
        assert np.array_equal(ref.scale_db(db, 1.0).view(np.uint32), db.view(np.uint32))
        half = ref.scale_db(db, 0.5)
        assert half.shape[1] == (c - 1) // 2 + 1 and np.array_equal(half, db[:, ::2])
        dbl = ref.scale_db(db, 2.0)
        assert dbl.shape[1] == 2 * c - 1
        assert np.array_equal(dbl[:, ::2], db)
        mid = ((db[:, :-1].astype(np.float64) + db[:, 1:].astype(np.float64)) / 2).astype(np.float32)
        assert np.array_equal(dbl[:, 1::2], mid)
        for rho in (0.92, 0.97, 1.04, 1.08, 0.5, 2.0, 1.5):
            s = ref.scale_db(db, rho)
            step = ref.tempo_step(rho)
            p = np.arange(s.shape[1], dtype=np.int64) * step
            i = p >> 16
            a, b = db[:, i], db[:, np.minimum(i + 1, c - 1)]
            assert (s >= np.minimum(a, b)).all() and (s <= np.maximum(a, b)).all(), rho
            assert (s >= -80).all() and (s <= 0).all()
            assert i[-1] <= c - 1 and s.shape[1] * step > (c - 1) * 65536    # C_rho: every column whose position lies in S


def test_scale_and_shift_commute():
    rng = np.random.default_rng(4)
    for trial in range(20):
        c = int(rng.integers(100, 700))
        db = _random_db(rng, c)
        rho = float(rng.choice([0.5, 0.92, 0.96, 1.0, 1.04, 1.08, 2.0, rng.uniform(0.5, 2.0)]))
        s = int(rng.integers(-30, 31))
        a = transpose_ref.shift_db(ref.scale_db(db, rho), s)
        b = ref.scale_db(transpose_ref.shift_db(db, s), rho)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (trial, rho, s)


def test_tempo_clip_at_tempo_one_is_gen_clip():
    for cid, sec in ((0, 2.0), (7, 3.3), (3, 30.0)):
        x = ref.gen_clip(cid, sec)
        assert np.array_equal(x, synth.gen_clip(cid, sec)) and np.array_equal(x, transpose_ref.gen_clip(cid, sec))
    up = 2 ** (1 / 12)
    assert np.array_equal(ref.gen_clip(5, 4.0, factor=up), transpose_ref.gen_clip(5, 4.0, factor=up))
    fast = ref.gen_clip(0, 30.0, tempo=1.08)
    assert fast.size == round(30.0 * synth.SR / 1.08) and not np.array_equal(fast[11025:12025], synth.gen_clip(0, 30.0)[11025:12025])
    assert ref.gen_clip(0, 30.0, tempo=0.92).size == round(30.0 * synth.SR / 0.92)


def test_tempo_lists_are_checked_in_python():
    assert _lib.check_tempos([0.92, 1.0, 1.08]) == [float(np.float32(t)) for t in (0.92, 1.0, 1.08)]
    assert len(_lib.check_tempos(np.linspace(0.5, 2.0, 64))) == 64
    assert len(_lib.check_tempos(np.linspace(0.9, 1.1, 16), 4)) == 16
    for bad, n_shifts in [(b, 0) for b in BAD] + [(list(np.linspace(0.9, 1.1, 16)), 5), ([1.0, 1.04], 33)]:
        with pytest.raises(ValueError):
            _lib.check_tempos(bad, n_shifts)


FACADE = r"""
#include <hpfw/gpu/gpu_collector.h>
#include <hpfw/gpu/gpu_storage.h>
#include <hpfw/gpu/tempo.h>
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    hpfw::db::GpuStorage<hpfw::GpuCollector> storage;
    hpfw_gpu *h = nullptr;
    if (hpfw_gpu_create(0, &h) != 0) return 1;
    const std::vector<float> tempos{0.96f, 1.0f, 1.04f};
    auto per_variant = hpfw::tempo_hashprints(h, argv[1], tempos);
    auto both = hpfw::tempo_hashprints(h, argv[1], tempos, {-2, 0, 2});
    auto top = storage.find_topk_transposed(per_variant, 10);
    hpfw_gpu_destroy(h);
    return top.empty() || both.empty() ? 0 : top[0].shift_index;
}
"""


def test_tempo_facade_compiles_and_links(tmp_path):
    import subprocess
    src = tmp_path / "tempo.cpp"
    src.write_text(FACADE)
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
           str(tmp_path / "tempo"), "-L", lib_dir, "-lhpfw_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "tempo")], capture_output=True, text=True)   # no argument: no device touched
    assert r.returncode == 2
