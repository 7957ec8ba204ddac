"""ctypes binding of libhpfw_gpu_multi.so (include/hpfw_gpu_multi.h): the native multi-GPU host path -- one
process, one handle per shard, one RCCL all-gather of the per-shard top-k lists per search.  (bench.py's N > 1
leg runs one process per GPU under torch.distributed instead, as its launch contract demands; both use the
same shard arithmetic and the same merge.)"""
import ctypes
import os

import numpy as np

from . import _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libhpfw_gpu_multi.so")

EXPORTS = (
    "hpfw_gpu_group_create", "hpfw_gpu_group_create_env", "hpfw_gpu_group_destroy", "hpfw_gpu_group_size",
    "hpfw_gpu_group_handle", "hpfw_gpu_group_exchange", "hpfw_gpu_group_set_filters",
    "hpfw_gpu_group_extract_pcm16", "hpfw_gpu_group_index_build", "hpfw_gpu_group_index_size",
    "hpfw_gpu_shard_range", "hpfw_gpu_group_search_topk", "hpfw_gpu_group_cov_reset",
    "hpfw_gpu_group_cov_accumulate_pcm16", "hpfw_gpu_group_learn_filters",
    "hpfw_gpu_group_load", "hpfw_gpu_group_save", "hpfw_gpu_group_prepare", "hpfw_gpu_group_calc_hashprint",
)
# include/hpfw_gpu_multi_resample.h
RESAMPLE_EXPORTS = ("hpfw_gpu_group_set_resample",)
# include/hpfw_gpu_multi_search.h
SEARCH_EXPORTS = (
    "hpfw_gpu_group_search_topk_scored", "hpfw_gpu_group_search_topk_transposed",
    "hpfw_gpu_group_search_topk_transposed_scored", "hpfw_gpu_group_extract_windows_pcm16",
)
# include/hpfw_gpu_multi_votes.h
VOTES_EXPORTS = ("hpfw_gpu_group_search_votes",)
# include/hpfw_gpu_multi_index.h
INDEX_EXPORTS = ("hpfw_gpu_group_index_remove",)

_multi = None


def lib():
    global _multi
    if _multi is not None:
        return _multi
    _lib.lib()                                             # libhpfw_gpu.so first (the multi library is built on it)
    if not os.path.exists(LIB_PATH):
        raise _lib.HpfwError(f"{LIB_PATH} is missing: build it with hpfw_amd.build.build()")
    L = ctypes.CDLL(LIB_PATH)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    L.hpfw_gpu_group_create.argtypes = [vp, i32, ctypes.POINTER(vp)]
    L.hpfw_gpu_group_create_env.argtypes = [ctypes.POINTER(vp)]
    L.hpfw_gpu_group_destroy.argtypes = [vp]
    L.hpfw_gpu_group_destroy.restype = None
    L.hpfw_gpu_group_size.argtypes = [vp]
    L.hpfw_gpu_group_handle.argtypes = [vp, i32]
    L.hpfw_gpu_group_handle.restype = vp
    L.hpfw_gpu_group_exchange.argtypes = [vp]
    L.hpfw_gpu_group_exchange.restype = ctypes.c_char_p
    L.hpfw_gpu_group_set_filters.argtypes = [vp, vp]
    L.hpfw_gpu_group_extract_pcm16.argtypes = [vp, vp, i64, i64, vp]
    L.hpfw_gpu_group_index_build.argtypes = [vp, vp, vp, i64]
    L.hpfw_gpu_group_index_size.argtypes = [vp]
    L.hpfw_gpu_group_index_size.restype = i64
    L.hpfw_gpu_shard_range.argtypes = [i64, i32, i32, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.hpfw_gpu_shard_range.restype = None
    L.hpfw_gpu_group_search_topk.argtypes = [vp, vp, vp, i64, i32, vp]
    L.hpfw_gpu_group_cov_reset.argtypes = [vp]
    L.hpfw_gpu_group_cov_accumulate_pcm16.argtypes = [vp, vp, i64, i64]
    L.hpfw_gpu_group_learn_filters.argtypes = [vp, vp]
    L.hpfw_gpu_group_load.argtypes = [vp, ctypes.c_char_p]
    L.hpfw_gpu_group_save.argtypes = [vp, ctypes.c_char_p]
    L.hpfw_gpu_group_prepare.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), i32, ctypes.POINTER(i32)]
    L.hpfw_gpu_group_prepare.restype = ctypes.POINTER(_lib.FilenameHashprintPair)
    L.hpfw_gpu_group_calc_hashprint.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(i32)]
    L.hpfw_gpu_group_calc_hashprint.restype = ctypes.POINTER(ctypes.c_uint64)
    L.hpfw_gpu_group_set_resample.argtypes = [vp, i32]
    L.hpfw_gpu_group_search_topk_scored.argtypes = [vp, vp, vp, i64, i32, vp, vp]
    L.hpfw_gpu_group_search_topk_transposed.argtypes = [vp, vp, vp, i64, i32, i32, vp]
    L.hpfw_gpu_group_search_topk_transposed_scored.argtypes = [vp, vp, vp, i64, i32, i32, vp, vp]
    L.hpfw_gpu_group_extract_windows_pcm16.argtypes = [vp, vp, i64, i64, i64, vp, i32, vp, i32, vp]
    L.hpfw_gpu_group_search_votes.argtypes = [vp, vp, vp, i64, vp]
    L.hpfw_gpu_group_index_remove.argtypes = [vp, vp, i64]
    _multi = L
    return L


def shard_range(n_clips, shard, n_shards):
    lo, hi = ctypes.c_int64(0), ctypes.c_int64(0)
    lib().hpfw_gpu_shard_range(int(n_clips), int(shard), int(n_shards), ctypes.byref(lo), ctypes.byref(hi))
    return int(lo.value), int(hi.value)


class GpuGroup:
    """devices: one ordinal per shard (an ordinal may repeat); None = HPFW_GPU_DEVICES / every visible device"""

    def __init__(self, devices=None):
        self._g = ctypes.c_void_p()
        self._offsets = np.zeros(1, np.int64)
        if devices is None:
            _lib.check(lib().hpfw_gpu_group_create_env(ctypes.byref(self._g)))
        else:
            d = np.ascontiguousarray(devices, np.int32)
            _lib.check(lib().hpfw_gpu_group_create(_lib._hp(d), d.size, ctypes.byref(self._g)))

    def close(self):
        if getattr(self, "_g", None):
            lib().hpfw_gpu_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def shards(self):
        return int(lib().hpfw_gpu_group_size(self._g))

    def handle(self, shard):
        """the hpfw_gpu handle of a shard (owned by the group): wrap it with hpfw_amd.Gpu.from_handle"""
        h = lib().hpfw_gpu_group_handle(self._g, int(shard))
        if not h:
            raise _lib.HpfwError(f"no shard {shard}")
        return h

    @property
    def exchange(self):
        return lib().hpfw_gpu_group_exchange(self._g).decode()

    def set_filters(self, filters_colmajor):
        f = np.ascontiguousarray(filters_colmajor, np.float32).ravel()
        assert f.size == 64 * 2420
        _lib.check(lib().hpfw_gpu_group_set_filters(self._g, _lib._hp(f)))

    def extract(self, pcm, n_hp):
        pcm = np.ascontiguousarray(pcm, np.int16)
        hp = np.zeros((pcm.shape[0], n_hp), np.uint64)
        _lib.check(lib().hpfw_gpu_group_extract_pcm16(self._g, _lib._hp(pcm), pcm.shape[1], pcm.shape[0], _lib._hp(hp)))
        return hp

    def index_build(self, hp, offsets):
        hp = np.ascontiguousarray(hp, np.uint64).ravel()
        off = np.ascontiguousarray(offsets, np.int64)
        _lib.check(lib().hpfw_gpu_group_index_build(self._g, _lib._hp(hp), _lib._hp(off), off.size - 1))
        self._offsets = off - off[0]

    def index_offsets(self):
        """the clip offsets int64 [n_clips + 1] of the index as index_build last took it and index_remove left it, from 0 (as
        Gpu.index_offsets)"""
        return self._offsets.copy()

    def index_remove(self, clips):
        """the clips named (global ids) become empty on the shards that hold them; ids and the shards' ranges stay (DESIGN.md
        section 21).  Adding to a sharded index is not offered: rebuild with index_build."""
        ids = np.ascontiguousarray(clips, np.int64).ravel()
        _lib.check(lib().hpfw_gpu_group_index_remove(self._g, _lib._hp(ids) if ids.size else None, ids.size))
        lengths = np.diff(self._offsets)
        lengths[ids] = 0
        self._offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)

    def _search(self, fn, q_hp, q_off, n_q, extra, k, hit_dtype, stats_shape=None):
        """contiguous queries and offsets in, fn(group, q, off, n_q, *extra, k, out[, stats]), out [n_q][k] (and the moments) back"""
        q = np.ascontiguousarray(q_hp, np.uint64).ravel()
        off = np.ascontiguousarray(q_off, np.int64)
        out = np.zeros((n_q, k), hit_dtype)
        stats = None if stats_shape is None else np.zeros(stats_shape, _lib.STATS_DTYPE)
        tail = () if stats is None else (_lib._hp(stats),)
        _lib.check(fn(self._g, _lib._hp(q), _lib._hp(off), n_q, *extra, int(k), _lib._hp(out), *tail))
        return out if stats is None else (out, stats)

    def search_topk(self, q_hp, q_off, k):
        return self._search(lib().hpfw_gpu_group_search_topk, q_hp, q_off, np.size(q_off) - 1, (), k, _lib.HIT_DTYPE)

    # ---- key, tempo and scored searches, windows (include/hpfw_gpu_multi_search.h): what their Gpu namesakes return
    def search_topk_scored(self, q_hp, q_off, k):
        """(HIT_DTYPE [n_q][k], STATS_DTYPE [n_q])"""
        n_q = np.size(q_off) - 1
        return self._search(lib().hpfw_gpu_group_search_topk_scored, q_hp, q_off, n_q, (), k, _lib.HIT_DTYPE, n_q)

    def _transposed(self, q_hp, q_off, n_shifts, k, scored):
        sets = np.size(q_off) - 1
        if n_shifts < 1 or sets % n_shifts:
            raise ValueError("q_off must hold n_q * n_shifts + 1 offsets")
        n_q = sets // n_shifts
        fn = lib().hpfw_gpu_group_search_topk_transposed_scored if scored else lib().hpfw_gpu_group_search_topk_transposed
        return self._search(fn, q_hp, q_off, n_q, (int(n_shifts),), k, _lib.SHIFT_HIT_DTYPE, (n_q, n_shifts) if scored else None)

    def search_topk_transposed(self, q_hp, q_off, n_shifts, k):
        """q_off [n_q * n_shifts + 1] -> SHIFT_HIT_DTYPE [n_q][k]"""
        return self._transposed(q_hp, q_off, n_shifts, k, False)

    def search_topk_transposed_scored(self, q_hp, q_off, n_shifts, k):
        """(SHIFT_HIT_DTYPE [n_q][k], STATS_DTYPE [n_q][n_shifts])"""
        return self._transposed(q_hp, q_off, n_shifts, k, True)

    def search_votes(self, q_hp, q_off):
        """Gpu.search_votes over the shards (include/hpfw_gpu_multi_votes.h): VOTE_DTYPE [n_q]"""
        q = np.ascontiguousarray(q_hp, np.uint64).ravel()
        off = np.ascontiguousarray(q_off, np.int64)
        out = np.zeros(off.size - 1, _lib.VOTE_DTYPE)
        _lib.check(lib().hpfw_gpu_group_search_votes(self._g, _lib._hp(q), _lib._hp(off), off.size - 1, _lib._hp(out)))
        return out

    def extract_windows(self, pcm, win, hop, tempos=None, shifts=None):
        """Gpu.extract_windows with the windows sharded: uint64 [n_w][n_hp], or [n_w][V][n_hp_v] with shifts and / or tempos"""
        pcm = np.ascontiguousarray(pcm, np.int16).ravel()
        shape = _lib.Gpu.from_handle(self.handle(0))._windows_shape(pcm.size, win, hop, tempos, shifts)
        n_w, sets, nhp, t, (keep, sp, ns) = shape
        hp = np.zeros((n_w, sets, nhp), np.uint64)
        _lib.check(lib().hpfw_gpu_group_extract_windows_pcm16(self._g, _lib._hp(pcm), pcm.size, int(win), int(hop),
                                                              None if t is None else _lib._hp(t), 0 if t is None else t.size, sp, ns,
                                                              _lib._hp(hp) if hp.size else None))
        return hp if (tempos is not None or shifts is not None) else hp[:, 0, :]

    def cov_reset(self):
        _lib.check(lib().hpfw_gpu_group_cov_reset(self._g))

    def cov_accumulate(self, pcm):
        pcm = np.ascontiguousarray(pcm, np.int16)
        _lib.check(lib().hpfw_gpu_group_cov_accumulate_pcm16(self._g, _lib._hp(pcm), pcm.shape[1], pcm.shape[0]))

    def learn_filters(self):
        f = np.zeros(64 * 2420, np.float32)
        _lib.check(lib().hpfw_gpu_group_learn_filters(self._g, _lib._hp(f)))
        return f

    # ---- ParallelCollector over the shards ------------------------------------------------------------
    def load(self, cache=""):
        _lib.check(lib().hpfw_gpu_group_load(self._g, cache.encode("utf-8")))

    def save(self, cache=""):
        _lib.check(lib().hpfw_gpu_group_save(self._g, cache.encode("utf-8")))

    def prepare(self, filenames):
        """list of (uint64 array, stem): this call's files in input order, then the older tracks of the cache"""
        raw = [str(f).encode("utf-8") for f in filenames]
        names = (ctypes.c_char_p * len(raw))(*raw)
        got = ctypes.c_int(0)
        res = lib().hpfw_gpu_group_prepare(self._g, names, len(raw), ctypes.byref(got))
        if not res:
            raise _lib.HpfwError("group prepare failed: " + _lib.lib().hpfw_gpu_last_error().decode())
        out = []
        for i in range(got.value):
            a = np.ctypeslib.as_array(res[i].hashprint, shape=(res[i].hp_size,)).astype(np.uint64).copy()
            out.append((a, res[i].filename.decode("utf-8")))
        _lib.lib().prepare_result_free(res, got)
        return out

    def set_resample(self, on=True):
        """files at any rate in [8 000, 192 000] Hz, converted to 44.1 kHz on the GPU (every shard, later ones too)"""
        _lib.check(lib().hpfw_gpu_group_set_resample(self._g, int(bool(on))))

    def calc_hashprint(self, filename):
        size = ctypes.c_int(0)
        hp = lib().hpfw_gpu_group_calc_hashprint(self._g, str(filename).encode("utf-8"), ctypes.byref(size))
        if not hp:
            raise _lib.HpfwError("group calc_hashprint failed: " + _lib.lib().hpfw_gpu_last_error().decode())
        a = np.ctypeslib.as_array(hp, shape=(size.value,)).astype(np.uint64).copy()
        _lib.lib().calc_hashprint_result_free(hp)
        return a
