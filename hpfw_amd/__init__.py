"""hpfw_amd -- MI355X-native (gfx950) hashprint fingerprinting hot path of hpfw.

Only what the path needs: csrc/ (HIP kernels + the C-ABI of include/hpfw_gpu.h), a ctypes
binding, a twin of the reference's Python class (modules/python/pyhpfw/pyhpfw.py) and the
synthetic-audio generator used by tests and bench.py.  No CPU fallback exists.
"""
from ._lib import (Gpu, HpfwError, COMBINER_CONFIG, HIT_DTYPE, SHIFT_HIT_DTYPE, OVERLAP_HIT_DTYPE, DTW_HIT_DTYPE, LOCAL_HIT_DTYPE, PASSAGE_PAIR_DTYPE, VOTE_DTYPE, KERNEL_KINDS, LIB_PATH, lib, merge_topk,  # noqa: F401
                   plan_checksum, plan_cols_tables, plan_bz_shape, supported_length, resample_length, resample_table, wav_read, wav_read_any,
                   wav_write, warp_table)
from .collector import ParallelCollector  # noqa: F401
from .liveid import LiveSongIdentification  # noqa: F401
from .combiner import AudioCombiner  # noqa: F401

__all__ = ["Gpu", "HpfwError", "HIT_DTYPE", "SHIFT_HIT_DTYPE", "OVERLAP_HIT_DTYPE", "DTW_HIT_DTYPE", "LOCAL_HIT_DTYPE", "PASSAGE_PAIR_DTYPE", "VOTE_DTYPE", "KERNEL_KINDS", "LIB_PATH", "lib", "merge_topk",
           "plan_checksum", "plan_cols_tables", "plan_bz_shape", "supported_length", "resample_length", "resample_table", "wav_read", "wav_read_any", "wav_write", "warp_table",
           "ParallelCollector", "LiveSongIdentification",
           "AudioCombiner"]
