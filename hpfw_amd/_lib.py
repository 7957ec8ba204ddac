"""ctypes binding of libhpfw_gpu.so (include/hpfw_gpu.h).

There is no CPU fallback: if the HIP library is missing or fails to load, importing the symbols
raises.  The library is built in-tree by hpfw_amd.build.build() (hipcc --offload-arch=gfx950).
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (HPFW_GPU_LIB: another build of the same library, for diagnosis -- tools/interfere.py)
LIB_PATH = os.environ.get("HPFW_GPU_LIB") or os.path.join(_HERE, "lib", "libhpfw_gpu.so")

HIT_DTYPE = np.dtype([("dist", "<u4"), ("clip", "<u4"), ("offset", "<i4"), ("pad", "<u4")])
# hpfw_shift_hit: a hit of the transposed search and the index of its shift in the caller's list (-1 = none)
SHIFT_HIT_DTYPE = np.dtype([("dist", "<u4"), ("clip", "<u4"), ("offset", "<i4"), ("shift_index", "<i4")])
# hpfw_overlap_hit: a hit of the overlap search; padding: dist = clip = 0xffffffff, lag = overlap = 0
OVERLAP_HIT_DTYPE = np.dtype([("dist", "<u4"), ("clip", "<u4"), ("lag", "<i4"), ("overlap", "<u4")])
# the lags of a (query, clip) pair are scanned in chunks of this many, the first at min_overlap - (the query's length; on the
# matrix cores the longest of its group of 32) -- kOverlapChunk of csrc/kernels.h, for tests that plant matches on the seams
OVERLAP_CHUNK = 1024
# hpfw_dtw_hit: a hit of the warped search; padding: dist = clip = 0xffffffff, start = end = 0
DTW_HIT_DTYPE = np.dtype([("dist", "<u4"), ("clip", "<u4"), ("start", "<i4"), ("end", "<i4")])
DTW_MAX_PATH_CELLS = 1 << 31                             # the path call's cap on K n
# the pairs kernel: a lane holds DTW_STRIP columns, a wave's pass DTW_BLOCK; a wider clip runs in blocks (hpfw_gpu_dtw_geometry)
DTW_STRIP, DTW_BLOCK = 8, 512
# hpfw_local_hit: a hit of the local search; padding: clip = 0xffffffff, the rest 0
LOCAL_HIT_DTYPE = np.dtype([("score", "<i4"), ("clip", "<u4"), ("lag", "<i4"), ("q_start", "<u4"), ("length", "<u4"), ("dist", "<u4")])
# a clip's lags 1 - k .. n - 1 are scanned in chunks of this many, the first at 1 - (the query's length; on the matrix cores the
# longest of its group of 32) -- kLocalChunk of csrc/kernels.h, for tests that plant passages on the seams
LOCAL_CHUNK = 1024
# hpfw_index_move: a piece of the plan of a removal from the index
# hpfw_dup_pair: a pair of the catalogue self-join: clips a < b, position 0 of a on position lag of b
DUP_PAIR_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("dist", "<u4"), ("overlap", "<u4"), ("lag", "<i4"), ("pad", "<u4")])
# hpfw_passage_pair: a pair of the local self-join: clips a < b, a[a_start .. a_start + length) lies on
# b[lag + a_start ..), score = max_rate length - dist
PASSAGE_PAIR_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("score", "<i4"), ("lag", "<i4"), ("a_start", "<u4"), ("length", "<u4"),
                               ("dist", "<u4"), ("pad", "<u4")])
INDEX_MOVE_DTYPE = np.dtype([("dst", "<i8"), ("src", "<i8"), ("len", "<i8"), ("chunk", "<i8"), ("staged", "<i4"), ("pad", "<i4")])
VOTE_DTYPE = np.dtype([("clip", "<u4"), ("pad", "<u4"), ("offset", "<i8"), ("cnt", "<f4"), ("pad2", "<f4")])
# hpfw_combine_result / hpfw_align_hit (AudioCombiner::find and the per-recording alignment peaks)
COMBINE_DTYPE = np.dtype([("rec", "<u4"), ("pad", "<u4"), ("cnt", "<i8"), ("confidence", "<i8"), ("offset", "<i8")])
ALIGN_DTYPE = np.dtype([("rec", "<u4"), ("peak", "<u4"), ("offset", "<i8")])
NO_REC = 0xFFFFFFFF
# hpfw_xcorr_job / hpfw_xcorr_peak: the exact cross-correlation of PCM16
XCORR_JOB_DTYPE = np.dtype([("a_off", "<i8"), ("a_len", "<i8"), ("b_off", "<i8"), ("b_len", "<i8"), ("p", "<i8"), ("q", "<i8"),
                            ("len", "<i8"), ("radius", "<i4"), ("pad", "<i4")])
XCORR_PEAK_DTYPE = np.dtype([("r", "<i8"), ("energy_a", "<i8"), ("energy_b", "<i8"), ("lag", "<i4"), ("pad", "<i4")])
XCORR_MAX_LEN, XCORR_MAX_RADIUS = 1 << 22, 4096
# hpfw_warp_track: a track of the time warp and the mix
WARP_TRACK_DTYPE = np.dtype([("src_off", "<i8"), ("src_len", "<i8"), ("i0", "<i8"), ("f0", "<i8"), ("d", "<i8"), ("gain", "<i4"),
                             ("pad", "<i4")])
# the timeline of a long recording: hpfw_dist_stats, hpfw_window_hit, hpfw_segment
STATS_DTYPE = np.dtype([("sum", "<u8"), ("sum_sq", "<u8"), ("n", "<u4"), ("pad", "<u4")])
WINDOW_HIT_DTYPE = np.dtype([("clip", "<u4"), ("offset", "<i4"), ("variant", "<i4"), ("pad", "<i4"), ("tempo", "<f8"),
                             ("score", "<f8")])
SEGMENT_DTYPE = np.dtype([("clip", "<u4"), ("n_strong", "<i4"), ("first", "<i8"), ("last", "<i8"), ("start", "<i8"),
                          ("end", "<i8"), ("best_window", "<i8"), ("best_score", "<f8"), ("best_tempo", "<f8"),
                          ("best_offset", "<i4"), ("best_variant", "<i4"), ("first_offset", "<i4"), ("pad", "<i4")])
NO_CLIP = 0xFFFFFFFF
# live feeds: hpfw_stream_window
STREAM_WINDOW_DTYPE = np.dtype([("feed", "<i4"), ("pad", "<i4"), ("window", "<i8")])

KERNEL_KINDS = ("fwd_rows", "fwd_cols", "cq_chirpz", "db", "project_mfma", "delta_pack",
                "hamming_scan", "topk", "pcm_pairs", "fwd_span")

# every symbol include/hpfw_gpu.h declares (tests check that the library exports all of them)
EXPORTS = (
    "hpfw_gpu_last_error", "hpfw_gpu_version", "hpfw_gpu_create", "hpfw_gpu_destroy", "hpfw_gpu_device",
    "hpfw_gpu_set_filters", "hpfw_gpu_geometry", "hpfw_gpu_extract_pcm16",
    "hpfw_gpu_extract_pcm16_host", "hpfw_gpu_set_batch", "hpfw_gpu_stage_spectrum",
    "hpfw_gpu_stage_cqmag", "hpfw_gpu_stage_db", "hpfw_gpu_stage_project", "hpfw_gpu_stage_pack",
    "hpfw_gpu_cov_reset", "hpfw_gpu_cov_accumulate_pcm16", "hpfw_gpu_cov_accumulate_pcm16_host",
    "hpfw_gpu_cov_accumulate_db", "hpfw_gpu_cov_get",
    "hpfw_gpu_cov_set", "hpfw_gpu_learn_filters", "hpfw_gpu_host_top_eigenvectors",
    "hpfw_gpu_cov_device", "hpfw_gpu_cov_files", "hpfw_gpu_cov_set_files",
    "hpfw_gpu_index_clear", "hpfw_gpu_index_add", "hpfw_gpu_index_add_device",
    "hpfw_gpu_index_size", "hpfw_gpu_index_set_clip_base", "hpfw_gpu_search_topk_device",
    "hpfw_gpu_search_topk", "hpfw_gpu_merge_topk", "hpfw_gpu_timer_start", "hpfw_gpu_timer_stop",
    "hpfw_gpu_index_get", "hpfw_gpu_extract_db_host", "hpfw_gpu_stage_spectrogram",
    "hpfw_gpu_search_votes", "hpfw_gpu_knn_windows", "hpfw_gpu_supported_length",
    "hpfw_gpu_mel_frames", "hpfw_gpu_mel_spectrogram_pcm16", "hpfw_gpu_mel_spectrogram_pcm16_host",
    "hpfw_gpu_cfg_set_filters", "hpfw_gpu_cfg_hashprints", "hpfw_gpu_mel_hashprints_pcm16_host",
    "hpfw_gpu_cfg_cov_reset", "hpfw_gpu_cfg_cov_accumulate", "hpfw_gpu_cfg_cov_get", "hpfw_gpu_cfg_learn_filters",
    "hpfw_gpu_set_kernel_timing", "hpfw_gpu_get_kernel_timing", "hpfw_gpu_plan_checksum",
    "hpfw_gpu_plan_checksum_ex", "hpfw_gpu_plan_cols_tables", "hpfw_gpu_plan_bz_shape", "hpfw_gpu_set_conventions", "hpfw_gpu_chirpz_table", "hpfw_gpu_debug_workspace", "hpfw_gpu_debug_db_term_sweep", "hpfw_gpu_prepare_length", "hpfw_gpu_set_projection", "hpfw_gpu_get_projection",
    "hpfw_gpu_hashprints_from_db", "hpfw_gpu_stage_delta_q", "hpfw_gpu_debug_q_products",
    "hpfw_gpu_mel_cov_accumulate_pcm16_host", "hpfw_gpu_combiner_clear", "hpfw_gpu_combiner_add",
    "hpfw_gpu_combiner_add_device", "hpfw_gpu_combiner_size", "hpfw_gpu_combiner_get", "hpfw_gpu_combiner_find",
    "hpfw_gpu_combiner_find_device", "hpfw_gpu_combiner_align", "hpfw_gpu_combiner_align_device", "hpfw_gpu_wav_read_pcm16",
    "hpfw_gpu_xcorr_pcm16", "hpfw_gpu_xcorr_pcm16_host", "hpfw_gpu_mel_kept_frames_pcm16_host",
    "hpfw_gpu_wav_read_pcm16_any", "hpfw_gpu_resample_length", "hpfw_gpu_resample_table", "hpfw_gpu_resample_pcm16",
    "hpfw_gpu_resample_pcm16_host", "hpfw_gpu_collector_set_resample",
    "hpfw_gpu_warp_table", "hpfw_gpu_warp_pcm16", "hpfw_gpu_warp_pcm16_host", "hpfw_gpu_mix_pcm16", "hpfw_gpu_mix_pcm16_host",
    "hpfw_gpu_drift_anchors", "hpfw_gpu_drift_fit", "hpfw_gpu_time_map_q40", "hpfw_gpu_wav_write_pcm16",
    "hpfw_gpu_extract_transposed_pcm16", "hpfw_gpu_extract_transposed_pcm16_host", "hpfw_gpu_hashprints_from_db_transposed",
    "hpfw_gpu_search_topk_transposed_device", "hpfw_gpu_search_topk_transposed",
    "hpfw_gpu_tempo_columns", "hpfw_gpu_hashprints_from_db_tempo", "hpfw_gpu_extract_tempo_pcm16",
    "hpfw_gpu_extract_tempo_pcm16_host",
    "hpfw_gpu_search_topk_scored_device", "hpfw_gpu_search_topk_scored", "hpfw_gpu_search_topk_transposed_scored_device",
    "hpfw_gpu_search_topk_transposed_scored", "hpfw_gpu_hit_score", "hpfw_gpu_window_count", "hpfw_gpu_extract_windows_pcm16",
    "hpfw_gpu_extract_windows_pcm16_host", "hpfw_gpu_timeline_segments",
    "hpfw_gpu_merge_topk_device", "hpfw_gpu_sum_stats_device", "hpfw_gpu_get_filters",
    "hpfw_gpu_streams_create", "hpfw_gpu_streams_destroy", "hpfw_gpu_streams_push", "hpfw_gpu_streams_push_device",
    "hpfw_gpu_streams_room", "hpfw_gpu_streams_extract", "hpfw_gpu_streams_extract_host", "hpfw_gpu_streams_reset",
    "hpfw_gpu_streams_info", "hpfw_gpu_streams_create_rates", "hpfw_gpu_streams_rates", "hpfw_gpu_streams_emitted",
    "hpfw_gpu_timeline_tracker_create", "hpfw_gpu_timeline_tracker_destroy",
    "hpfw_gpu_timeline_tracker_push", "hpfw_gpu_timeline_tracker_pop", "hpfw_gpu_timeline_tracker_open",
    "hpfw_gpu_timeline_tracker_finish",
    "hpfw_gpu_search_overlap_device", "hpfw_gpu_search_overlap",
    "hpfw_gpu_search_overlap_scored_device", "hpfw_gpu_search_overlap_scored", "hpfw_gpu_overlap_rate", "hpfw_gpu_overlap_extent",
    "hpfw_gpu_knn_windows_device", "hpfw_gpu_vote_windows_device", "hpfw_gpu_search_votes_device", "hpfw_gpu_merge_knn_device",
    "hpfw_gpu_dtw_pairs_device", "hpfw_gpu_dtw_pairs", "hpfw_gpu_search_dtw_device", "hpfw_gpu_search_dtw",
    "hpfw_gpu_dtw_path_device", "hpfw_gpu_dtw_path", "hpfw_gpu_dtw_geometry",
    "hpfw_gpu_search_local_device", "hpfw_gpu_search_local",
    "hpfw_gpu_index_remove", "hpfw_gpu_index_reserve", "hpfw_gpu_index_capacity", "hpfw_gpu_index_remove_plan",
    "hpfw_gpu_index_remove_geometry",
    "hpfw_gpu_index_selfjoin_device", "hpfw_gpu_index_selfjoin", "hpfw_gpu_selfjoin_geometry",
    "hpfw_gpu_index_join_device", "hpfw_gpu_index_join", "hpfw_gpu_join_plan",
    "hpfw_gpu_index_localjoin_device", "hpfw_gpu_index_localjoin", "hpfw_gpu_localjoin_geometry",
    "hpfw_gpu_search_topk_within_device", "hpfw_gpu_search_topk_within",
    "hpfw_gpu_search_topk_transposed_within_device", "hpfw_gpu_search_topk_transposed_within",
    "par_collector_new", "par_collector_del", "par_collector_prepare",
    "par_collector_calc_hashprint", "par_collector_calc_hashprints", "par_collector_save", "par_collector_load",
    "prepare_result_free", "calc_hashprint_result_free",
)


class HandleConfig(ctypes.Structure):
    """hpfw_handle_config: HashprintHandle<N, SH, FramesContext, T> (hashprint_handle.h:50-64)"""
    _fields_ = [("rows", ctypes.c_int32), ("context", ctypes.c_int32), ("lag", ctypes.c_int32), ("bits", ctypes.c_int32)]


COMBINER_CONFIG = (33, 32, 50, 16)      # combiner.h:12: HashPrint<uint16_t, MelSpectrogram<>, 32, 50>


class TimelineParams(ctypes.Structure):
    """hpfw_timeline_params: min_score is required; tol_cols 0, max_gap -1 and min_windows 0 ask for the defaults"""
    _fields_ = [("min_score", ctypes.c_double), ("hop_cols", ctypes.c_double), ("tol_cols", ctypes.c_double),
                ("win", ctypes.c_int64), ("hop", ctypes.c_int64), ("max_gap", ctypes.c_int32), ("min_windows", ctypes.c_int32)]


class StreamsParams(ctypes.Structure):
    """hpfw_streams_params: capacity 0 asks for 2 win; tempos / shifts NULL and 0 for none"""
    _fields_ = [("n_streams", ctypes.c_int32), ("n_tempos", ctypes.c_int32), ("n_shifts", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("win", ctypes.c_int64), ("hop", ctypes.c_int64), ("capacity", ctypes.c_int64), ("tempos", ctypes.c_void_p),
                ("shifts", ctypes.c_void_p)]


class StreamsInfo(ctypes.Structure):
    _fields_ = [("per_window", ctypes.c_int64), ("win", ctypes.c_int64), ("hop", ctypes.c_int64), ("capacity", ctypes.c_int64),
                ("n_streams", ctypes.c_int32), ("n_sets", ctypes.c_int32)]


class DistStats(ctypes.Structure):
    _fields_ = [("sum", ctypes.c_uint64), ("sum_sq", ctypes.c_uint64), ("n", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


class Geometry(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in
                ("n_samples", "n1", "n2", "kmin", "kmax", "m", "c", "n_frames", "n_hp")]


class FilenameHashprintPair(ctypes.Structure):
    """modules/python/pyhpfw/pyhpfw.py:7-10 of the reference."""
    _fields_ = [("filename", ctypes.c_char_p),
                ("hashprint", ctypes.POINTER(ctypes.c_uint64)),
                ("hp_size", ctypes.c_int)]


class HpfwError(RuntimeError):
    """a failed library call; status is its hpfw_status (HPFW_E_*), None when the failure was not a library status"""

    def __init__(self, msg, status=None):
        super().__init__(msg)
        self.status = status


# hpfw_status values (include/hpfw_gpu.h)
E_INVALID, E_UNSUPPORTED, E_NOFILTERS, E_HIP, E_NOMEM, E_IO = -1, -2, -3, -4, -5, -6
MAX_SHIFTS, MAX_ABS_SHIFT = 64, 120
MAX_TEMPOS, MIN_TEMPO, MAX_TEMPO = 64, 0.5, 2.0


_lib = None


def lib():
    """Load the HIP library, or raise: the product has no other path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HpfwError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                        "g.build()'` (hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = ctypes.CDLL(LIB_PATH)
    vp, i64, i32, u32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_uint32
    L.hpfw_gpu_last_error.restype = ctypes.c_char_p
    L.hpfw_gpu_version.restype = ctypes.c_char_p
    L.hpfw_gpu_create.argtypes = [i32, ctypes.POINTER(vp)]
    L.hpfw_gpu_destroy.argtypes = [vp]
    L.hpfw_gpu_destroy.restype = None
    L.hpfw_gpu_set_filters.argtypes = [vp, vp]
    L.hpfw_gpu_get_filters.argtypes = [vp, vp]
    L.hpfw_gpu_geometry.argtypes = [vp, i64, ctypes.POINTER(Geometry)]
    L.hpfw_gpu_extract_pcm16.argtypes = [vp, vp, i64, i64, vp, vp]
    L.hpfw_gpu_extract_pcm16_host.argtypes = [vp, vp, i64, i64, vp]
    L.hpfw_gpu_set_batch.argtypes = [vp, i32]
    L.hpfw_gpu_stage_spectrum.argtypes = [vp, vp, i64, i64, vp, vp]
    L.hpfw_gpu_stage_cqmag.argtypes = [vp, vp, i64, i64, vp, vp]
    L.hpfw_gpu_stage_db.argtypes = [vp, vp, i64, i64, vp, vp]
    L.hpfw_gpu_stage_project.argtypes = [vp, vp, i64, i64, vp, vp]
    L.hpfw_gpu_stage_pack.argtypes = [vp, vp, i64, i64, vp, vp]
    L.hpfw_gpu_cov_reset.argtypes = [vp]
    L.hpfw_gpu_cov_accumulate_pcm16.argtypes = [vp, vp, i64, i64, vp]
    L.hpfw_gpu_cov_accumulate_pcm16_host.argtypes = [vp, vp, i64, i64]
    L.hpfw_gpu_cov_accumulate_db.argtypes = [vp, vp, i64, i64, vp]
    L.hpfw_gpu_cov_get.argtypes = [vp, vp, ctypes.POINTER(i64)]
    L.hpfw_gpu_cov_set.argtypes = [vp, vp, i64]
    L.hpfw_gpu_learn_filters.argtypes = [vp, vp]
    L.hpfw_gpu_host_top_eigenvectors.argtypes = [vp, i32, i32, vp, vp]
    L.hpfw_gpu_index_clear.argtypes = [vp]
    L.hpfw_gpu_index_add.argtypes = [vp, vp, vp, i64]
    L.hpfw_gpu_index_add_device.argtypes = [vp, vp, vp, i64, vp]
    L.hpfw_gpu_index_size.argtypes = [vp]
    L.hpfw_gpu_index_size.restype = i64
    L.hpfw_gpu_index_set_clip_base.argtypes = [vp, u32]
    L.hpfw_gpu_search_topk_device.argtypes = [vp, vp, vp, i64, i32, vp, vp]
    L.hpfw_gpu_search_topk.argtypes = [vp, vp, vp, i64, i32, vp]
    L.hpfw_gpu_merge_topk.argtypes = [vp, i32, i64, i32, vp]
    L.hpfw_gpu_search_overlap_device.argtypes = [vp, vp, vp, i64, vp, i32, i32, vp, vp]
    L.hpfw_gpu_search_overlap.argtypes = [vp, vp, vp, i64, vp, i32, i32, vp]
    L.hpfw_gpu_search_overlap_scored_device.argtypes = [vp, vp, vp, i64, vp, i32, i32, vp, vp, vp]
    L.hpfw_gpu_search_overlap_scored.argtypes = [vp, vp, vp, i64, vp, i32, i32, vp, vp]
    L.hpfw_gpu_overlap_rate.argtypes = [u32, u32, ctypes.POINTER(u32)]
    L.hpfw_gpu_overlap_extent.argtypes = [i32, i64, i64, i64, i64, i64, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.hpfw_gpu_dtw_pairs_device.argtypes = [vp, vp, vp, i64, vp, i64, vp, vp]
    L.hpfw_gpu_dtw_pairs.argtypes = [vp, vp, vp, i64, vp, i64, vp]
    L.hpfw_gpu_search_dtw_device.argtypes = [vp, vp, vp, i64, i32, i32, vp, vp]
    L.hpfw_gpu_search_dtw.argtypes = [vp, vp, vp, i64, i32, i32, vp]
    L.hpfw_gpu_dtw_path_device.argtypes = [vp, vp, i64, i32, vp, vp, vp]
    L.hpfw_gpu_dtw_path.argtypes = [vp, vp, i64, i32, vp, vp]
    L.hpfw_gpu_dtw_geometry.argtypes = [ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.hpfw_gpu_search_local_device.argtypes = [vp, vp, vp, i64, i32, i32, vp, vp]
    L.hpfw_gpu_search_local.argtypes = [vp, vp, vp, i64, i32, i32, vp]
    L.hpfw_gpu_index_remove.argtypes = [vp, vp, i64, vp]
    L.hpfw_gpu_index_reserve.argtypes = [vp, i64]
    L.hpfw_gpu_index_capacity.argtypes = [vp]
    L.hpfw_gpu_index_capacity.restype = i64
    L.hpfw_gpu_index_remove_plan.argtypes = [vp, i64, vp, i64, i64, vp, vp, i64, ctypes.POINTER(i64)]
    L.hpfw_gpu_index_remove_geometry.argtypes = [ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.hpfw_gpu_index_selfjoin_device.argtypes = [vp, i32, i32, i32, vp, i64, vp, vp]
    L.hpfw_gpu_index_selfjoin.argtypes = [vp, i32, i32, i32, vp, i64, ctypes.POINTER(i64)]
    L.hpfw_gpu_selfjoin_geometry.argtypes = [ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.hpfw_gpu_index_localjoin_device.argtypes = [vp, i32, i32, vp, i64, vp, vp]
    L.hpfw_gpu_index_localjoin.argtypes = [vp, i32, i32, vp, i64, ctypes.POINTER(i64)]
    L.hpfw_gpu_localjoin_geometry.argtypes = [ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.hpfw_gpu_index_join_device.argtypes = [vp, vp, vp, i64, i32, i32, i32, i32, vp, i64, vp, vp]
    L.hpfw_gpu_index_join.argtypes = [vp, vp, vp, i64, i32, i32, i32, i32, vp, i64, ctypes.POINTER(i64)]
    L.hpfw_gpu_join_plan.argtypes = [i64, i64, i32, i64, i64, vp]
    L.hpfw_gpu_timer_start.argtypes = [vp, vp]
    L.hpfw_gpu_timer_stop.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_float)]
    L.hpfw_gpu_stage_spectrogram.argtypes = [vp, vp, i64, i64, vp, vp]
    L.hpfw_gpu_mel_frames.argtypes = [i64]
    L.hpfw_gpu_mel_frames.restype = i64
    L.hpfw_gpu_mel_spectrogram_pcm16.argtypes = [vp, vp, i64, i64, vp, vp, vp]
    L.hpfw_gpu_mel_spectrogram_pcm16_host.argtypes = [vp, vp, i64, i64, vp, vp]
    L.hpfw_gpu_cfg_set_filters.argtypes = [vp, ctypes.POINTER(HandleConfig), vp]
    L.hpfw_gpu_cfg_hashprints.argtypes = [vp, ctypes.POINTER(HandleConfig), vp, vp, i64, i64, vp, i64, vp, vp]
    L.hpfw_gpu_mel_hashprints_pcm16_host.argtypes = [vp, vp, i64, i64, vp, i64, vp]
    L.hpfw_gpu_cfg_cov_reset.argtypes = [vp, ctypes.POINTER(HandleConfig)]
    L.hpfw_gpu_cfg_cov_accumulate.argtypes = [vp, ctypes.POINTER(HandleConfig), vp, vp, i64, i64, vp]
    L.hpfw_gpu_cfg_cov_get.argtypes = [vp, ctypes.POINTER(HandleConfig), vp, ctypes.POINTER(i64)]
    L.hpfw_gpu_cfg_learn_filters.argtypes = [vp, ctypes.POINTER(HandleConfig), vp]
    L.hpfw_gpu_supported_length.argtypes = [i64]
    L.hpfw_gpu_supported_length.restype = i64
    L.hpfw_gpu_search_votes.argtypes = [vp, vp, vp, i64, vp]
    L.hpfw_gpu_knn_windows.argtypes = [vp, vp, vp, i64, vp, i64]
    L.hpfw_gpu_knn_windows_device.argtypes = [vp, vp, vp, i64, vp, i64, vp]
    L.hpfw_gpu_vote_windows_device.argtypes = [vp, vp, vp, i64, vp, i64, u32, vp, vp]
    L.hpfw_gpu_search_votes_device.argtypes = [vp, vp, vp, i64, vp, vp]
    L.hpfw_gpu_merge_knn_device.argtypes = [vp, vp, vp, i32, i64, vp, vp]
    L.hpfw_gpu_index_get.argtypes = [vp, vp, vp, ctypes.c_int64]
    L.hpfw_gpu_extract_db_host.argtypes = [vp, vp, i32, i32, vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    L.hpfw_gpu_set_kernel_timing.argtypes = [vp, i32]
    L.hpfw_gpu_get_kernel_timing.argtypes = [vp, vp, vp, vp, ctypes.POINTER(i32)]
    L.hpfw_gpu_plan_checksum.argtypes = [i64, vp]
    L.hpfw_gpu_plan_checksum_ex.argtypes = [i64, i32, u32, vp]
    L.hpfw_gpu_plan_cols_tables.argtypes = [i64, vp, vp, vp, vp, vp]
    L.hpfw_gpu_plan_bz_shape.argtypes = [i64, i32, vp]
    L.hpfw_gpu_chirpz_table.argtypes = [vp, i64, i32, vp, i64, vp]
    L.hpfw_gpu_debug_workspace.argtypes = [vp, i32, vp, vp]
    L.hpfw_gpu_debug_db_term_sweep.argtypes = [u32, ctypes.c_uint64, vp]
    L.hpfw_gpu_prepare_length.argtypes = [vp, i64]
    L.hpfw_gpu_set_projection.argtypes = [vp, i32]
    L.hpfw_gpu_get_projection.argtypes = [vp]
    L.hpfw_gpu_hashprints_from_db.argtypes = [vp, vp, i64, i64, vp, vp]
    L.hpfw_gpu_stage_delta_q.argtypes = [vp, vp, i64, i64, vp, vp, vp]
    L.hpfw_gpu_debug_q_products.argtypes = [vp, vp, vp, vp]
    L.hpfw_gpu_set_conventions.argtypes = [vp, u32]
    L.hpfw_gpu_mel_cov_accumulate_pcm16_host.argtypes = [vp, vp, i64, i64]
    L.hpfw_gpu_combiner_clear.argtypes = [vp]
    L.hpfw_gpu_combiner_add.argtypes = [vp, vp, vp, i64]
    L.hpfw_gpu_combiner_add_device.argtypes = [vp, vp, vp, i64, vp]
    L.hpfw_gpu_combiner_size.argtypes = [vp]
    L.hpfw_gpu_combiner_size.restype = i64
    L.hpfw_gpu_combiner_get.argtypes = [vp, vp, vp, vp, i64]
    L.hpfw_gpu_combiner_find.argtypes = [vp, vp, vp, vp, i64, vp]
    L.hpfw_gpu_combiner_find_device.argtypes = [vp, vp, vp, vp, i64, vp, vp]
    L.hpfw_gpu_combiner_align.argtypes = [vp, vp, vp, vp, i64, i32, vp]
    L.hpfw_gpu_combiner_align_device.argtypes = [vp, vp, vp, vp, i64, i32, vp, vp]
    L.hpfw_gpu_xcorr_pcm16.argtypes = [vp, vp, vp, i64, vp, vp, vp]
    L.hpfw_gpu_xcorr_pcm16_host.argtypes = [vp, vp, i64, vp, i64, vp, vp]
    L.hpfw_gpu_mel_kept_frames_pcm16_host.argtypes = [vp, vp, i64, i64, vp, i64, vp]
    L.hpfw_gpu_wav_read_pcm16.argtypes = [ctypes.c_char_p, vp, i64, ctypes.POINTER(i64)]
    L.hpfw_gpu_wav_read_pcm16_any.argtypes = [ctypes.c_char_p, vp, i64, ctypes.POINTER(i64), ctypes.POINTER(i32)]
    L.hpfw_gpu_resample_length.argtypes = [i64, i32, ctypes.POINTER(i64)]
    L.hpfw_gpu_resample_table.argtypes = [i32, vp, i64, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.hpfw_gpu_resample_pcm16.argtypes = [vp, vp, i64, i64, i32, vp, vp]
    L.hpfw_gpu_resample_pcm16_host.argtypes = [vp, vp, i64, i64, i32, vp]
    L.hpfw_gpu_collector_set_resample.argtypes = [vp, i32]
    L.hpfw_gpu_warp_table.argtypes = [vp, i64, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.hpfw_gpu_warp_pcm16.argtypes = [vp, vp, i64, vp, i64, i64, i64, vp, vp]
    L.hpfw_gpu_warp_pcm16_host.argtypes = [vp, vp, i64, vp, i64, i64, i64, vp]
    L.hpfw_gpu_mix_pcm16.argtypes = [vp, vp, i64, vp, i64, i64, i64, vp, vp]
    L.hpfw_gpu_mix_pcm16_host.argtypes = [vp, vp, i64, vp, i64, i64, i64, vp]
    L.hpfw_gpu_drift_anchors.argtypes = [i64, i64, i64, i64, i64, i64, vp, i64, ctypes.POINTER(i32), ctypes.POINTER(i32),
                                         ctypes.POINTER(i64)]
    L.hpfw_gpu_drift_fit.argtypes = [vp, vp, i32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                     ctypes.POINTER(ctypes.c_double)]
    L.hpfw_gpu_time_map_q40.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.hpfw_gpu_wav_write_pcm16.argtypes = [ctypes.c_char_p, vp, i64, i32]
    L.hpfw_gpu_extract_transposed_pcm16.argtypes = [vp, vp, i64, i64, vp, i32, vp, vp]
    L.hpfw_gpu_extract_transposed_pcm16_host.argtypes = [vp, vp, i64, i64, vp, i32, vp]
    L.hpfw_gpu_hashprints_from_db_transposed.argtypes = [vp, vp, i64, i64, vp, i32, vp, vp]
    L.hpfw_gpu_search_topk_transposed_device.argtypes = [vp, vp, vp, i64, i32, i32, vp, vp]
    L.hpfw_gpu_search_topk_transposed.argtypes = [vp, vp, vp, i64, i32, i32, vp]
    L.hpfw_gpu_tempo_columns.argtypes = [i64, vp, i32, ctypes.POINTER(i64)]
    L.hpfw_gpu_hashprints_from_db_tempo.argtypes = [vp, vp, i64, i64, vp, i32, vp, i32, vp, vp]
    L.hpfw_gpu_extract_tempo_pcm16.argtypes = [vp, vp, i64, i64, vp, i32, vp, i32, vp, vp]
    L.hpfw_gpu_extract_tempo_pcm16_host.argtypes = [vp, vp, i64, i64, vp, i32, vp, i32, vp]
    L.hpfw_gpu_search_topk_scored_device.argtypes = [vp, vp, vp, i64, i32, vp, vp, vp]
    L.hpfw_gpu_search_topk_scored.argtypes = [vp, vp, vp, i64, i32, vp, vp]
    L.hpfw_gpu_search_topk_transposed_scored_device.argtypes = [vp, vp, vp, i64, i32, i32, vp, vp, vp]
    L.hpfw_gpu_search_topk_transposed_scored.argtypes = [vp, vp, vp, i64, i32, i32, vp, vp]
    L.hpfw_gpu_search_topk_within_device.argtypes = [vp, vp, vp, i64, i32, vp, i64, vp, vp, vp, vp, vp]
    L.hpfw_gpu_search_topk_within.argtypes = [vp, vp, vp, i64, i32, vp, i64, vp, vp, vp, vp]
    L.hpfw_gpu_search_topk_transposed_within_device.argtypes = [vp, vp, vp, i64, i32, i32, vp, i64, vp, vp, vp, vp, vp]
    L.hpfw_gpu_search_topk_transposed_within.argtypes = [vp, vp, vp, i64, i32, i32, vp, i64, vp, vp, vp, vp]
    L.hpfw_gpu_hit_score.argtypes = [u32, i32, ctypes.POINTER(DistStats), ctypes.POINTER(ctypes.c_double)]
    L.hpfw_gpu_window_count.argtypes = [i64, i64, i64, ctypes.POINTER(i64)]
    L.hpfw_gpu_extract_windows_pcm16.argtypes = [vp, vp, i64, i64, i64, vp, i32, vp, i32, vp, vp]
    L.hpfw_gpu_extract_windows_pcm16_host.argtypes = [vp, vp, i64, i64, i64, vp, i32, vp, i32, vp]
    L.hpfw_gpu_timeline_segments.argtypes = [vp, i64, ctypes.POINTER(TimelineParams), vp, i64, ctypes.POINTER(i64)]
    L.hpfw_gpu_merge_topk_device.argtypes = [vp, vp, i32, i64, i32, vp, vp]
    L.hpfw_gpu_sum_stats_device.argtypes = [vp, vp, i32, i64, vp, vp]
    L.hpfw_gpu_streams_create.argtypes = [vp, ctypes.POINTER(StreamsParams), ctypes.POINTER(vp)]
    L.hpfw_gpu_streams_create_rates.argtypes = [vp, ctypes.POINTER(StreamsParams), vp, ctypes.POINTER(vp)]
    L.hpfw_gpu_streams_rates.argtypes = [vp, vp, vp]
    L.hpfw_gpu_streams_emitted.argtypes = [i64, i32, ctypes.POINTER(i64)]
    L.hpfw_gpu_streams_destroy.argtypes = [vp]
    L.hpfw_gpu_streams_destroy.restype = None
    L.hpfw_gpu_streams_push.argtypes = [vp, vp, vp, ctypes.POINTER(i64)]
    L.hpfw_gpu_streams_push_device.argtypes = [vp, vp, vp, ctypes.POINTER(i64), vp]
    L.hpfw_gpu_streams_room.argtypes = [vp, vp]
    L.hpfw_gpu_streams_extract.argtypes = [vp, i64, vp, vp, vp, ctypes.POINTER(i64), vp]
    L.hpfw_gpu_streams_extract_host.argtypes = [vp, i64, vp, vp, vp, ctypes.POINTER(i64)]
    L.hpfw_gpu_streams_reset.argtypes = [vp, i32]
    L.hpfw_gpu_streams_info.argtypes = [vp, ctypes.POINTER(StreamsInfo), vp, vp]
    L.hpfw_gpu_timeline_tracker_create.argtypes = [ctypes.POINTER(TimelineParams), ctypes.POINTER(vp)]
    L.hpfw_gpu_timeline_tracker_destroy.argtypes = [vp]
    L.hpfw_gpu_timeline_tracker_destroy.restype = None
    L.hpfw_gpu_timeline_tracker_push.argtypes = [vp, vp, i64]
    L.hpfw_gpu_timeline_tracker_pop.argtypes = [vp, vp, i64, ctypes.POINTER(i64)]
    L.hpfw_gpu_timeline_tracker_open.argtypes = [vp, vp, ctypes.POINTER(i32)]
    L.hpfw_gpu_timeline_tracker_finish.argtypes = [vp]
    L.par_collector_new.restype = vp
    L.par_collector_del.argtypes = [vp]
    L.par_collector_del.restype = None
    L.par_collector_prepare.restype = ctypes.POINTER(FilenameHashprintPair)
    L.par_collector_prepare.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), i32, ctypes.POINTER(i32)]
    L.par_collector_calc_hashprints.restype = ctypes.POINTER(FilenameHashprintPair)
    L.par_collector_calc_hashprints.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), i32]
    L.par_collector_calc_hashprint.restype = ctypes.POINTER(ctypes.c_uint64)
    L.par_collector_calc_hashprint.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(i32)]
    L.par_collector_load.argtypes = [vp, ctypes.c_char_p]
    L.par_collector_load.restype = None
    L.par_collector_save.argtypes = [vp, ctypes.c_char_p]
    L.par_collector_save.restype = None
    L.prepare_result_free.argtypes = [vp, i32]
    L.prepare_result_free.restype = None
    L.calc_hashprint_result_free.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    L.calc_hashprint_result_free.restype = None
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise HpfwError(f"hpfw_gpu error {rc}: {lib().hpfw_gpu_last_error().decode()}", rc)


def check_shifts(shifts):
    """the bin shifts of a transposed query as the library accepts them: 1 to 64 distinct integers, |s| <= 120
    (ValueError otherwise); returned as a list of int"""
    out = [int(s) for s in shifts]
    if not 1 <= len(out) <= MAX_SHIFTS:
        raise ValueError(f"shifts: 1 to {MAX_SHIFTS} values, got {len(out)}")
    if any(abs(s) > MAX_ABS_SHIFT for s in out):
        raise ValueError(f"shifts: |s| <= {MAX_ABS_SHIFT}, got {out}")
    if len(set(out)) != len(out):
        raise ValueError(f"shifts: values must be distinct, got {out}")
    return out


def tempo_step(rho):
    """rint(65536 / rho) of the float32 tempo rho: its step along the source in sixteenths of a column"""
    return int(np.rint(65536.0 / float(np.float32(rho))))


def check_tempos(tempos, n_shifts=0):
    """the tempo factors of a tempo query as the library accepts them: 1 to 64 finite values in [0.5, 2] with distinct
    steps, at most 64 variants together with n_shifts shifts (ValueError otherwise); returned as a list of float"""
    out = [float(t) for t in np.asarray(tempos, np.float32).ravel()] if tempos is not None else []
    if not 1 <= len(out) <= MAX_TEMPOS:
        raise ValueError(f"tempos: 1 to {MAX_TEMPOS} values, got {len(out)}")
    if not all(MIN_TEMPO <= t <= MAX_TEMPO for t in out):           # (NaN fails the comparison)
        raise ValueError(f"tempos: finite values in [{MIN_TEMPO}, {MAX_TEMPO}], got {out}")
    if len({tempo_step(t) for t in out}) != len(out):
        raise ValueError(f"tempos: values must have distinct steps rint(65536 / tempo), got {out}")
    if len(out) * max(int(n_shifts), 1) > MAX_SHIFTS:
        raise ValueError(f"tempos x shifts: at most {MAX_SHIFTS} variants, got {len(out)} x {n_shifts}")
    return out


def tempo_columns(c, tempos):
    """columns c_t every tempo variant of a clip of c spectrogram columns is cut to (hpfw_gpu_tempo_columns)"""
    t = np.ascontiguousarray(tempos, np.float32).ravel()
    out = ctypes.c_int64()
    check(lib().hpfw_gpu_tempo_columns(int(c), _hp(t), t.size, ctypes.byref(out)))
    return out.value


def window_count(n_total, win, hop):
    """windows [w hop, w hop + win) of a recording of n_total samples (hpfw_gpu_window_count)"""
    n = ctypes.c_int64()
    check(lib().hpfw_gpu_window_count(int(n_total), int(win), int(hop), ctypes.byref(n)))
    return n.value


def hit_score(dist, counted, stats):
    """(mean of the other counted clips' distances - dist) / their standard deviation, from a STATS_DTYPE row
    (hpfw_gpu_hit_score); NaN when the clip is not counted, n < 3 or the variance is 0"""
    st = DistStats(int(stats["sum"]), int(stats["sum_sq"]), int(stats["n"]), 0)
    out = ctypes.c_double()
    check(lib().hpfw_gpu_hit_score(int(dist), int(bool(counted)), ctypes.byref(st), ctypes.byref(out)))
    return out.value


OVERLAP_RATE_BITS = 10                                   # HPFW_OVERLAP_RATE_BITS


def join_plan(n_clips, n_x, among_new, group0, n_groups):
    """uint32 [n_groups + 1]: the numbering of the (row group, external) items of a pass of the join over the row groups
    group0 .. group0 + n_groups - 1 (hpfw_gpu_join_plan): item pair_first[i] + j is (group0 + i, b = max(n_clips, 32 (group0 + i) +
    1) + j)"""
    pair_first = np.zeros(int(n_groups) + 1, np.uint32)
    check(lib().hpfw_gpu_join_plan(int(n_clips), int(n_x), int(among_new), int(group0), int(n_groups), _hp(pair_first)))
    return pair_first


def selfjoin_geometry():
    """(slice, chunk) of the catalogue self-join: positions of a staged per pass, lags of b per workgroup pass
    (hpfw_gpu_selfjoin_geometry)"""
    sl, ch = ctypes.c_int32(0), ctypes.c_int32(0)
    check(lib().hpfw_gpu_selfjoin_geometry(ctypes.byref(sl), ctypes.byref(ch)))
    return int(sl.value), int(ch.value)


def localjoin_geometry():
    """(slice, chunk) of the local self-join: positions of a staged per pass, lags of b per workgroup pass; a pair's chunks
    begin at ceil(min_score / max_rate) - (the longest a of the row group) (hpfw_gpu_localjoin_geometry)"""
    sl, ch = ctypes.c_int32(0), ctypes.c_int32(0)
    check(lib().hpfw_gpu_localjoin_geometry(ctypes.byref(sl), ctypes.byref(ch)))
    return int(sl.value), int(ch.value)


def overlap_rate(dist, overlap):
    """floor(dist 2^10 / overlap): the integer the scored overlap search takes its moments of (hpfw_gpu_overlap_rate)"""
    out = ctypes.c_uint32()
    check(lib().hpfw_gpu_overlap_rate(int(dist), int(overlap), ctypes.byref(out)))
    return out.value


def overlap_extent(lag, n_clip, k_q, span, win, m):
    """(a, b): the samples [a, b) of a window of k_q hashprints that lie on the clip of n_clip hashprints it was found in at
    lag `lag`; span: columns per hashprint (c - n_hp + 1 of the window's geometry), m: the geometry's m (hpfw_gpu_overlap_extent)"""
    a, b = ctypes.c_int64(), ctypes.c_int64()
    check(lib().hpfw_gpu_overlap_extent(int(lag), int(n_clip), int(k_q), int(span), int(win), int(m), ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def timeline_segments(windows, min_score, hop_cols, win, hop, tol_cols=None, max_gap=1, min_windows=1):
    """WINDOW_HIT_DTYPE [n_w] -> SEGMENT_DTYPE [n_seg] by the rule of include/hpfw_gpu.h (hpfw_gpu_timeline_segments);
    tol_cols None = the default max(2, 0.08 hop_cols)"""
    w = np.ascontiguousarray(windows, WINDOW_HIT_DTYPE).ravel()
    p = _timeline_params(min_score, hop_cols, win, hop, tol_cols, max_gap, min_windows)
    out = np.zeros(max(w.size, 1), SEGMENT_DTYPE)
    n = ctypes.c_int64()
    check(lib().hpfw_gpu_timeline_segments(_hp(w) if w.size else None, w.size, ctypes.byref(p), _hp(out), out.size, ctypes.byref(n)))
    return out[:n.value].copy()


def _timeline_params(min_score, hop_cols, win, hop, tol_cols, max_gap, min_windows):
    if tol_cols is not None and not tol_cols > 0:
        raise ValueError("tol_cols must be positive")
    if max_gap < 0 or min_windows < 1:
        raise ValueError("max_gap >= 0 and min_windows >= 1")
    return TimelineParams(float(min_score), float(hop_cols), 0.0 if tol_cols is None else float(tol_cols), int(win), int(hop),
                          int(max_gap), int(min_windows))


class TimelineTracker:
    """hpfw_gpu_timeline_segments as the windows arrive (hpfw_timeline_tracker): push() window rows,
    pop() the segments nothing can continue any more, open() the one in progress, finish() at the end of the feed"""

    def __init__(self, min_score, hop_cols, win, hop, tol_cols=None, max_gap=1, min_windows=1):
        p = _timeline_params(min_score, hop_cols, win, hop, tol_cols, max_gap, min_windows)
        self._t = ctypes.c_void_p()
        check(lib().hpfw_gpu_timeline_tracker_create(ctypes.byref(p), ctypes.byref(self._t)))

    def push(self, windows):
        w = np.ascontiguousarray(windows, WINDOW_HIT_DTYPE).ravel()
        check(lib().hpfw_gpu_timeline_tracker_push(self._t, _hp(w) if w.size else None, w.size))

    def pop(self, cap=None):
        """the closed segments not yet popped, oldest first (at most cap of them): SEGMENT_DTYPE [n]"""
        got, left = [], (None if cap is None else int(cap))
        chunk = np.zeros(16, SEGMENT_DTYPE)
        n = ctypes.c_int64()
        while left is None or left > 0:
            want = chunk.size if left is None else min(chunk.size, left)
            check(lib().hpfw_gpu_timeline_tracker_pop(self._t, _hp(chunk), want, ctypes.byref(n)))
            got.append(chunk[:n.value].copy())
            left = None if left is None else left - n.value
            if n.value < want:
                break
        return np.concatenate(got) if got else np.zeros(0, SEGMENT_DTYPE)

    def open(self):
        """the segment in progress as it would close now (a SEGMENT_DTYPE record), or None"""
        cur = np.zeros(1, SEGMENT_DTYPE)
        has = ctypes.c_int(0)
        check(lib().hpfw_gpu_timeline_tracker_open(self._t, _hp(cur), ctypes.byref(has)))
        return cur[0] if has.value else None

    def finish(self):
        check(lib().hpfw_gpu_timeline_tracker_finish(self._t))

    def close(self):
        if getattr(self, "_t", None):
            lib().hpfw_gpu_timeline_tracker_destroy(self._t)
            self._t = None

    def __del__(self):
        try:
            self.close()
        except Exception:        # interpreter teardown
            pass


def _shift_arg(shifts):
    """(array kept alive, pointer, count) of an optional shift list: None is (NULL, 0)"""
    if shifts is None:
        return None, None, 0
    sh = np.ascontiguousarray(shifts, np.int32).ravel()
    return sh, _hp(sh), sh.size


def _hp(a):
    """host pointer of a contiguous numpy array"""
    return a.ctypes.data_as(ctypes.c_void_p)


def _within_sets(set_off, set_clips, q_set, n_q):
    """the set arguments of the searches within sets as the C ABI takes them: int64 offsets, int32 clips, int32 [n_q] sets"""
    so = np.ascontiguousarray(set_off, np.int64).ravel()
    sc = np.ascontiguousarray(set_clips, np.int32).ravel()
    qs = np.ascontiguousarray(q_set, np.int32).ravel()
    if so.size < 1:
        raise ValueError("set_off must hold n_sets + 1 offsets")
    if qs.size != n_q:
        raise ValueError(f"q_set must hold one entry per query ({n_q}), got {qs.size}")
    if sc.size < so[-1]:
        raise ValueError("set_clips is shorter than set_off[n_sets]")
    return so, sc, qs


class Gpu:
    """One handle = one MI355X device.  Device-pointer methods take integers (tensor.data_ptr())."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        check(lib().hpfw_gpu_create(int(device), ctypes.byref(self._h)))

    @classmethod
    def from_handle(cls, handle):
        """a view of a handle somebody else owns (a shard of hpfw_amd.multi.GpuGroup): close() does not destroy it"""
        g = cls.__new__(cls)
        g._h = ctypes.c_void_p(handle) if not isinstance(handle, ctypes.c_void_p) else handle
        g._borrowed = True
        return g

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):
                lib().hpfw_gpu_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:        # interpreter teardown: the module globals may already be gone
            pass

    # ---- configuration -------------------------------------------------------------------
    def set_filters(self, filters_colmajor):
        f = np.ascontiguousarray(filters_colmajor, np.float32).ravel()
        if f.size != 64 * 2420:
            raise ValueError("filters must hold 64 x 2420 floats (column-major)")
        check(lib().hpfw_gpu_set_filters(self._h, _hp(f)))

    def get_filters(self):
        """the filters the handle holds, float32 [64 * 2420] column-major (HPFW_E_NOFILTERS when none)"""
        f = np.zeros(64 * 2420, np.float32)
        check(lib().hpfw_gpu_get_filters(self._h, _hp(f)))
        return f

    def geometry(self, n_samples):
        g = Geometry()
        check(lib().hpfw_gpu_geometry(self._h, int(n_samples), ctypes.byref(g)))
        return g

    def set_conventions(self, flags):
        """HPFW_CONV_* bits: essentia conventions that cannot be checked offline (include/hpfw_gpu.h)"""
        check(lib().hpfw_gpu_set_conventions(self._h, int(flags)))

    def set_batch(self, clips_per_pass):
        check(lib().hpfw_gpu_set_batch(self._h, int(clips_per_pass)))

    # ---- extraction ----------------------------------------------------------------------
    def extract_dev(self, d_pcm, n_samples, n_clips, d_hp, stream=0):
        check(lib().hpfw_gpu_extract_pcm16(self._h, d_pcm, n_samples, n_clips, d_hp, stream))

    def extract(self, pcm):
        """pcm: int16 [n_clips][n_samples] (host) -> uint64 [n_clips][n_hp]"""
        pcm = np.ascontiguousarray(pcm, np.int16)
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        g = self.geometry(pcm.shape[1])
        hp = np.zeros((pcm.shape[0], g.n_hp), np.uint64)
        check(lib().hpfw_gpu_extract_pcm16_host(self._h, _hp(pcm), pcm.shape[1], pcm.shape[0], _hp(hp)))
        return hp

    # ---- transposed queries -------------------------------------------
    def extract_transposed(self, pcm, shifts):
        """pcm int16 [n] or [n_clips][n] -> uint64 [n_clips][len(shifts)][n_hp]: shift s hashes the dB spectrogram moved by
        s bins (row b = row b + s, -80 dB outside); 24 bins per octave, so t semitones up is s = 2t"""
        pcm = np.ascontiguousarray(pcm, np.int16)
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        sh = np.ascontiguousarray(shifts, np.int32).ravel()
        g = self.geometry(pcm.shape[1])
        hp = np.zeros((pcm.shape[0], sh.size, max(g.n_hp, 0)), np.uint64)
        check(lib().hpfw_gpu_extract_transposed_pcm16_host(self._h, _hp(pcm), pcm.shape[1], pcm.shape[0], _hp(sh), sh.size,
                                                           _hp(hp)))
        return hp

    def extract_transposed_dev(self, d_pcm, n_samples, n_clips, shifts, d_hp, stream=0):
        sh = np.ascontiguousarray(shifts, np.int32).ravel()
        check(lib().hpfw_gpu_extract_transposed_pcm16(self._h, d_pcm, n_samples, n_clips, _hp(sh), sh.size, d_hp, stream))

    def hashprints_from_db_transposed_dev(self, d_db, n_clips, c, shifts, d_hp, stream=0):
        sh = np.ascontiguousarray(shifts, np.int32).ravel()
        check(lib().hpfw_gpu_hashprints_from_db_transposed(self._h, d_db, n_clips, c, _hp(sh), sh.size, d_hp, stream))

    # ---- queries at another tempo -------------------------------------
    def extract_tempo(self, pcm, tempos, shifts=None):
        """pcm int16 [n] or [n_clips][n] -> uint64 [n_clips][V][n_hp_t], V = len(tempos) max(len(shifts), 1): variant
        v = j max(len(shifts), 1) + i hashes the dB spectrogram rescaled to tempo j (column k shows query time k / tempo)
        and moved by shift i; every variant is cut to tempo_columns(c, tempos) columns"""
        pcm = np.ascontiguousarray(pcm, np.int16)
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        t = np.ascontiguousarray(tempos, np.float32).ravel()
        keep, sp, ns = _shift_arg(shifts)
        check_tempos(t, ns)
        g = self.geometry(pcm.shape[1])
        nhp = tempo_columns(g.c, t) - 99
        hp = np.zeros((pcm.shape[0], t.size * max(ns, 1), max(nhp, 0)), np.uint64)
        check(lib().hpfw_gpu_extract_tempo_pcm16_host(self._h, _hp(pcm), pcm.shape[1], pcm.shape[0], _hp(t), t.size, sp, ns,
                                                      _hp(hp)))
        return hp

    def extract_tempo_dev(self, d_pcm, n_samples, n_clips, tempos, d_hp, shifts=None, stream=0):
        t = np.ascontiguousarray(tempos, np.float32).ravel()
        keep, sp, ns = _shift_arg(shifts)
        check(lib().hpfw_gpu_extract_tempo_pcm16(self._h, d_pcm, n_samples, n_clips, _hp(t), t.size, sp, ns, d_hp, stream))

    def hashprints_from_db_tempo_dev(self, d_db, n_clips, c, tempos, d_hp, shifts=None, stream=0):
        t = np.ascontiguousarray(tempos, np.float32).ravel()
        keep, sp, ns = _shift_arg(shifts)
        check(lib().hpfw_gpu_hashprints_from_db_tempo(self._h, d_db, n_clips, c, _hp(t), t.size, sp, ns, d_hp, stream))

    # ---- windows of one recording ---------------------------------------
    def _windows_shape(self, n_total, win, hop, tempos, shifts):
        """(n_w, sets per window, hashprints per set, tempo array, shift tuple) of extract_windows"""
        t = None if tempos is None else np.ascontiguousarray(tempos, np.float32).ravel()
        sh = _shift_arg(shifts)
        n_w = window_count(n_total, win, hop)
        g = self.geometry(win)
        nhp = g.n_hp if t is None else tempo_columns(g.c, t) - 99
        return n_w, (1 if t is None else t.size) * max(sh[2], 1), max(int(nhp), 0), t, sh

    def extract_windows(self, pcm, win, hop, tempos=None, shifts=None):
        """pcm int16 [n_total] (host), ONE recording of any length -> uint64 [n_w][n_hp] of windows [w hop, w hop + win), or
        [n_w][V][n_hp_v] with shifts and / or tempos (as extract_transposed / extract_tempo on the windows copied out)"""
        pcm = np.ascontiguousarray(pcm, np.int16).ravel()
        n_w, sets, nhp, t, (keep, sp, ns) = self._windows_shape(pcm.size, win, hop, tempos, shifts)
        hp = np.zeros((n_w, sets, nhp), np.uint64)
        check(lib().hpfw_gpu_extract_windows_pcm16_host(self._h, _hp(pcm), pcm.size, int(win), int(hop),
                                                        None if t is None else _hp(t), 0 if t is None else t.size, sp, ns,
                                                        _hp(hp) if hp.size else None))
        return hp if (tempos is not None or shifts is not None) else hp[:, 0, :]

    def extract_windows_dev(self, d_pcm, n_total, win, hop, d_hp, tempos=None, shifts=None, stream=0):
        t = None if tempos is None else np.ascontiguousarray(tempos, np.float32).ravel()
        keep, sp, ns = _shift_arg(shifts)
        check(lib().hpfw_gpu_extract_windows_pcm16(self._h, d_pcm, int(n_total), int(win), int(hop),
                                                   None if t is None else _hp(t), 0 if t is None else t.size, sp, ns, d_hp, stream))

    hit_score = staticmethod(hit_score)
    timeline_segments = staticmethod(timeline_segments)

    def streams(self, n_streams, win, hop, capacity=0, tempos=None, shifts=None, rates=None):
        """a set of live feeds on this handle: GpuStreams.  rates: the feeds' sample rate, one int for
        all or one per feed (None: 44 100 Hz); win, hop and capacity are in 44.1 kHz samples whatever the rates"""
        return GpuStreams(self, n_streams, win, hop, capacity, tempos, shifts, rates)

    # ---- sample-rate conversion to 44.1 kHz (k_resample.hip) --------------------------------
    def resample_dev(self, d_in, n_in, n_clips, rate, d_out, stream=0):
        """d_in int16 [n_clips][n_in] at `rate` -> d_out int16 [n_clips][resample_length(n_in, rate)] (device pointers)"""
        check(lib().hpfw_gpu_resample_pcm16(self._h, d_in, int(n_in), int(n_clips), int(rate), d_out, stream))

    def resample(self, pcm, rate):
        """int16 [n] or [n_clips][n] at `rate` (8 000 .. 192 000 Hz) -> int16 at 44 100 Hz, same shape but the length"""
        pcm = np.ascontiguousarray(pcm, np.int16)
        one = pcm.ndim == 1
        if one:
            pcm = pcm[None, :]
        out = np.zeros((pcm.shape[0], resample_length(pcm.shape[1], rate)), np.int16)
        if out.size:
            check(lib().hpfw_gpu_resample_pcm16_host(self._h, _hp(pcm), pcm.shape[1], pcm.shape[0], int(rate), _hp(out)))
        return out[0] if one else out

    # ---- time warp and mix (k_warp.hip) ---------------------------------
    warp_table = staticmethod(lambda: warp_table())

    def _warp(self, pcm, tracks, m0, n_out, mix):
        pcm = np.ascontiguousarray(pcm, np.int16).ravel()
        tracks = np.ascontiguousarray(tracks, WARP_TRACK_DTYPE).ravel()
        out = np.zeros(max(int(n_out), 0) if mix else (tracks.size, max(int(n_out), 0)), np.int16)
        fn = lib().hpfw_gpu_mix_pcm16_host if mix else lib().hpfw_gpu_warp_pcm16_host
        check(fn(self._h, _hp(pcm) if pcm.size else None, pcm.size, _hp(tracks) if tracks.size else None, tracks.size, int(m0), int(n_out),
                 _hp(out) if out.size else None))
        return out

    def warp(self, pcm, tracks, m0, n_out):
        """pcm int16 [n] (host), tracks WARP_TRACK_DTYPE (sources are ranges of pcm) -> int16 [n_tracks][n_out]: outputs
        m0 .. m0 + n_out - 1 of every track, read at i0 + m + (f0 + m d) 2^-40; a negative gain negates"""
        return self._warp(pcm, tracks, m0, n_out, False)

    def mix(self, pcm, tracks, m0, n_out):
        """-> int16 [n_out]: clamp((sum_k gain_k y_k + 2^14) >> 15) of the tracks' outputs, fused"""
        return self._warp(pcm, tracks, m0, n_out, True)

    def warp_dev(self, d_pcm, n_pcm, tracks, m0, n_out, d_out, stream=0):
        """device pointers; tracks WARP_TRACK_DTYPE on the host; d_out int16 [n_tracks][n_out]"""
        tracks = np.ascontiguousarray(tracks, WARP_TRACK_DTYPE).ravel()
        check(lib().hpfw_gpu_warp_pcm16(self._h, d_pcm, int(n_pcm), _hp(tracks) if tracks.size else None, tracks.size, int(m0), int(n_out),
                                        d_out, stream))

    def mix_dev(self, d_pcm, n_pcm, tracks, m0, n_out, d_mix, stream=0):
        """device pointers; d_mix int16 [n_out]"""
        tracks = np.ascontiguousarray(tracks, WARP_TRACK_DTYPE).ravel()
        check(lib().hpfw_gpu_mix_pcm16(self._h, d_pcm, int(n_pcm), _hp(tracks) if tracks.size else None, tracks.size, int(m0), int(n_out),
                                       d_mix, stream))

    def set_projection(self, mode):
        """1 (default): fixed-point projection, exact integer sums (S9q); 0: the f32 fma chain (S9)"""
        check(lib().hpfw_gpu_set_projection(self._h, int(mode)))

    def get_projection(self):
        return int(lib().hpfw_gpu_get_projection(self._h))

    def hashprints_from_db_dev(self, d_db, n_clips, c, d_hp, stream=0):
        check(lib().hpfw_gpu_hashprints_from_db(self._h, d_db, n_clips, c, d_hp, stream))

    def stage_delta_q_dev(self, d_db, n_clips, c, d_delta, d_hp=0, stream=0):
        """the exact integer sums of the fixed-point projection, int64 [n_clips][64][c - 99] (parity checkpoint)"""
        check(lib().hpfw_gpu_stage_delta_q(self._h, d_db, n_clips, c, d_delta, d_hp, stream))

    def debug_q_products(self):
        """(tiles, listed values, redone tiles) of the last six-product launch of this handle; waits for the device"""
        v = (ctypes.c_int64 * 3)()
        p = [ctypes.cast(ctypes.byref(v, 8 * i), ctypes.c_void_p) for i in range(3)]
        check(lib().hpfw_gpu_debug_q_products(self._h, *p))
        return int(v[0]), int(v[1]), int(v[2])

    def prepare_length(self, n_samples):
        """build the host half of the tables of a clip length on the calling thread (thread-safe; see hpfw_gpu.h)"""
        check(lib().hpfw_gpu_prepare_length(self._h, int(n_samples)))

    def debug_workspace(self, which):
        """(device pointer, bytes) of extraction workspace `which` as the last call left it (diagnosis)"""
        p, b = ctypes.c_void_p(), ctypes.c_size_t()
        check(lib().hpfw_gpu_debug_workspace(self._h, which, ctypes.byref(p), ctypes.byref(b)))
        return p.value or 0, b.value

    def chirpz_table(self, n_samples, which):
        """device-generated table as complex64: 0 w, 1 T_L, 2 Bhat, 3 w[k] / L of the chirp-z forward transform; 4 (every
        length) the constant-Q stage's windows, bands concatenated"""
        count = ctypes.c_int64(0)
        check(lib().hpfw_gpu_chirpz_table(self._h, n_samples, which, None, 0, ctypes.byref(count)))
        out = np.zeros(count.value, np.float32)
        check(lib().hpfw_gpu_chirpz_table(self._h, n_samples, which, _hp(out), count.value, ctypes.byref(count)))
        return out.view(np.complex64)

    def stage_spectrum_dev(self, d_pcm, n_samples, n_clips, d_x, stream=0):
        check(lib().hpfw_gpu_stage_spectrum(self._h, d_pcm, n_samples, n_clips, d_x, stream))

    def stage_cqmag_dev(self, d_x, n_samples, n_clips, d_mag, stream=0):
        check(lib().hpfw_gpu_stage_cqmag(self._h, d_x, n_samples, n_clips, d_mag, stream))

    def stage_db_dev(self, d_mag, n_clips, c, d_db, stream=0):
        check(lib().hpfw_gpu_stage_db(self._h, d_mag, n_clips, c, d_db, stream))

    def stage_project_dev(self, d_db, n_clips, c, d_proj, stream=0):
        check(lib().hpfw_gpu_stage_project(self._h, d_db, n_clips, c, d_proj, stream))

    def stage_pack_dev(self, d_proj, n_clips, n_frames, d_hp, stream=0):
        check(lib().hpfw_gpu_stage_pack(self._h, d_proj, n_clips, n_frames, d_hp, stream))

    def stage_spectrogram_dev(self, d_pcm, n_samples, n_clips, d_db, stream=0):
        check(lib().hpfw_gpu_stage_spectrogram(self._h, d_pcm, n_samples, n_clips, d_db, stream))

    # ---- Mel front-end ---------------------------------------------------------------------
    def mel_spectrogram(self, pcm):
        """pcm int16 [n_clips][n] (host) -> list of dB-mel spectrograms [33][kept columns] (mel.h:34-104)"""
        pcm = np.ascontiguousarray(pcm, np.int16)
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        nf = int(lib().hpfw_gpu_mel_frames(pcm.shape[1]))
        out = np.zeros((pcm.shape[0], 33, nf), np.float32)
        cols = np.zeros(pcm.shape[0], np.int32)
        check(lib().hpfw_gpu_mel_spectrogram_pcm16_host(self._h, _hp(pcm), pcm.shape[1], pcm.shape[0], _hp(out), _hp(cols)))
        return [np.ascontiguousarray(out[i, :, :cols[i]]) for i in range(pcm.shape[0])]

    # ---- HashprintHandle with other template arguments ---------------------------------------
    def cfg_set_filters(self, cfg, filters_colmajor):
        c = HandleConfig(*cfg)
        f = np.ascontiguousarray(filters_colmajor, np.float32).ravel()
        if f.size != c.bits * c.rows * c.context:
            raise ValueError("filters must hold bits x rows * context floats (column-major)")
        check(lib().hpfw_gpu_cfg_set_filters(self._h, ctypes.byref(c), _hp(f)))

    def cfg_hashprints_dev(self, cfg, d_s, d_cols, n_clips, stride, d_hp, hp_stride, d_proj=0, stream=0):
        c = HandleConfig(*cfg)
        check(lib().hpfw_gpu_cfg_hashprints(self._h, ctypes.byref(c), d_s, d_cols, n_clips, stride, d_hp, hp_stride,
                                            d_proj, stream))

    def cfg_cov_reset(self, cfg):
        check(lib().hpfw_gpu_cfg_cov_reset(self._h, ctypes.byref(HandleConfig(*cfg))))

    def cfg_cov_accumulate_dev(self, cfg, d_s, d_cols, n_clips, stride, stream=0):
        check(lib().hpfw_gpu_cfg_cov_accumulate(self._h, ctypes.byref(HandleConfig(*cfg)), d_s, d_cols, n_clips, stride, stream))

    def cfg_cov_get(self, cfg):
        kt = cfg[0] * cfg[1]
        cov = np.zeros((kt, kt), np.float32)
        n = ctypes.c_int64(0)
        check(lib().hpfw_gpu_cfg_cov_get(self._h, ctypes.byref(HandleConfig(*cfg)), _hp(cov), ctypes.byref(n)))
        return cov, int(n.value)

    def cfg_learn_filters(self, cfg):
        f = np.zeros(cfg[3] * cfg[0] * cfg[1], np.float32)
        check(lib().hpfw_gpu_cfg_learn_filters(self._h, ctypes.byref(HandleConfig(*cfg)), _hp(f)))
        return f

    def mel_hashprints(self, pcm):
        """the combiner's Algo (combiner.h:12) on host PCM [n_clips][n]: list of uint16 hashprint arrays"""
        pcm = np.ascontiguousarray(pcm, np.int16)
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        stride = max(int(lib().hpfw_gpu_mel_frames(pcm.shape[1])) - 81, 1)
        hp = np.zeros((pcm.shape[0], stride), np.uint16)
        n = np.zeros(pcm.shape[0], np.int32)
        check(lib().hpfw_gpu_mel_hashprints_pcm16_host(self._h, _hp(pcm), pcm.shape[1], pcm.shape[0], _hp(hp), stride, _hp(n)))
        return [hp[i, :n[i]].copy() for i in range(pcm.shape[0])]

    def mel_cov_accumulate(self, pcm):
        """the combiner's filter learning: Mel front end + covariance of HPFW_CONFIG_COMBINER frames, pcm [n_clips][n] host"""
        pcm = np.ascontiguousarray(pcm, np.int16)
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        check(lib().hpfw_gpu_mel_cov_accumulate_pcm16_host(self._h, _hp(pcm), pcm.shape[1], pcm.shape[0]))

    # ---- AudioCombiner's inverted index (combiner.h:90-132) ----------------------------------
    def combiner_clear(self):
        check(lib().hpfw_gpu_combiner_clear(self._h))

    def combiner_add(self, recordings):
        """append recordings (a list of uint16 arrays), numbered on from combiner_size()"""
        hp, off = _ragged(recordings, np.uint16)
        check(lib().hpfw_gpu_combiner_add(self._h, _hp(hp), _hp(off), off.size - 1))

    def combiner_add_dev(self, d_hp, offsets, stream=0):
        off = np.ascontiguousarray(offsets, np.int64)
        check(lib().hpfw_gpu_combiner_add_device(self._h, d_hp, _hp(off), off.size - 1, stream))

    def combiner_size(self):
        return int(lib().hpfw_gpu_combiner_size(self._h))

    def combiner_get(self):
        """(val_start int64 [65537], rec uint32 [postings], off uint32 [postings]) copied back from HBM"""
        vs = np.zeros(65537, np.int64)
        check(lib().hpfw_gpu_combiner_get(self._h, _hp(vs), None, None, 0))
        n = int(vs[-1])
        rec, off = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        check(lib().hpfw_gpu_combiner_get(self._h, _hp(vs), _hp(rec), _hp(off), n))
        return vs, rec, off

    def combiner_find(self, queries, exclude=None):
        """AudioCombiner::find for every query (a list of uint16 arrays): COMBINE_DTYPE [n_q]; exclude: ids or -1"""
        hp, off = _ragged(queries, np.uint16)
        ex = _exclude(exclude, off.size - 1)
        out = np.zeros(off.size - 1, COMBINE_DTYPE)
        check(lib().hpfw_gpu_combiner_find(self._h, _hp(hp), _hp(off), _hp(ex), off.size - 1, _hp(out)))
        return out

    def combiner_find_dev(self, d_q, q_off, exclude, d_out, stream=0):
        off = np.ascontiguousarray(q_off, np.int64)
        ex = _exclude(exclude, off.size - 1)
        check(lib().hpfw_gpu_combiner_find_device(self._h, d_q, _hp(off), _hp(ex), off.size - 1, d_out, stream))

    def combiner_align(self, queries, k, exclude=None):
        """per query the k recordings with the highest per-offset peak: ALIGN_DTYPE [n_q][k]"""
        hp, off = _ragged(queries, np.uint16)
        ex = _exclude(exclude, off.size - 1)
        out = np.zeros((off.size - 1, int(k)), ALIGN_DTYPE)
        check(lib().hpfw_gpu_combiner_align(self._h, _hp(hp), _hp(off), _hp(ex), off.size - 1, int(k), _hp(out)))
        return out

    def combiner_align_dev(self, d_q, q_off, exclude, k, d_out, stream=0):
        off = np.ascontiguousarray(q_off, np.int64)
        ex = _exclude(exclude, off.size - 1)
        check(lib().hpfw_gpu_combiner_align_device(self._h, d_q, _hp(off), _hp(ex), off.size - 1, int(k), d_out, stream))

    # ---- sample-accurate offsets ------------------------------------------
    def xcorr(self, pcm, jobs, want_r=False):
        """pcm int16 [n] (host), jobs XCORR_JOB_DTYPE [n_jobs] (operands are ranges of pcm) -> XCORR_PEAK_DTYPE [n_jobs], or
        (peaks, list of int64 r [2 radius + 1] per job, lag -radius first) with want_r: exact int64 sums"""
        pcm = np.ascontiguousarray(pcm, np.int16).ravel()
        jobs = np.ascontiguousarray(jobs, XCORR_JOB_DTYPE).ravel()
        peaks = np.zeros(jobs.size, XCORR_PEAK_DTYPE)
        # (the library validates the jobs; r is sized from radii it would accept)
        lags = 2 * np.clip(jobs["radius"].astype(np.int64), 0, XCORR_MAX_RADIUS) + 1
        r = np.zeros(int(lags.sum()) if want_r else 0, np.int64)
        check(lib().hpfw_gpu_xcorr_pcm16_host(self._h, _hp(pcm), pcm.size, _hp(jobs), jobs.size, _hp(r) if want_r else None,
                                              _hp(peaks)))
        if not want_r:
            return peaks
        off = np.concatenate([[0], np.cumsum(lags)])
        return peaks, [r[off[i]:off[i + 1]] for i in range(jobs.size)]

    def xcorr_dev(self, d_pcm, jobs, d_r, d_peaks, stream=0):
        """device pointers (d_r 0 for none); jobs XCORR_JOB_DTYPE on the host"""
        jobs = np.ascontiguousarray(jobs, XCORR_JOB_DTYPE).ravel()
        check(lib().hpfw_gpu_xcorr_pcm16(self._h, d_pcm, _hp(jobs), jobs.size, d_r or None, d_peaks, stream))

    def mel_kept_frames(self, pcm):
        """pcm int16 [n] or [n_clips][n] (host) -> per clip the int32 frames its Mel columns came from (the silent frames are
        dropped before hashing): column c is frame frames[c], centred on sample 441 * frames[c]"""
        pcm = np.ascontiguousarray(pcm, np.int16)
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        stride = max(int(lib().hpfw_gpu_mel_frames(pcm.shape[1])), 1)
        frames = np.zeros((pcm.shape[0], stride), np.int32)
        n = np.zeros(pcm.shape[0], np.int32)
        check(lib().hpfw_gpu_mel_kept_frames_pcm16_host(self._h, _hp(pcm), pcm.shape[1], pcm.shape[0], _hp(frames), stride, _hp(n)))
        return [frames[i, :n[i]].copy() for i in range(pcm.shape[0])]

    # ---- filter learning ------------------------------------------------------------------
    def cov_reset(self):
        check(lib().hpfw_gpu_cov_reset(self._h))

    def cov_accumulate_dev(self, d_pcm, n_samples, n_clips, stream=0):
        check(lib().hpfw_gpu_cov_accumulate_pcm16(self._h, d_pcm, n_samples, n_clips, stream))

    def cov_accumulate(self, pcm):
        """pcm: int16 [n_clips][n_samples] on the host"""
        pcm = np.ascontiguousarray(pcm, np.int16)
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        check(lib().hpfw_gpu_cov_accumulate_pcm16_host(self._h, _hp(pcm), pcm.shape[1], pcm.shape[0]))

    def cov_accumulate_db_dev(self, d_db, n_clips, c, stream=0):
        check(lib().hpfw_gpu_cov_accumulate_db(self._h, d_db, n_clips, c, stream))

    def cov_get(self):
        """(accum_cov [2420][2420] float32, number of clips accumulated)"""
        cov = np.zeros((2420, 2420), np.float32)
        n = ctypes.c_int64(0)
        check(lib().hpfw_gpu_cov_get(self._h, _hp(cov), ctypes.byref(n)))
        return cov, int(n.value)

    def cov_set(self, cov, n_files):
        c = np.ascontiguousarray(cov, np.float32)
        assert c.shape == (2420, 2420)
        check(lib().hpfw_gpu_cov_set(self._h, _hp(c), int(n_files)))

    def learn_filters(self):
        """eigen-solve the accumulated covariance, install and return the filters (flat column-major)"""
        f = np.zeros(64 * 2420, np.float32)
        check(lib().hpfw_gpu_learn_filters(self._h, _hp(f)))
        return f

    # ---- index + search ------------------------------------------------------------------
    def index_clear(self):
        check(lib().hpfw_gpu_index_clear(self._h))

    def index_add(self, hp, offsets):
        hp = np.ascontiguousarray(hp, np.uint64).ravel()
        off = np.ascontiguousarray(offsets, np.int64)
        check(lib().hpfw_gpu_index_add(self._h, _hp(hp), _hp(off), off.size - 1))

    def index_add_dev(self, d_hp, offsets, stream=0):
        off = np.ascontiguousarray(offsets, np.int64)
        check(lib().hpfw_gpu_index_add_device(self._h, d_hp, _hp(off), off.size - 1, stream))

    def index_get(self):
        """(hashprints uint64 [total], offsets int64 [n_clips + 1]) copied back from HBM"""
        off = np.zeros(self.index_size() + 1, np.int64)
        check(lib().hpfw_gpu_index_get(self._h, _hp(off), None, 0))
        hp = np.zeros(int(off[-1]), np.uint64)
        check(lib().hpfw_gpu_index_get(self._h, _hp(off), _hp(hp), hp.size))
        return hp, off

    def extract_db(self, s_colmajor):
        """hashprints of a cached dB spectrogram: s_colmajor float32 [cols][121] (Eigen column-major
        [121 x cols] as cache/spectros/<stem> holds it)"""
        s = np.ascontiguousarray(s_colmajor, np.float32)
        cols, rows = s.shape
        n = ctypes.c_int64(0)
        hp = np.zeros(max(cols - 99, 0), np.uint64)
        check(lib().hpfw_gpu_extract_db_host(self._h, _hp(s), rows, cols, _hp(hp), hp.size, ctypes.byref(n)))
        return hp[:n.value]

    def index_size(self):
        return int(lib().hpfw_gpu_index_size(self._h))

    def index_set_clip_base(self, base):
        check(lib().hpfw_gpu_index_set_clip_base(self._h, int(base)))

    # ---- index maintenance
    def index_remove(self, clips, stream=0):
        """the clips named (ids in add order, without the clip base) become empty and the others' hashprints close up in
        place; ids, index_size() and index_capacity() stay.  Enqueues on stream, ordered with every other call."""
        ids = np.ascontiguousarray(clips, np.int64).ravel()
        check(lib().hpfw_gpu_index_remove(self._h, _hp(ids) if ids.size else None, ids.size, stream))

    def index_reserve(self, n_hashprints):
        check(lib().hpfw_gpu_index_reserve(self._h, int(n_hashprints)))

    def index_capacity(self):
        return int(lib().hpfw_gpu_index_capacity(self._h))

    # ---- catalogue self-join: the recordings of the index that duplicate or contain each other
    def index_selfjoin(self, min_overlap, rate_num, rate_den, cap=1024):
        """DUP_PAIR_DTYPE [n]: every pair of clips a < b whose best lag by the overlap rule, over at least min_overlap
        hashprints, has dist * rate_den <= rate_num * overlap, in ascending (a, b) (include/hpfw_gpu.h).  Neither min_overlap
        nor the threshold has a default.  cap: the pairs the first call has room for; the buffer grows to the count and the call
        repeats while the count exceeds it."""
        cap = max(int(cap), 0)
        while True:
            out = np.zeros(cap, DUP_PAIR_DTYPE)
            count = ctypes.c_int64(0)
            check(lib().hpfw_gpu_index_selfjoin(self._h, int(min_overlap), int(rate_num), int(rate_den), _hp(out), cap, ctypes.byref(count)))
            if count.value <= cap:
                return out[:count.value].copy()
            cap = int(count.value)

    def index_selfjoin_dev(self, min_overlap, rate_num, rate_den, d_out, cap, d_count, stream=0):
        """device pointers: d_out DUP_PAIR_DTYPE [cap] (0 with cap = 0) receives the first cap pairs, d_count (int64) their
        total number, which may exceed cap"""
        check(lib().hpfw_gpu_index_selfjoin_device(self._h, int(min_overlap), int(rate_num), int(rate_den), d_out, int(cap), d_count, stream))

    # ---- local self-join: the passages that recordings of the index share
    def index_localjoin(self, max_rate, min_score, cap=1024):
        """PASSAGE_PAIR_DTYPE [n]: every pair of clips a < b whose best run of consecutive hashprints on any diagonal, at
        max_rate - popcount a hashprint, scores at least min_score, in ascending (a, b) (include/hpfw_gpu.h).  Neither
        max_rate (1..31) nor min_score (>= 1) has a default.  cap: as index_selfjoin's."""
        cap = max(int(cap), 0)
        while True:
            out = np.zeros(cap, PASSAGE_PAIR_DTYPE)
            count = ctypes.c_int64(0)
            check(lib().hpfw_gpu_index_localjoin(self._h, int(max_rate), int(min_score), _hp(out), cap, ctypes.byref(count)))
            if count.value <= cap:
                return out[:count.value].copy()
            cap = int(count.value)

    def index_localjoin_dev(self, max_rate, min_score, d_out, cap, d_count, stream=0):
        """device pointers: d_out PASSAGE_PAIR_DTYPE [cap] (0 with cap = 0) receives the first cap pairs, d_count (int64) their
        total number, which may exceed cap"""
        check(lib().hpfw_gpu_index_localjoin_device(self._h, int(max_rate), int(min_score), d_out, int(cap), d_count, stream))

    # ---- ingest check: recordings that are not in the index joined against it
    def index_join(self, x_hp, x_off, min_overlap, rate_num, rate_den, among_new, cap=1024):
        """DUP_PAIR_DTYPE [n]: the pairs (a, b) that index_add(x_hp, x_off) followed by index_selfjoin would add to the
        self-join's answer -- b one of the recordings x (id index_size() + its position), a < b an indexed recording or, with
        among_new, an earlier x -- without the index changing (include/hpfw_gpu.h).  Neither min_overlap nor the threshold nor
        among_new has a default.  cap: as index_selfjoin's."""
        x = np.ascontiguousarray(x_hp, np.uint64).ravel()
        off = np.ascontiguousarray(x_off, np.int64)
        cap = max(int(cap), 0)
        while True:
            out = np.zeros(cap, DUP_PAIR_DTYPE)
            count = ctypes.c_int64(0)
            check(lib().hpfw_gpu_index_join(self._h, _hp(x) if x.size else None, _hp(off), off.size - 1, int(among_new), int(min_overlap),
                                            int(rate_num), int(rate_den), _hp(out), cap, ctypes.byref(count)))
            if count.value <= cap:
                return out[:count.value].copy()
            cap = int(count.value)

    def index_join_dev(self, d_x_hp, x_off, min_overlap, rate_num, rate_den, among_new, d_out, cap, d_count, stream=0):
        """device pointers: d_x_hp the recordings' hashprints (x_off: host), d_out DUP_PAIR_DTYPE [cap] (0 with cap = 0) receives
        the first cap pairs, d_count (int64) their total number, which may exceed cap"""
        off = np.ascontiguousarray(x_off, np.int64)
        check(lib().hpfw_gpu_index_join_device(self._h, d_x_hp, _hp(off), off.size - 1, int(among_new), int(min_overlap), int(rate_num),
                                               int(rate_den), d_out, int(cap), d_count, stream))

    def search_topk(self, q_hp, q_off, k):
        q = np.ascontiguousarray(q_hp, np.uint64).ravel()
        off = np.ascontiguousarray(q_off, np.int64)
        out = np.zeros((off.size - 1, k), HIT_DTYPE)
        check(lib().hpfw_gpu_search_topk(self._h, _hp(q), _hp(off), off.size - 1, int(k), _hp(out)))
        return out

    # ---- overlap search: lags that overhang a clip's ends, rated per overlapping hashprint
    @staticmethod
    def _exclude(exclude, n_q):
        if exclude is None:
            return None
        ex = np.ascontiguousarray(exclude, np.int32).ravel()
        if ex.size != n_q:
            raise ValueError("exclude must hold one clip index (or -1) per query")
        return ex

    def search_overlap(self, q_hp, q_off, k, min_overlap, exclude=None):
        """OVERLAP_HIT_DTYPE [n_q][k] by the rule of include/hpfw_gpu.h; exclude: None or per query the clip (in add order)
        to leave out, -1 for none"""
        q = np.ascontiguousarray(q_hp, np.uint64).ravel()
        off = np.ascontiguousarray(q_off, np.int64)
        ex = self._exclude(exclude, off.size - 1)
        out = np.zeros((off.size - 1, k), OVERLAP_HIT_DTYPE)
        check(lib().hpfw_gpu_search_overlap(self._h, _hp(q), _hp(off), off.size - 1, None if ex is None else _hp(ex), int(min_overlap),
                                            int(k), _hp(out)))
        return out

    def search_overlap_dev(self, d_q, q_off, k, min_overlap, d_out, exclude=None, stream=0):
        off = np.ascontiguousarray(q_off, np.int64)
        ex = self._exclude(exclude, off.size - 1)
        check(lib().hpfw_gpu_search_overlap_device(self._h, d_q, _hp(off), off.size - 1, None if ex is None else _hp(ex), int(min_overlap),
                                                   int(k), d_out, stream))

    def search_overlap_scored(self, q_hp, q_off, k, min_overlap, exclude=None):
        """(OVERLAP_HIT_DTYPE [n_q][k] as search_overlap, STATS_DTYPE [n_q]): the moments of overlap_rate(dist, overlap) over the
        clips that have a candidate for the query, the excluded one left out"""
        q = np.ascontiguousarray(q_hp, np.uint64).ravel()
        off = np.ascontiguousarray(q_off, np.int64)
        ex = self._exclude(exclude, off.size - 1)
        out = np.zeros((off.size - 1, k), OVERLAP_HIT_DTYPE)
        stats = np.zeros(off.size - 1, STATS_DTYPE)
        check(lib().hpfw_gpu_search_overlap_scored(self._h, _hp(q), _hp(off), off.size - 1, None if ex is None else _hp(ex),
                                                   int(min_overlap), int(k), _hp(out), _hp(stats)))
        return out, stats

    def search_overlap_scored_dev(self, d_q, q_off, k, min_overlap, d_out, d_stats, exclude=None, stream=0):
        off = np.ascontiguousarray(q_off, np.int64)
        ex = self._exclude(exclude, off.size - 1)
        check(lib().hpfw_gpu_search_overlap_scored_device(self._h, d_q, _hp(off), off.size - 1, None if ex is None else _hp(ex),
                                                          int(min_overlap), int(k), d_out, d_stats, stream))

    # ---- warped search: subsequence DTW over hashprints, distance and path
    @staticmethod
    def _pairs(pairs):
        p = np.ascontiguousarray(pairs, np.int32)
        if p.size and (p.ndim != 2 or p.shape[1] != 2):
            raise ValueError("pairs must be [n_pairs][2]: (query index, clip index)")
        return p.reshape(-1, 2)

    def dtw_pairs(self, q_hp, q_off, pairs):
        """DTW_HIT_DTYPE [n_pairs] by the rule of include/hpfw_gpu.h: pairs [n_pairs][2] of (query index, clip index in add
        order, without the clip base); the hit names the clip as the pair does, a pair without a candidate gives padding"""
        q = np.ascontiguousarray(q_hp, np.uint64).ravel()
        off = np.ascontiguousarray(q_off, np.int64)
        p = self._pairs(pairs)
        out = np.zeros(p.shape[0], DTW_HIT_DTYPE)
        check(lib().hpfw_gpu_dtw_pairs(self._h, _hp(q), _hp(off), off.size - 1, _hp(p), p.shape[0], _hp(out)))
        return out

    def dtw_pairs_dev(self, d_q, q_off, pairs, d_out, stream=0):
        off = np.ascontiguousarray(q_off, np.int64)
        p = self._pairs(pairs)
        check(lib().hpfw_gpu_dtw_pairs_device(self._h, d_q, _hp(off), off.size - 1, _hp(p), p.shape[0], d_out, stream))

    def search_dtw(self, q_hp, q_off, k, candidates):
        """DTW_HIT_DTYPE [n_q][k], the k best clips by (dist, clip).  candidates (no default): 0 = every clip of the index is
        warped against every query; k..64 = the plain search's that many best clips of each query are re-ranked"""
        q = np.ascontiguousarray(q_hp, np.uint64).ravel()
        off = np.ascontiguousarray(q_off, np.int64)
        out = np.zeros((off.size - 1, k), DTW_HIT_DTYPE)
        check(lib().hpfw_gpu_search_dtw(self._h, _hp(q), _hp(off), off.size - 1, int(candidates), int(k), _hp(out)))
        return out

    def search_dtw_dev(self, d_q, q_off, k, candidates, d_out, stream=0):
        off = np.ascontiguousarray(q_off, np.int64)
        check(lib().hpfw_gpu_search_dtw_device(self._h, d_q, _hp(off), off.size - 1, int(candidates), int(k), d_out, stream))

    def dtw_path(self, q_hp, clip):
        """(hit DTW_HIT_DTYPE scalar, path int32 [K]): the column of clip `clip` (add order) every query hashprint lies on;
        no candidate: the padding record and -1 everywhere"""
        q = np.ascontiguousarray(q_hp, np.uint64).ravel()
        path = np.full(max(q.size, 1), -1, np.int32)
        hit = np.zeros(1, DTW_HIT_DTYPE)
        check(lib().hpfw_gpu_dtw_path(self._h, _hp(q) if q.size else None, q.size, int(clip), _hp(path), _hp(hit)))
        return hit[0], path[:q.size]

    def dtw_path_dev(self, d_q, k_q, clip, d_path, d_hit, stream=0):
        check(lib().hpfw_gpu_dtw_path_device(self._h, d_q, int(k_q), int(clip), d_path, d_hit, stream))

    # ---- local search: the best-scoring run of query hashprints on any diagonal of a clip
    def search_local(self, q_hp, q_off, k, max_rate):
        """LOCAL_HIT_DTYPE [n_q][k] by the rule of include/hpfw_gpu.h: per query the k clips with the best run, larger score
        first, then the smaller clip.  max_rate (no default), 1..31: a run's score is max_rate * length - dist"""
        q = np.ascontiguousarray(q_hp, np.uint64).ravel()
        off = np.ascontiguousarray(q_off, np.int64)
        out = np.zeros((off.size - 1, k), LOCAL_HIT_DTYPE)
        check(lib().hpfw_gpu_search_local(self._h, _hp(q), _hp(off), off.size - 1, int(max_rate), int(k), _hp(out)))
        return out

    def search_local_dev(self, d_q, q_off, k, max_rate, d_out, stream=0):
        off = np.ascontiguousarray(q_off, np.int64)
        check(lib().hpfw_gpu_search_local_device(self._h, d_q, _hp(off), off.size - 1, int(max_rate), int(k), d_out, stream))

    def search_votes(self, q_hp, q_off):
        """AnnStorage-style voting search with exact neighbours: VOTE_DTYPE [n_q]"""
        q = np.ascontiguousarray(q_hp, np.uint64).ravel()
        off = np.ascontiguousarray(q_off, np.int64)
        out = np.zeros(off.size - 1, VOTE_DTYPE)
        check(lib().hpfw_gpu_search_votes(self._h, _hp(q), _hp(off), off.size - 1, _hp(out)))
        return out

    def knn_windows(self, q_hp, q_off):
        """the 5 nearest 64-hashprint windows of every query position: keys [n_windows][5]"""
        q = np.ascontiguousarray(q_hp, np.uint64).ravel()
        off = np.ascontiguousarray(q_off, np.int64)
        n_win = int(np.maximum(np.diff(off) - 63, 0).sum())
        keys = np.zeros((n_win, 5), np.uint64)
        check(lib().hpfw_gpu_knn_windows(self._h, _hp(q), _hp(off), off.size - 1, _hp(keys), keys.size))
        return keys

    # ---- the voting search with device buffers: the tally runs on the device
    def knn_windows_dev(self, d_q, q_off, d_keys, keys_cap, stream=0):
        """d_keys [n_windows][5] uint64 on the device (keys_cap: its capacity in keys), ascending per window"""
        off = np.ascontiguousarray(q_off, np.int64)
        check(lib().hpfw_gpu_knn_windows_device(self._h, d_q, _hp(off), off.size - 1, d_keys, int(keys_cap), stream))

    def vote_windows_dev(self, d_keys, w_first, d_db_off, n_clips, d_out, clip_base=0, stream=0):
        """the tally alone: w_first [n_q + 1] (host) the first window of each query in d_keys [..][5]; d_db_off int64
        [n_clips + 1] and d_out VOTE_DTYPE [n_q] on the device"""
        wf = np.ascontiguousarray(w_first, np.int64)
        check(lib().hpfw_gpu_vote_windows_device(self._h, d_keys, _hp(wf), wf.size - 1, d_db_off, int(n_clips), int(clip_base), d_out, stream))

    def search_votes_dev(self, d_q, q_off, d_out, stream=0):
        """search_votes with the queries and d_out (VOTE_DTYPE [n_q]) on the device"""
        off = np.ascontiguousarray(q_off, np.int64)
        check(lib().hpfw_gpu_search_votes_device(self._h, d_q, _hp(off), off.size - 1, d_out, stream))

    def merge_knn_dev(self, d_in, pos_base, n_win, d_out, stream=0):
        """d_in [n_shards][n_win][5] -> d_out [n_win][5]; pos_base [n_shards] (host): the hashprints in earlier shards"""
        base = np.ascontiguousarray(pos_base, np.int64)
        check(lib().hpfw_gpu_merge_knn_device(self._h, d_in, _hp(base), base.size, int(n_win), d_out, stream))

    def search_topk_transposed(self, q_hp, q_off, n_shifts, k):
        """q_off [n_q * n_shifts + 1]: query set q * n_shifts + i is shift i of query q -> SHIFT_HIT_DTYPE [n_q][k]"""
        q = np.ascontiguousarray(q_hp, np.uint64).ravel()
        off = np.ascontiguousarray(q_off, np.int64)
        if (off.size - 1) % n_shifts:
            raise ValueError("q_off must hold n_q * n_shifts + 1 offsets")
        out = np.zeros(((off.size - 1) // n_shifts, k), SHIFT_HIT_DTYPE)
        check(lib().hpfw_gpu_search_topk_transposed(self._h, _hp(q), _hp(off), out.shape[0], int(n_shifts), int(k), _hp(out)))
        return out

    def search_topk_transposed_dev(self, d_q, q_off, n_shifts, k, d_out, stream=0):
        off = np.ascontiguousarray(q_off, np.int64)
        check(lib().hpfw_gpu_search_topk_transposed_device(self._h, d_q, _hp(off), (off.size - 1) // n_shifts, int(n_shifts),
                                                            int(k), d_out, stream))

    # ---- scored search: the same hits and, per query row, the moments of the per-clip distances
    def search_topk_scored(self, q_hp, q_off, k):
        """(HIT_DTYPE [n_q][k] as search_topk, STATS_DTYPE [n_q])"""
        q = np.ascontiguousarray(q_hp, np.uint64).ravel()
        off = np.ascontiguousarray(q_off, np.int64)
        out = np.zeros((off.size - 1, k), HIT_DTYPE)
        stats = np.zeros(off.size - 1, STATS_DTYPE)
        check(lib().hpfw_gpu_search_topk_scored(self._h, _hp(q), _hp(off), off.size - 1, int(k), _hp(out), _hp(stats)))
        return out, stats

    def search_topk_scored_dev(self, d_q, q_off, k, d_out, d_stats, stream=0):
        off = np.ascontiguousarray(q_off, np.int64)
        check(lib().hpfw_gpu_search_topk_scored_device(self._h, d_q, _hp(off), off.size - 1, int(k), d_out, d_stats, stream))

    def search_topk_transposed_scored(self, q_hp, q_off, n_shifts, k):
        """(SHIFT_HIT_DTYPE [n_q][k] as search_topk_transposed, STATS_DTYPE [n_q][n_shifts]): a hit is scored against
        stats[q][hit.shift_index]"""
        q = np.ascontiguousarray(q_hp, np.uint64).ravel()
        off = np.ascontiguousarray(q_off, np.int64)
        if (off.size - 1) % n_shifts:
            raise ValueError("q_off must hold n_q * n_shifts + 1 offsets")
        n_q = (off.size - 1) // n_shifts
        out = np.zeros((n_q, k), SHIFT_HIT_DTYPE)
        stats = np.zeros((n_q, n_shifts), STATS_DTYPE)
        check(lib().hpfw_gpu_search_topk_transposed_scored(self._h, _hp(q), _hp(off), n_q, int(n_shifts), int(k), _hp(out),
                                                           _hp(stats)))
        return out, stats

    def search_topk_transposed_scored_dev(self, d_q, q_off, n_shifts, k, d_out, d_stats, stream=0):
        off = np.ascontiguousarray(q_off, np.int64)
        check(lib().hpfw_gpu_search_topk_transposed_scored_device(self._h, d_q, _hp(off), (off.size - 1) // n_shifts, int(n_shifts),
                                                                   int(k), d_out, d_stats, stream))

    # ---- search within sets of clips: every query names the set it may be answered with
    def search_topk_within(self, q_hp, q_off, k, set_off, set_clips, q_set, scored=False):
        """search_topk with query q restricted to the clips of set q_set[q] (-1: the whole index): the sets in CSR form,
        set_off [n_sets + 1] and set_clips (clip indexes in add order, strictly ascending inside a set).  The answer is the one
        an index of just those clips gives, with this index's clip ids.  HIT_DTYPE [n_q][k]; scored: (hits, STATS_DTYPE [n_q]),
        the moments over the set's counted clips."""
        q = np.ascontiguousarray(q_hp, np.uint64).ravel()
        off = np.ascontiguousarray(q_off, np.int64)
        so, sc, qs = _within_sets(set_off, set_clips, q_set, off.size - 1)
        out = np.zeros((off.size - 1, k), HIT_DTYPE)
        stats = np.zeros(off.size - 1, STATS_DTYPE) if scored else None
        check(lib().hpfw_gpu_search_topk_within(self._h, _hp(q), _hp(off), off.size - 1, int(k), _hp(so), so.size - 1, _hp(sc), _hp(qs),
                                                _hp(out), _hp(stats) if scored else None))
        return (out, stats) if scored else out

    def search_topk_within_dev(self, d_q, q_off, k, set_off, set_clips, q_set, d_out, d_stats=None, stream=0):
        """the same with the queries, d_out and d_stats (None: no moments) on the device; the sets stay on the host"""
        off = np.ascontiguousarray(q_off, np.int64)
        so, sc, qs = _within_sets(set_off, set_clips, q_set, off.size - 1)
        check(lib().hpfw_gpu_search_topk_within_device(self._h, d_q, _hp(off), off.size - 1, int(k), _hp(so), so.size - 1, _hp(sc), _hp(qs),
                                                       d_out, d_stats, stream))

    def search_topk_transposed_within(self, q_hp, q_off, n_shifts, k, set_off, set_clips, q_set, scored=False):
        """search_topk_transposed within sets: q_set has one entry per query (for all its n_shifts variants).
        SHIFT_HIT_DTYPE [n_q][k]; scored: (hits, STATS_DTYPE [n_q][n_shifts])"""
        q = np.ascontiguousarray(q_hp, np.uint64).ravel()
        off = np.ascontiguousarray(q_off, np.int64)
        if (off.size - 1) % n_shifts:
            raise ValueError("q_off must hold n_q * n_shifts + 1 offsets")
        n_q = (off.size - 1) // n_shifts
        so, sc, qs = _within_sets(set_off, set_clips, q_set, n_q)
        out = np.zeros((n_q, k), SHIFT_HIT_DTYPE)
        stats = np.zeros((n_q, n_shifts), STATS_DTYPE) if scored else None
        check(lib().hpfw_gpu_search_topk_transposed_within(self._h, _hp(q), _hp(off), n_q, int(n_shifts), int(k), _hp(so), so.size - 1,
                                                           _hp(sc), _hp(qs), _hp(out), _hp(stats) if scored else None))
        return (out, stats) if scored else out

    def search_topk_transposed_within_dev(self, d_q, q_off, n_shifts, k, set_off, set_clips, q_set, d_out, d_stats=None, stream=0):
        off = np.ascontiguousarray(q_off, np.int64)
        n_q = (off.size - 1) // n_shifts
        so, sc, qs = _within_sets(set_off, set_clips, q_set, n_q)
        check(lib().hpfw_gpu_search_topk_transposed_within_device(self._h, d_q, _hp(off), n_q, int(n_shifts), int(k), _hp(so), so.size - 1,
                                                                  _hp(sc), _hp(qs), d_out, d_stats, stream))

    # ---- a sharded search's gathered results (k_merge.hip): device twins of merge_topk and of the sum of the moments
    def merge_topk_dev(self, d_in, n_shards, n_q, k, d_out, stream=0):
        """d_in [n_shards][n_q][k] of HIT_DTYPE or SHIFT_HIT_DTYPE records -> d_out [n_q][k] (device pointers)"""
        check(lib().hpfw_gpu_merge_topk_device(self._h, d_in, int(n_shards), int(n_q), int(k), d_out, stream))

    def sum_stats_dev(self, d_in, n_shards, rows, d_out, stream=0):
        """d_out[r] = sum over shards of d_in[shard][r] (STATS_DTYPE rows, device pointers)"""
        check(lib().hpfw_gpu_sum_stats_device(self._h, d_in, int(n_shards), int(rows), d_out, stream))

    def index_offsets(self):
        """the index's clip offsets int64 [n_clips + 1] (host copy; no hashprint is downloaded)"""
        off = np.zeros(self.index_size() + 1, np.int64)
        check(lib().hpfw_gpu_index_get(self._h, _hp(off), None, 0))
        return off

    def search_topk_dev(self, d_q, q_off, k, d_out, stream=0):
        off = np.ascontiguousarray(q_off, np.int64)
        check(lib().hpfw_gpu_search_topk_device(self._h, d_q, _hp(off), off.size - 1, int(k), d_out, stream))

    # ---- timing --------------------------------------------------------------------------
    def timer_start(self, stream=0):
        check(lib().hpfw_gpu_timer_start(self._h, stream))

    def timer_stop(self, stream=0):
        ms = ctypes.c_float(0)
        check(lib().hpfw_gpu_timer_stop(self._h, stream, ctypes.byref(ms)))
        return float(ms.value)

    def set_kernel_timing(self, mask):
        check(lib().hpfw_gpu_set_kernel_timing(self._h, int(mask)))

    def kernel_timing(self):
        n = ctypes.c_int(16)
        names = (ctypes.c_char_p * 16)()
        ms = (ctypes.c_float * 16)()
        launches = (ctypes.c_int * 16)()
        check(lib().hpfw_gpu_get_kernel_timing(self._h, names, ms, launches, ctypes.byref(n)))
        return {names[i].decode(): (float(ms[i]), int(launches[i])) for i in range(n.value)}


class GpuStreams:
    """hpfw_gpu_streams: n_streams rings of `capacity` samples on a Gpu handle; push() appends chunks, extract() hashes the
    windows [w hop, w hop + win) that have become complete, bit for bit what Gpu.extract_windows gives for the feed so far.
    A feed at another rate than 44 100 Hz (rates) is converted chunk by chunk on its way into the ring: its ring holds the
    first emitted() samples of Gpu.resample of everything pushed, and push, push_dev and room count in samples at the feed's
    rate.  Close it before its Gpu."""

    def __init__(self, gpu, n_streams, win, hop, capacity=0, tempos=None, shifts=None, rates=None):
        self._t = None if tempos is None else np.ascontiguousarray(tempos, np.float32).ravel()
        self._sh = None if shifts is None else np.ascontiguousarray(shifts, np.int32).ravel()
        p = StreamsParams(int(n_streams), 0 if self._t is None else self._t.size, 0 if self._sh is None else self._sh.size, 0, int(win),
                          int(hop), int(capacity), None if self._t is None else _hp(self._t), None if self._sh is None else _hp(self._sh))
        self._s = ctypes.c_void_p()
        self._gpu = gpu                                   # (keeps the handle alive as long as the set)
        if rates is not None:
            rates = np.clip(np.asarray(rates, np.int64), -1, 2 ** 31 - 1).astype(np.int32)
            rates = np.full(int(n_streams), rates, np.int32) if rates.ndim == 0 else np.ascontiguousarray(rates).ravel()
            if rates.size != int(n_streams):
                raise ValueError("one rate per feed")
        check(lib().hpfw_gpu_streams_create_rates(gpu._h, ctypes.byref(p), None if rates is None else _hp(rates), ctypes.byref(self._s)))
        info = StreamsInfo()
        check(lib().hpfw_gpu_streams_info(self._s, ctypes.byref(info), None, None))
        self.n_streams, self.win, self.hop, self.capacity = info.n_streams, info.win, info.hop, info.capacity
        self.per_window, self.n_sets = info.per_window, info.n_sets
        self.variants = tempos is not None or shifts is not None
        self.rates = np.zeros(self.n_streams, np.int32)
        check(lib().hpfw_gpu_streams_rates(self._s, _hp(self.rates), None))

    def emitted(self):
        """per feed the 44.1 kHz samples its ring has received so far (the samples pushed, for a 44.1 kHz feed)"""
        out = np.zeros(self.n_streams, np.int64)
        check(lib().hpfw_gpu_streams_rates(self._s, None, _hp(out)))
        return out

    def close(self):
        if getattr(self, "_s", None):
            lib().hpfw_gpu_streams_destroy(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:        # interpreter teardown
            pass

    def _counts(self, counts):
        c = np.ascontiguousarray(counts, np.int64).ravel()
        if c.size != self.n_streams:
            raise ValueError("one count per feed")
        return c

    def push(self, chunks):
        """chunks: one int16 array or None per feed (host) -> the number of complete windows not yet handed out"""
        if len(chunks) != self.n_streams:
            raise ValueError("one chunk (or None) per feed")
        parts = [np.zeros(0, np.int16) if c is None else np.ascontiguousarray(c, np.int16).ravel() for c in chunks]
        counts = np.array([p.size for p in parts], np.int64)
        pcm = np.concatenate(parts) if counts.sum() else np.zeros(1, np.int16)
        n = ctypes.c_int64()
        check(lib().hpfw_gpu_streams_push(self._s, _hp(pcm), _hp(counts), ctypes.byref(n)))
        return n.value

    def push_dev(self, d_pcm, counts, stream=0):
        """d_pcm: the chunks concatenated in feed order (device pointer), counts [n_streams]"""
        c = self._counts(counts)
        n = ctypes.c_int64()
        check(lib().hpfw_gpu_streams_push_device(self._s, d_pcm, _hp(c), ctypes.byref(n), stream))
        return n.value

    def room(self):
        """the samples every feed can take now, at the feed's rate"""
        out = np.zeros(self.n_streams, np.int64)
        check(lib().hpfw_gpu_streams_room(self._s, _hp(out)))
        return out

    def info(self):
        """(samples received, windows handed out) per feed"""
        n, e = np.zeros(self.n_streams, np.int64), np.zeros(self.n_streams, np.int64)
        check(lib().hpfw_gpu_streams_info(self._s, None, _hp(n), _hp(e)))
        return n, e

    def ready(self):
        e = self.info()[1]
        return int(sum(window_count(int(a), self.win, self.hop) - int(b) for a, b in zip(self.emitted(), e)))

    def _hp_shape(self, n):
        return (n, self.n_sets, self.per_window // self.n_sets) if self.variants else (n, self.per_window)

    def extract(self, cap=None, clips=False):
        """hashes up to cap ready windows (None: all): (STREAM_WINDOW_DTYPE [n], uint64 [n][n_hp] or [n][V][n_hp_v]) and
        with clips=True also their samples int16 [n][win]"""
        cap = self.ready() if cap is None else min(int(cap), self.ready())
        which = np.zeros(max(cap, 1), STREAM_WINDOW_DTYPE)
        hp = np.zeros(max(cap, 1) * self.per_window, np.uint64)
        pcm = np.zeros((max(cap, 1), self.win), np.int16) if clips else None
        n = ctypes.c_int64()
        check(lib().hpfw_gpu_streams_extract_host(self._s, cap, _hp(hp), None if pcm is None else _hp(pcm), _hp(which), ctypes.byref(n)))
        out = (which[:n.value], hp[:n.value * self.per_window].reshape(self._hp_shape(n.value)))
        return out + (pcm[:n.value],) if clips else out

    def extract_dev(self, cap, d_hp, d_clips=0, stream=0):
        """the device form: d_hp [cap][per_window] and d_clips (0 or [cap][win]) are device pointers -> STREAM_WINDOW_DTYPE [n]"""
        which = np.zeros(max(int(cap), 1), STREAM_WINDOW_DTYPE)
        n = ctypes.c_int64()
        check(lib().hpfw_gpu_streams_extract(self._s, int(cap), d_hp, d_clips or None, _hp(which), ctypes.byref(n), stream))
        return which[:n.value]

    def reset(self, feed):
        check(lib().hpfw_gpu_streams_reset(self._s, int(feed)))


def _ragged(arrays, dtype):
    """a list of 1-D arrays -> (concatenation, offsets int64 [n + 1])"""
    arrays = [np.ascontiguousarray(a, dtype).ravel() for a in arrays]
    off = np.zeros(len(arrays) + 1, np.int64)
    off[1:] = np.cumsum([a.size for a in arrays])
    hp = np.concatenate(arrays) if arrays and off[-1] else np.zeros(1, dtype)
    return np.ascontiguousarray(hp, dtype), off


def _exclude(exclude, n):
    if exclude is None:
        return np.full(max(n, 1), -1, np.int32)
    ex = np.ascontiguousarray(exclude, np.int32).ravel()
    if ex.size != n:
        raise ValueError("exclude needs one recording id (or -1) per query")
    return ex if n else np.full(1, -1, np.int32)


def wav_read(path):
    """a WAV file as the live-id file entry points read it: int16 mono (stereo averaged), 44.1 kHz only"""
    n = ctypes.c_int64(0)
    p = os.fsencode(path)
    check(lib().hpfw_gpu_wav_read_pcm16(p, None, 0, ctypes.byref(n)))
    out = np.zeros(max(n.value, 1), np.int16)
    check(lib().hpfw_gpu_wav_read_pcm16(p, _hp(out), out.size, ctypes.byref(n)))
    return out[:n.value]


def wav_read_any(path):
    """a WAV file at its own rate: (int16 mono (stereo averaged, truncating), rate in Hz); not resampled"""
    n, rate = ctypes.c_int64(0), ctypes.c_int32(0)
    p = os.fsencode(path)
    check(lib().hpfw_gpu_wav_read_pcm16_any(p, None, 0, ctypes.byref(n), ctypes.byref(rate)))
    out = np.zeros(max(n.value, 1), np.int16)
    check(lib().hpfw_gpu_wav_read_pcm16_any(p, _hp(out), out.size, ctypes.byref(n), ctypes.byref(rate)))
    return out[:n.value], int(rate.value)


def read_wav_44k(gpu, path, resample):
    """a WAV file's PCM at 44.1 kHz: wav_read, or with `resample` wav_read_any converted on `gpu` (Gpu.resample)"""
    if not resample:
        return wav_read(path)
    x, rate = wav_read_any(path)
    return gpu.resample(x, rate) if rate != 44100 and x.size else x


def resample_length(n_in, rate):
    """samples at 44.1 kHz of n_in samples at `rate`: ceil(n_in L / M)"""
    n = ctypes.c_int64(0)
    check(lib().hpfw_gpu_resample_length(int(n_in), int(rate), ctypes.byref(n)))
    return int(n.value)


def streams_emitted(n_in, rate):
    """the 44.1 kHz samples a live feed at `rate` has been given after n_in input samples (hpfw_gpu_streams_emitted)"""
    n = ctypes.c_int64()
    check(lib().hpfw_gpu_streams_emitted(int(n_in), int(rate), ctypes.byref(n)))
    return n.value


def streams_tail(rate):
    """H of the filter of `rate` (T = 2 H taps per phase; 0 at 44 100 Hz): emitted(n + H) = resample_length(n)"""
    L, M, T = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    check(lib().hpfw_gpu_resample_table(int(rate), None, 0, ctypes.byref(L), ctypes.byref(M), ctypes.byref(T)))
    return T.value // 2


def resample_table(rate):
    """(L, M, taps int16 [L][T]) of the conversion from `rate` to 44.1 kHz (T = 0 at 44.1 kHz: the identity)"""
    L, M, T = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    check(lib().hpfw_gpu_resample_table(int(rate), None, 0, ctypes.byref(L), ctypes.byref(M), ctypes.byref(T)))
    taps = np.zeros((L.value, T.value), np.int16)
    if taps.size:
        check(lib().hpfw_gpu_resample_table(int(rate), _hp(taps), taps.size, ctypes.byref(L), ctypes.byref(M), ctypes.byref(T)))
    return int(L.value), int(M.value), taps


def warp_table():
    """taps int16 [P][T] of the time warp: row p the fractional delay p / P (hpfw_gpu_warp_table)"""
    P, T = ctypes.c_int32(0), ctypes.c_int32(0)
    check(lib().hpfw_gpu_warp_table(None, 0, ctypes.byref(P), ctypes.byref(T)))
    taps = np.zeros((P.value, T.value), np.int16)
    check(lib().hpfw_gpu_warp_table(_hp(taps), taps.size, ctypes.byref(P), ctypes.byref(T)))
    return taps


def drift_anchors(s_lo, s_hi, q, length, anchor_len, anchor_hop):
    """(centre start, left starts going outward, right starts going outward) of a pair's anchors (hpfw_gpu_drift_anchors)"""
    nl, nr, n = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0)
    args = (int(s_lo), int(s_hi), int(q), int(length), int(anchor_len), int(anchor_hop))
    check(lib().hpfw_gpu_drift_anchors(*args, None, 0, ctypes.byref(nl), ctypes.byref(nr), ctypes.byref(n)))
    starts = np.zeros(n.value, np.int64)
    check(lib().hpfw_gpu_drift_anchors(*args, _hp(starts), starts.size, ctypes.byref(nl), ctypes.byref(nr), ctypes.byref(n)))
    return int(starts[0]), [int(v) for v in starts[1:1 + nl.value]], [int(v) for v in starts[1 + nl.value:]]


def drift_fit(n, lag):
    """(a, b, rms) of the Theil-Sen line lag ~ a + b n (hpfw_gpu_drift_fit; the centre anchor first)"""
    n = np.ascontiguousarray(n, np.int64).ravel()
    lag = np.ascontiguousarray(lag, np.int64).ravel()
    if n.size != lag.size:
        raise ValueError("drift_fit: one lag per position")
    a, b, rms = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
    check(lib().hpfw_gpu_drift_fit(_hp(n) if n.size else None, _hp(lag) if n.size else None, n.size, ctypes.byref(a), ctypes.byref(b),
                                   ctypes.byref(rms)))
    return a.value, b.value, rms.value


def time_map_q40(A, B):
    """(i0, f0, d) of a source whose sample n sits at A + (1 + B) n of the output's timeline (hpfw_gpu_time_map_q40)"""
    i0, f0, d = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    check(lib().hpfw_gpu_time_map_q40(float(A), float(B), ctypes.byref(i0), ctypes.byref(f0), ctypes.byref(d)))
    return i0.value, f0.value, d.value


def wav_write(path, pcm, channels=1):
    """int16 [n] (interleaved for 2 channels) as a 44.1 kHz PCM16 WAV file with a 44-byte header (hpfw_gpu_wav_write_pcm16)"""
    pcm = np.ascontiguousarray(pcm, np.int16).ravel()
    check(lib().hpfw_gpu_wav_write_pcm16(os.fsencode(path), _hp(pcm) if pcm.size else None, pcm.size, int(channels)))


def merge_topk(per_shard_hits, k):
    """per_shard_hits: [n_shards][n_q][k] HIT_DTYPE -> [n_q][k], ascending (dist, clip)."""
    a = np.ascontiguousarray(per_shard_hits, HIT_DTYPE)
    n_shards, n_q, kk = a.shape
    assert kk == k
    out = np.zeros((n_q, k), HIT_DTYPE)
    check(lib().hpfw_gpu_merge_topk(_hp(a), n_shards, n_q, k, _hp(out)))
    return out


def supported_length(n_samples):
    """the smallest supported clip length >= n_samples, or -1"""
    return int(lib().hpfw_gpu_supported_length(int(n_samples)))


CONV_HANN_PERIODIC, CONV_LG_HALF_EVEN, CONV_FLOAT_GEOMETRY, CONV_NO_IFFT_SCALE = 1, 2, 4, 8


def plan_checksum(n_samples, conventions=0):
    out = np.zeros(8, np.uint64)
    rc = lib().hpfw_gpu_plan_checksum_ex(abs(int(n_samples)), int(n_samples < 0), int(conventions), _hp(out))
    if rc != 0:
        raise HpfwError(f"unsupported clip length {n_samples}")
    return out


def debug_db_term_sweep(first, count):
    """(differing, fallbacks, first differing pattern or None) of the two evaluations of the dB term on the `count`
    consecutive float bit patterns from `first` (hpfw_gpu_debug_db_term_sweep), on the current device"""
    out = np.zeros(3, np.uint64)
    check(lib().hpfw_gpu_debug_db_term_sweep(int(first), int(count), _hp(out)))
    return int(out[0]), int(out[1]), (None if int(out[2]) == 2 ** 64 - 1 else int(out[2]))


def plan_cols_tables(n_samples):
    """the column stage's host tables of a 7-smooth clip length (hpfw_gpu_plan_cols_tables): a dict of n1, n2, hq, the
    tile and step counts, wq int32 [n1][2], corr float64 [hq][2], image int8 [mt][ks][3][64][16] and image2 int8
    [mt2][2 ks2][3][64][16] (None when the length does not take the parity-split kernel)"""
    d = np.zeros(9, np.int32)
    if lib().hpfw_gpu_plan_cols_tables(int(n_samples), _hp(d), None, None, None, None) != 0:
        raise HpfwError(f"no column-stage tables for clip length {n_samples}")
    n1, n2, hq, mt, ks, mt2, ks2, split = (int(v) for v in d[:8])
    wq, corr = np.zeros((n1, 2), np.int32), np.zeros((hq, 2), np.float64)
    image = np.zeros((mt, ks, 3, 64, 16), np.int8)
    image2 = np.zeros((mt2, 2 * ks2, 3, 64, 16), np.int8) if split else None
    check_rc = lib().hpfw_gpu_plan_cols_tables(int(n_samples), _hp(d), _hp(wq), _hp(corr), _hp(image),
                                               _hp(image2) if split else None)
    if check_rc != 0:
        raise HpfwError(f"no column-stage tables for clip length {n_samples}")
    return dict(n1=n1, n2=n2, hq=hq, mt=mt, ks=ks, mt2=mt2, ks2=ks2, wq=wq, corr=corr, image=image, image2=image2)


BZ_SHAPE_FIELDS = ("a", "n1", "L", "slack", "k1lo", "k1n", "need", "nt2", "n_tiles2", "step", "n_blocks", "n2", "n_tiles1",
                   "kmin", "kmax")


def plan_bz_shape(n_samples, force_bluestein=False):
    """the shape of the chirp-z forward transform of a clip length (hpfw_gpu_plan_bz_shape, host only): a dict of a, n1 = 16 a,
    L = n1 n2, slack = L - (n + (kmax - kmin) - 1), the consumed rows k1lo, k1n, their row tiles need, nt2, n_tiles2, the last
    stage's step and n_blocks, n2, n_tiles1, kmin, kmax"""
    d = np.zeros(len(BZ_SHAPE_FIELDS), np.int32)
    if lib().hpfw_gpu_plan_bz_shape(int(n_samples), int(bool(force_bluestein)), _hp(d)) != 0:
        raise HpfwError(f"no chirp-z forward transform for clip length {n_samples}")
    return {k: int(v) for k, v in zip(BZ_SHAPE_FIELDS, d)}
