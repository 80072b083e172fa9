"""ctypes binding of ``libffsalign.so`` (the C ABI declared in ``include/ffsubsync_amd.h``).

There is deliberately no fallback: if the HIP library is missing or no MI355X is visible, the
product path raises -- it never degrades to a CPU implementation.
"""
import ctypes
import math
import os
import threading
from typing import Dict, Optional, Tuple

import numpy as np

_LIB_NAME = "libffsalign.so"
_lib = None
_lib_lock = threading.Lock()

FFS_DTYPE_U8 = 0
FFS_DTYPE_F32 = 1
FFS_DTYPE_F64 = 3  # float64 samples (fp32 transforms nominate, fp64 re-evaluation of the caller's own samples)
FFS_DTYPE_U1 = 2  # one bit per sample, numpy.packbits(..., bitorder="little") order, 32-bit words
FFS_DTYPE_RUNS = 5  # the vector's boundary list (an `ffs_runs_list` device block: 16-byte header + 8-byte entries)
FLAG_EMPTY_WINDOW = 1
FLAG_AMBIGUOUS = 2
FLAG_FILTERED = 4
FLAG_DIRECT = 8

MAX_FFT_LENGTH = 1 << 24

CAND_RESULT_DTYPE = np.dtype(
    [("score", "<f8"), ("offset", "<i8"), ("score_f32", "<f4"), ("flags", "<i4")], align=True
)
PAIR_RESULT_DTYPE = np.dtype(
    [("score", "<f8"), ("offset", "<i8"), ("best_cand", "<i4"), ("flags", "<i4")], align=True
)
assert CAND_RESULT_DTYPE.itemsize == 24 and PAIR_RESULT_DTYPE.itemsize == 24
# ffs_quality_result (include/ffsubsync_amd.h; static size 160 bytes)
QUALITY_MAX_PEAKS = 8
QUALITY_FLAT = 1  # FFS_QUALITY_FLAT: every score of the lag set is equal (std = 0)
QUALITY_EMPTY_WINDOW = 2  # FFS_QUALITY_EMPTY_WINDOW: the lag set is empty
QUALITY_RESULT_DTYPE = np.dtype(
    [("peak_score", "<f8", (QUALITY_MAX_PEAKS,)), ("peak_offset", "<i8", (QUALITY_MAX_PEAKS,)), ("mean", "<f8"),
     ("std", "<f8"), ("n_lags", "<i8"), ("n_peaks", "<i4"), ("flags", "<i4")], align=True
)
QUALITY_RESULT_BYTES = 160
assert QUALITY_RESULT_DTYPE.itemsize == QUALITY_RESULT_BYTES
# ffs_piece_report (include/ffsubsync_amd.h; static size 224 bytes)
PIECE_OWN_NOT_PEAK = 4  # FFS_PIECE_OWN_NOT_PEAK: the piece's peak 1 is not at its own offset
PIECE_REPORT_DTYPE = np.dtype(
    [("first_block", "<i8"), ("end_block", "<i8"), ("start_sample", "<i8"), ("end_sample", "<i8"), ("offset", "<i8"),
     ("own_score", "<f8"), ("prev_score", "<f8"), ("next_score", "<f8"), ("mean", "<f8"), ("std", "<f8"),
     ("n_lags", "<i8"), ("peak_score", "<f8", (QUALITY_MAX_PEAKS,)), ("peak_offset", "<i8", (QUALITY_MAX_PEAKS,)),
     ("n_peaks", "<i4"), ("flags", "<i4")], align=True
)
PIECE_REPORT_BYTES = 224
assert PIECE_REPORT_DTYPE.itemsize == PIECE_REPORT_BYTES
# ffs_segment_report (include/ffsubsync_amd.h; static size 264 bytes)
SEGMENT_OWN_NOT_PEAK = 4  # FFS_SEGMENT_OWN_NOT_PEAK: the segment's peak 1 is not at shift 0 (its own path)
SEGMENT_REPORT_DTYPE = np.dtype(
    [("first_block", "<i8"), ("end_block", "<i8"), ("start_sample", "<i8"), ("end_sample", "<i8"),
     ("first_offset", "<i8"), ("last_offset", "<i8"), ("min_offset", "<i8"), ("max_offset", "<i8"),
     ("own_score", "<f8"), ("prev_score", "<f8"), ("next_score", "<f8"), ("flat_score", "<f8"), ("flat_offset", "<i8"),
     ("mean", "<f8"), ("std", "<f8"), ("n_lags", "<i8"), ("peak_score", "<f8", (QUALITY_MAX_PEAKS,)),
     ("peak_shift", "<i8", (QUALITY_MAX_PEAKS,)), ("n_peaks", "<i4"), ("flags", "<i4")], align=True
)
SEGMENT_REPORT_BYTES = 264
RPATH_ROUND_SEGMENTS, RPATH_CHUNK_WORDS = 8, 512  # csrc/ffs_drift_range_sched.h
assert SEGMENT_REPORT_DTYPE.itemsize == SEGMENT_REPORT_BYTES
# ffs_smooth_segment (include/ffsubsync_amd.h; static size 32 bytes) and the limits of the smooth fit
SMOOTH_MAX_KNOT_BLOCKS = 256  # FFS_SMOOTH_MAX_KNOT_BLOCKS
SMOOTH_MAX_RADIUS = 16  # FFS_SMOOTH_MAX_RADIUS
SMOOTH_SEGMENT_DTYPE = np.dtype(
    [("fit_total", "<f8"), ("line_score", "<f8"), ("bend_total", "<f8"), ("n_knots", "<i4"), ("reserved", "<i4")], align=True
)
SMOOTH_SEGMENT_BYTES = 32
assert SMOOTH_SEGMENT_DTYPE.itemsize == SMOOTH_SEGMENT_BYTES
SMOOTH_MAX_STATES = 33 * 33  # (2 * SMOOTH_MAX_RADIUS + 1) ** 2
SMOOTH_BLOCK_BYTES = 33 * 33 * 9 + 36  # smooth workspace per block of a pair in flight: line scores, back-pointers, tables
# ffs_break_refine (include/ffsubsync_amd.h; static size 88 bytes)
REFINE_MAX_RADIUS = 131072  # FFS_REFINE_MAX_RADIUS
REFINE_CLIPPED = 1  # FFS_REFINE_CLIPPED: the window was narrowed by a neighbouring break's midpoint
REFINE_AT_EDGE = 2  # FFS_REFINE_AT_EDGE: a cut sits at a window edge inside the file (the radius may be too small)
REFINE_UNMATCHED = 4  # FFS_REFINE_UNMATCHED: t1 < t2
BREAK_REFINE_DTYPE = np.dtype(
    [("block", "<i8"), ("cut", "<i8"), ("lo", "<i8"), ("hi", "<i8"), ("t1", "<i8"), ("t2", "<i8"),
     ("offset_prev", "<i8"), ("offset_next", "<i8"), ("coarse_score", "<f8"), ("refined_score", "<f8"),
     ("flags", "<i4"), ("reserved", "<i4")], align=True
)
BREAK_REFINE_BYTES = 88
assert BREAK_REFINE_DTYPE.itemsize == BREAK_REFINE_BYTES
# ffs_cue / ffs_cue_report (include/ffsubsync_amd.h; static sizes 24 and 120 bytes)
CUE_MAX_RADIUS = 4096  # FFS_CUE_MAX_RADIUS
CUE_MAX_CONTEXT = 65536  # FFS_CUE_MAX_CONTEXT
CUE_EMPTY = 1  # FFS_CUE_EMPTY: the cue holds no sample of the subtitle vector
CUE_INVALID = 2  # FFS_CUE_INVALID: |lag| > 2^31
CUE_NO_OVERLAP = 4  # FFS_CUE_NO_OVERLAP: no sample of the window has a partner at the applied lag
CUE_BEST_AT_EDGE = 8  # FFS_CUE_BEST_AT_EDGE: |best_delta| = radius > 0
CUE_FLAT = 16  # FFS_CUE_FLAT: every lag within the radius scores the same
CUE_SILENT = 32  # FFS_CUE_SILENT: no reference speech under the cue at any lag within the radius
CUE_DTYPE = np.dtype([("start", "<i8"), ("end", "<i8"), ("lag", "<i8")], align=True)
CUE_BYTES = 24
assert CUE_DTYPE.itemsize == CUE_BYTES
CUE_REPORT_DTYPE = np.dtype(
    [("start", "<i8"), ("end", "<i8"), ("lo", "<i8"), ("hi", "<i8"), ("lag", "<i8"), ("own", "<i4", (4,)),
     ("best", "<i4", (4,)), ("own_score", "<f8"), ("best_score", "<f8"), ("best_delta", "<i4"), ("n_best", "<i4"),
     ("cue_own_n11", "<i4"), ("cue_own_ov", "<i4"), ("cue_max_n11", "<i4"), ("cue_max_delta", "<i4"), ("flags", "<i4"),
     ("reserved", "<i4")], align=True
)
CUE_REPORT_BYTES = 120
assert CUE_REPORT_DTYPE.itemsize == CUE_REPORT_BYTES
# ffs_cue_retime / ffs_retime_summary (include/ffsubsync_amd.h; static sizes 64 and 40 bytes)
RETIME_MAX_RADIUS = 1024  # FFS_RETIME_MAX_RADIUS
RETIME_Q = 64  # FFS_RETIME_Q: penalty_q and jump_q are in 64ths of a score sample
RETIME_NO_JUMP = -1  # FFS_RETIME_NO_JUMP: the linear link cost is not capped
RETIME_MAX_PENALTY_Q = 1 << 20
RETIME_MAX_JUMP_Q = 1 << 40
RETIME_WORK_CAP = 256 << 20  # FFS_RETIME_WORK_CAP: bytes of retime workspace one sub-batch may use
RETIME_CELL_BYTES = 6  # int32 profile + int16 backpointer per (cue, delta)
RETIME_DESC_BYTES = 72  # the descriptor a retime call keeps per pair in flight
RETIME_KEEP_ORDER = 1  # FFS_RETIME_KEEP_ORDER (call flag)
RETIME_EMPTY = 1  # FFS_RETIME_EMPTY
RETIME_INVALID = 2  # FFS_RETIME_INVALID
RETIME_MOVED = 4  # FFS_RETIME_MOVED: delta != 0
RETIME_JUMP = 8  # FFS_RETIME_JUMP: the incoming link paid jump_q instead of the linear cost
RETIME_UNORDERED = 16  # FFS_RETIME_UNORDERED: the cue starts before its predecessor in the input
RETIME_ORDER_TIGHT = 32  # FFS_RETIME_ORDER_TIGHT: the order constraint holds with equality
RETIME_AT_EDGE = 64  # FFS_RETIME_AT_EDGE: |delta| = radius > 0
CUE_RETIME_DTYPE = np.dtype(
    [("start", "<i8"), ("end", "<i8"), ("lag", "<i8"), ("delta", "<i4"), ("flags", "<i4"), ("own", "<i4"), ("at", "<i4"),
     ("best", "<i4"), ("best_delta", "<i4"), ("link", "<i8"), ("reserved", "<i4", (2,))], align=True
)
CUE_RETIME_BYTES = 64
assert CUE_RETIME_DTYPE.itemsize == CUE_RETIME_BYTES
RETIME_SUMMARY_DTYPE = np.dtype(
    [("total", "<i8"), ("own_total", "<i8"), ("best_total", "<i8"), ("n_live", "<i4"), ("n_moved", "<i4"),
     ("n_jumps", "<i4"), ("reserved", "<i4")], align=True
)
RETIME_SUMMARY_BYTES = 40
assert RETIME_SUMMARY_DTYPE.itemsize == RETIME_SUMMARY_BYTES
# ffs_sweep_profile (include/ffsubsync_amd.h; static size 232 bytes)
SWEEP_MAX_PEAKS = 8
SWEEP_FLAT = 1  # FFS_SWEEP_FLAT: every point not skipped scores the same, or none is left (std = 0)
SWEEP_EMPTY = 2  # FFS_SWEEP_EMPTY: no point left after skipping
SWEEP_AMBIGUOUS = 4  # FFS_SWEEP_AMBIGUOUS: some point carried FFS_FLAG_AMBIGUOUS
SWEEP_PROFILE_DTYPE = np.dtype(
    [("peak_score", "<f8", (SWEEP_MAX_PEAKS,)), ("peak_offset", "<i8", (SWEEP_MAX_PEAKS,)),
     ("peak_index", "<i8", (SWEEP_MAX_PEAKS,)), ("mean", "<f8"), ("std", "<f8"), ("n_points", "<i8"), ("n_skipped", "<i8"),
     ("n_peaks", "<i4"), ("flags", "<i4")], align=True
)
SWEEP_PROFILE_BYTES = 232
assert SWEEP_PROFILE_DTYPE.itemsize == SWEEP_PROFILE_BYTES
# ffs_null_result and the limits of ffs_surrogate_lists (include/ffsubsync_amd.h; static size 56 bytes)
SURR_MAX_UNITS = 8192  # FFS_SURR_MAX_UNITS: units (runs but the last) of a list
SURR_MAX_K = 4096  # FFS_SURR_MAX_K: surrogates per vector
SURR_BAD_ODD, SURR_BAD_TRUNCATED, SURR_BAD_BOUND, SURR_BAD_UNITS = 1, 2, 4, 8  # FFS_SURR_BAD_*: bits of a vector's status
NULL_FLAT = 1  # FFS_NULL_FLAT: every usable null scores the same, or none is left (std = 0)
NULL_EMPTY = 2  # FFS_NULL_EMPTY: no usable null record, or the real record is not usable
NULL_AMBIGUOUS = 4  # FFS_NULL_AMBIGUOUS: some record carried FFS_FLAG_AMBIGUOUS
NULL_RESULT_DTYPE = np.dtype(
    [("real_score", "<f8"), ("null_mean", "<f8"), ("null_std", "<f8"), ("null_min", "<f8"), ("null_max", "<f8"),
     ("n_null", "<i4"), ("n_ge", "<i4"), ("n_gt", "<i4"), ("flags", "<i4")], align=True
)
NULL_RESULT_BYTES = 56
assert NULL_RESULT_DTYPE.itemsize == NULL_RESULT_BYTES
# ffs_stability_result and the limits of ffs_subsample_lists (include/ffsubsync_amd.h; static size 112 bytes)
STAB_MAX_K = 4096  # FFS_STAB_MAX_K: subsamples per vector
STAB_MAX_BLOCK_RUNS = 1 << 24  # FFS_STAB_MAX_BLOCK_RUNS
SUB_BAD_ODD, SUB_BAD_TRUNCATED, SUB_BAD_BOUND = 1, 2, 4  # FFS_SUB_BAD_*: bits of a vector's status
STAB_EMPTY = 1  # FFS_STAB_EMPTY: the real record is not usable, or no subsample record is
STAB_AMBIGUOUS = 2  # FFS_STAB_AMBIGUOUS: some record carried FFS_FLAG_AMBIGUOUS
STAB_NO_PAIRS = 4  # FFS_STAB_NO_PAIRS: no pair (2j, 2j + 1) with both members usable
STABILITY_RESULT_DTYPE = np.dtype(
    [("real_score", "<f8"), ("real_offset", "<i8"), ("off_min", "<i8"), ("off_max", "<i8"), ("off_median", "<i8"),
     ("off_lo", "<i8"), ("off_hi", "<i8"), ("max_dev", "<i8"), ("max_pair_gap", "<i8"), ("pair_score_min", "<f8"),
     ("n_sub", "<i4"), ("n_within", "<i4"), ("n_pairs", "<i4"), ("n_pairs_within", "<i4"), ("tol", "<i8"), ("flags", "<i4"),
     ("reserved", "<i4")], align=True
)
STABILITY_RESULT_BYTES = 112
assert STABILITY_RESULT_DTYPE.itemsize == STABILITY_RESULT_BYTES
# ffs_vad_threshold and the limits of the adaptive energy VAD (include/ffsubsync_amd.h; static size 48 bytes)
VAD_MAX_EDGES = 255  # FFS_VAD_MAX_EDGES
VAD_MAX_BINS = 256  # FFS_VAD_MAX_BINS
VAD_MAX_FRAMES = 1 << 23  # FFS_VAD_MAX_FRAMES: frames of one histogram the pick takes before it falls back
VAD_RULE_OTSU, VAD_RULE_FLOOR = 0, 1  # FFS_VAD_RULE_*
VAD_RULES = {"otsu": VAD_RULE_OTSU, "floor": VAD_RULE_FLOOR}
VAD_THR_FALLBACK = 1  # FFS_VAD_THR_FALLBACK: threshold_bin is fallback_bin
VAD_THR_TOO_LONG = 2  # FFS_VAD_THR_TOO_LONG
VAD_THR_EMPTY = 4  # FFS_VAD_THR_EMPTY: no frame at or above lo_bin
VAD_THR_FLAT = 8  # FFS_VAD_THR_FLAT: all counted frames share one bin
VAD_THR_CLAMPED_LO = 16  # FFS_VAD_THR_CLAMPED_LO
VAD_THR_CLAMPED_HI = 32  # FFS_VAD_THR_CLAMPED_HI
VAD_THRESHOLD_DTYPE = np.dtype(
    [("threshold_bin", "<i4"), ("flags", "<i4"), ("floor_bin", "<i4"), ("top_bin", "<i4"), ("n_frames", "<i8"),
     ("n_counted", "<i8"), ("n_speech", "<i8"), ("eta", "<f8")], align=True
)
VAD_THRESHOLD_BYTES = 48
assert VAD_THRESHOLD_DTYPE.itemsize == VAD_THRESHOLD_BYTES
# ffs_vad_gate, the record of the steady-run gate (include/ffsubsync_amd.h; static size 48 bytes)
VAD_GATE_NO_QUIET = 1  # FFS_VAD_GATE_NO_QUIET: threshold - dip_bins <= 0, no frame can close a stretch
VAD_GATE_ALL_REJECTED = 2  # FFS_VAD_GATE_ALL_REJECTED: active frames, none kept
VAD_GATE_TOO_LONG = 4  # FFS_VAD_GATE_TOO_LONG: more than VAD_MAX_FRAMES frames, the plain labels
VAD_GATE_TILE = 4096  # frames of one workgroup of the gate's tile kernels (csrc/ffs_vad_gate.h, GATE_TILE)
VAD_GATE_DTYPE = np.dtype(
    [("threshold_bin", "<i4"), ("flags", "<i4"), ("n_stretches", "<i4"), ("n_rejected", "<i4"), ("longest_run", "<i4"),
     ("reserved", "<i4"), ("n_frames", "<i8"), ("n_active", "<i8"), ("n_kept", "<i8")], align=True
)
VAD_GATE_BYTES = 48
assert VAD_GATE_DTYPE.itemsize == VAD_GATE_BYTES
# ffs_vad_centre, the record of the centre gate (include/ffsubsync_amd.h; static size 48 bytes)
VAD_CENTRE_MONO = 1  # FFS_VAD_CENTRE_MONO: no frame has a side level, the file is dual mono
VAD_CENTRE_ALL_REJECTED = 2  # FFS_VAD_CENTRE_ALL_REJECTED: active frames, none kept
VAD_STEREO_MAX_FRAME_VEC = 512  # pairs of the longest frame on the sweep's vector path (csrc/ffs_stereo_vad.h)
VAD_CENTRE_GRID_FRAMES = 256 * 256  # frames of one trip of the centre gate's capped grid (CENTRE_MAX_BLOCKS * CENTRE_THREADS)
VAD_CENTRE_DTYPE = np.dtype(
    [("threshold_bin", "<i4"), ("flags", "<i4"), ("min_contrast_bins", "<i4"), ("max_side", "<i4"), ("n_frames", "<i8"),
     ("n_active", "<i8"), ("n_kept", "<i8"), ("sum_contrast", "<i8")], align=True
)
VAD_CENTRE_BYTES = 48
assert VAD_CENTRE_DTYPE.itemsize == VAD_CENTRE_BYTES
# ffs_prog_state (include/ffsubsync_amd.h; static size 64 bytes)
PROG_STATE_DTYPE = np.dtype(
    [("ref_len", "<i8"), ("offset", "<i8"), ("score", "<f8"), ("mean", "<f8"), ("std", "<f8"), ("runner_up", "<f8"),
     ("other_best", "<f8"), ("best_cand", "<i4"), ("flags", "<i4")], align=True
)
PROG_STATE_BYTES = 64
assert PROG_STATE_DTYPE.itemsize == PROG_STATE_BYTES
PROG_MAX_CAND = 8  # PROG_MAX_CAND (csrc/ffs_progressive.h)
PROG_MAX_LAGS = 262144  # 2W of a slot's lag window, at most
PROG_MAX_INTERVALS = 256  # FFS_PROG_MAX_INTERVALS: merged known intervals of a sampled slot
PROG_PIECE_SAMPLES = 512 * 32  # PROG_PIECE words: the reference samples k_prog_counts stages at a time

# every symbol include/ffsubsync_amd.h declares (checked by tests/test_abi.py)
EXPORTED_SYMBOLS = (
    "ffs_fft_length",
    "ffs_plan_length",
    "ffs_plan_create",
    "ffs_plan_destroy",
    "ffs_plan_workspace_bytes",
    "ffs_align_batch",
    "ffs_align_batch_typed",
    "ffs_align_batch_runs",
    "ffs_runs_list_bytes",
    "ffs_runs_from_bits",
    "ffs_runs_from_bits_batch",
    "ffs_runs_to_bits",
    "ffs_rasterize_batch_runs",
    "ffs_correlate_full",
    "ffs_vad_energy",
    "ffs_vad_energy_bits",
    "ffs_speech_bounds",
    "ffs_vad_tokenize",
    "ffs_raster_length",
    "ffs_raster_intervals",
    "ffs_rasterize_subtitles",
    "ffs_rasterize_subtitles_bits",
    "ffs_raster_lengths",
    "ffs_rasterize_batch_bits",
    "ffs_two_level_pack",
    "ffs_pack_bits",
    "ffs_scatter_segments",
    "ffs_comm_unique_id",
    "ffs_comm_create",
    "ffs_gather_results",
    "ffs_comm_destroy",
    "ffs_plan_set_algorithm",
    "ffs_plan_runs_stats",
    "ffs_plan_dispatch_report",
    "ffs_plan_profile",
    "ffs_plan_profile_read",
    "ffs_split_plan_create",
    "ffs_split_plan_destroy",
    "ffs_split_plan_workspace_bytes",
    "ffs_align_split_batch",
    "ffs_align_split_report_batch",
    "ffs_split_refine_batch",
    "ffs_drift_refine_batch",
    "ffs_cue_report_batch",
    "ffs_cue_retime_batch",
    "ffs_split_range_plan_create",
    "ffs_split_range_plan_destroy",
    "ffs_split_range_plan_workspace_bytes",
    "ffs_align_split_range_batch",
    "ffs_split_range_report_batch",
    "ffs_drift_plan_create",
    "ffs_drift_plan_destroy",
    "ffs_drift_plan_workspace_bytes",
    "ffs_align_drift_batch",
    "ffs_align_drift_report_batch",
    "ffs_align_drift_smooth_batch",
    "ffs_drift_range_plan_create",
    "ffs_drift_range_plan_destroy",
    "ffs_drift_range_plan_workspace_bytes",
    "ffs_align_drift_range_batch",
    "ffs_align_drift_range_smooth_batch",
    "ffs_drift_range_report_batch",
    "ffs_quality_plan_create",
    "ffs_quality_plan_destroy",
    "ffs_quality_plan_workspace_bytes",
    "ffs_align_quality_batch",
    "ffs_match_plan_create",
    "ffs_match_plan_destroy",
    "ffs_match_plan_workspace_bytes",
    "ffs_match_quality_batch",
    "ffs_sweep_peaks",
    "ffs_surrogate_lists",
    "ffs_null_stats",
    "ffs_subsample_lists",
    "ffs_offset_stats",
    "ffs_vad_levels",
    "ffs_vad_level_hist",
    "ffs_vad_pick_threshold",
    "ffs_vad_level_labels",
    "ffs_vad_steady_gate_workspace_bytes",
    "ffs_vad_steady_gate",
    "ffs_vad_stereo_levels",
    "ffs_vad_centre_gate",
    "ffs_prog_plan_create",
    "ffs_prog_plan_destroy",
    "ffs_prog_plan_workspace_bytes",
    "ffs_prog_open",
    "ffs_prog_append",
    "ffs_prog_reference",
    "ffs_prog_close",
    "ffs_prog_open_sampled",
    "ffs_prog_append_at",
    "ffs_prog_known",
    "ffs_prog_plan_sampled_bytes",
    "ffs_last_error",
    "ffs_version",
)
# ffs_dispatch_report: twelve int32 fields, in the header's order
DISPATCH_FIELDS = ("transform_sub_batches", "transform_length", "n1", "n2", "seg_blocks", "half_flags", "pass_a_family",
                   "pass_a_ref_family", "pass_a_paired", "mid_family", "last_family", "sweep_family")
FFS_DISPATCH_PASS_A, FFS_DISPATCH_PASS_A3 = 1, 2
FFS_DISPATCH_MID, FFS_DISPATCH_MID_SEG_ONE_1, FFS_DISPATCH_MID_SEG_ONE_4, FFS_DISPATCH_MID_SEG_PIPE = 1, 2, 3, 4
FFS_DISPATCH_LAST_FULL, FFS_DISPATCH_LAST_C3, FFS_DISPATCH_LAST_PRUNED = 1, 2, 3
KERNEL_NAMES = ("pass_a", "mid", "pass_c", "nominees", "rescore", "runs_extract", "runs_corr", "levels")
FFS_ALGO_AUTO, FFS_ALGO_FFT, FFS_ALGO_RUNS = 0, 1, 2
ALGORITHMS = {"auto": FFS_ALGO_AUTO, "fft": FFS_ALGO_FFT, "runs": FFS_ALGO_RUNS}
FFS_MATCH_AUTO, FFS_MATCH_RUNS, FFS_MATCH_BITS = 0, 1, 2  # ffs_match_quality_batch's `algorithm`
MATCH_ALGORITHMS = {"auto": FFS_MATCH_AUTO, "runs": FFS_MATCH_RUNS, "bits": FFS_MATCH_BITS}


def algorithm_code(algorithm) -> int:
    """FFS_ALGO_* code of "auto" / "fft" / "runs" (any case, surrounding blanks ignored) or of a code itself."""
    if isinstance(algorithm, str):
        name = algorithm.strip().lower()
        if name not in ALGORITHMS:
            raise ValueError("unknown algorithm %r: expected one of %s" % (algorithm, ", ".join(sorted(ALGORITHMS))))
        return ALGORITHMS[name]
    if isinstance(algorithm, (int, np.integer)) and int(algorithm) in ALGORITHMS.values():
        return int(algorithm)
    raise ValueError("unknown algorithm %r: expected one of %s or an FFS_ALGO_* code" % (algorithm, ", ".join(sorted(ALGORITHMS))))


def env_algorithm() -> str:
    """FFS_ALGORITHM of the environment, validated ("auto" when unset or empty)."""
    name = os.environ.get("FFS_ALGORITHM", "").strip().lower() or "auto"
    if name not in ALGORITHMS:
        raise ValueError("FFS_ALGORITHM=%r: expected one of %s" % (os.environ.get("FFS_ALGORITHM"), ", ".join(sorted(ALGORITHMS))))
    return name


class NativeError(RuntimeError):
    """A call into libffsalign.so returned a negative FFS_E_* code."""

    def __init__(self, code: int, message: str) -> None:
        super().__init__("libffsalign error %d: %s" % (code, message))
        self.code = code


def library_path() -> str:
    """In-tree libffsalign.so; FFS_LIBRARY_PATH selects another build of it (A/B runs of compile-time variants)."""
    return os.environ.get("FFS_LIBRARY_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), _LIB_NAME)


def load():
    """Load the shared library once; raise ImportError loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        path = library_path()
        if not os.path.exists(path):
            raise ImportError(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C ffsubsync_amd/csrc` (hipcc --offload-arch=gfx950). "
                "There is no CPU fallback." % path
            )
        # torch first: its wheel bundles a HIP runtime (libamdhip64) with the same SONAME the library links
        # against.  Loaded in that order both share one runtime; the other way round the process ends
        # up with two, and the second one finds no device ("no ROCm-capable device is detected").
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = ctypes.CDLL(path)
        c = ctypes
        lib.ffs_fft_length.restype = c.c_int64
        lib.ffs_fft_length.argtypes = [c.c_int64, c.c_int64]
        lib.ffs_plan_length.restype = c.c_int64
        lib.ffs_plan_length.argtypes = [c.c_int64, c.c_int64, c.c_int64]
        lib.ffs_plan_create.restype = c.c_int
        lib.ffs_plan_create.argtypes = [c.c_int, c.c_int64, c.c_int, c.c_int, c.POINTER(c.c_void_p)]
        lib.ffs_plan_destroy.restype = c.c_int
        lib.ffs_plan_destroy.argtypes = [c.c_void_p]
        lib.ffs_plan_workspace_bytes.restype = c.c_int64
        lib.ffs_plan_workspace_bytes.argtypes = [c.c_void_p]
        lib.ffs_align_batch.restype = c.c_int
        lib.ffs_align_batch.argtypes = [
            c.c_void_p, c.c_int, c.c_int, c.c_int,
            c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
            c.c_int64, c.c_int64, c.c_void_p, c.c_void_p, c.c_void_p,
        ]
        lib.ffs_align_batch_typed.restype = c.c_int
        lib.ffs_align_batch_typed.argtypes = [
            c.c_void_p, c.c_int, c.c_int, c.c_void_p,
            c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
            c.c_int64, c.c_int64, c.c_void_p, c.c_void_p, c.c_void_p,
        ]
        lib.ffs_align_batch_runs.restype = c.c_int
        lib.ffs_align_batch_runs.argtypes = [
            c.c_void_p, c.c_int, c.c_int, c.c_void_p,
            c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
            c.c_int64, c.c_int64, c.c_void_p, c.c_void_p, c.c_void_p,
        ]
        lib.ffs_runs_list_bytes.restype = c.c_int64
        lib.ffs_runs_list_bytes.argtypes = [c.c_int64]
        lib.ffs_runs_from_bits.restype = c.c_int
        lib.ffs_runs_from_bits.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_void_p]
        lib.ffs_runs_from_bits_batch.restype = c.c_int
        lib.ffs_runs_from_bits_batch.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p]
        lib.ffs_runs_to_bits.restype = c.c_int
        lib.ffs_runs_to_bits.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p]
        lib.ffs_rasterize_batch_runs.restype = c.c_int
        lib.ffs_rasterize_batch_runs.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p,
                                                 c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_double,
                                                 c.c_double, c.c_void_p, c.c_int64, c.c_void_p]
        lib.ffs_correlate_full.restype = c.c_int
        lib.ffs_correlate_full.argtypes = [
            c.c_void_p, c.c_int,
            c.c_void_p, c.c_int64, c.c_double, c.c_double,
            c.c_void_p, c.c_int64, c.c_double, c.c_double,
            c.c_void_p, c.c_int64, c.c_double, c.c_double,
            c.c_void_p, c.c_void_p, c.c_void_p,
        ]
        lib.ffs_vad_energy.restype = c.c_int
        lib.ffs_vad_energy.argtypes = [c.c_void_p, c.c_int64, c.c_int, c.c_double, c.c_float, c.c_void_p, c.c_void_p]
        lib.ffs_vad_energy_bits.restype = c.c_int
        lib.ffs_vad_energy_bits.argtypes = [c.c_void_p, c.c_int64, c.c_int, c.c_double, c.c_void_p, c.c_void_p]
        lib.ffs_vad_tokenize.restype = c.c_int
        lib.ffs_vad_tokenize.argtypes = [c.c_void_p, c.c_int64, c.c_int64, c.c_int, c.c_int, c.c_int, c.c_float,
                                         c.c_void_p, c.c_void_p]
        lib.ffs_vad_levels.restype = c.c_int
        lib.ffs_vad_levels.argtypes = [c.c_void_p, c.c_int64, c.c_int, c.c_void_p, c.c_int, c.c_void_p, c.c_void_p]
        lib.ffs_vad_level_hist.restype = c.c_int
        lib.ffs_vad_level_hist.argtypes = [c.c_void_p, c.c_int64, c.c_int, c.c_void_p, c.c_void_p]
        lib.ffs_vad_pick_threshold.restype = c.c_int
        lib.ffs_vad_pick_threshold.argtypes = [c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int,
                                               c.c_int, c.c_void_p, c.c_void_p]
        lib.ffs_vad_level_labels.restype = c.c_int
        lib.ffs_vad_level_labels.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_int, c.c_float, c.c_void_p, c.c_void_p,
                                             c.c_void_p]
        lib.ffs_vad_steady_gate_workspace_bytes.restype = c.c_int64
        lib.ffs_vad_steady_gate_workspace_bytes.argtypes = [c.c_int64]
        lib.ffs_vad_steady_gate.restype = c.c_int
        lib.ffs_vad_steady_gate.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_int, c.c_int, c.c_int64, c.c_float, c.c_void_p,
                                            c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p]
        lib.ffs_vad_stereo_levels.restype = c.c_int
        lib.ffs_vad_stereo_levels.argtypes = [c.c_void_p, c.c_int64, c.c_int, c.c_void_p, c.c_int, c.c_void_p, c.c_void_p,
                                              c.c_void_p]
        lib.ffs_vad_centre_gate.restype = c.c_int
        lib.ffs_vad_centre_gate.argtypes = [c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p, c.c_int, c.c_int, c.c_void_p,
                                            c.c_void_p, c.c_void_p]
        lib.ffs_speech_bounds.restype = c.c_int
        lib.ffs_speech_bounds.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p]
        lib.ffs_raster_length.restype = c.c_int64
        lib.ffs_raster_length.argtypes = [c.c_void_p, c.c_int64, c.c_double, c.c_double]
        lib.ffs_raster_intervals.restype = c.c_int64
        lib.ffs_raster_intervals.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_double, c.c_double,
                                             c.c_double, c.c_int64, c.c_void_p]
        lib.ffs_rasterize_subtitles.restype = c.c_int
        lib.ffs_rasterize_subtitles.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_double, c.c_double,
                                                c.c_double, c.c_void_p, c.c_int64, c.c_void_p]
        lib.ffs_rasterize_subtitles_bits.restype = c.c_int
        lib.ffs_rasterize_subtitles_bits.argtypes = lib.ffs_rasterize_subtitles.argtypes
        lib.ffs_raster_lengths.restype = c.c_int
        lib.ffs_raster_lengths.argtypes = [c.c_void_p, c.c_void_p, c.c_int64, c.c_double, c.c_void_p]
        lib.ffs_two_level_pack.restype = c.c_int
        lib.ffs_two_level_pack.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p, c.c_void_p]
        lib.ffs_rasterize_batch_bits.restype = c.c_int
        lib.ffs_rasterize_batch_bits.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p,
                                                 c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_double, c.c_double,
                                                 c.c_void_p, c.c_int64, c.c_void_p]
        lib.ffs_pack_bits.restype = c.c_int
        lib.ffs_pack_bits.argtypes = [c.c_void_p, c.c_int, c.c_int64, c.c_double, c.c_void_p, c.c_void_p]
        lib.ffs_scatter_segments.restype = c.c_int
        lib.ffs_scatter_segments.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_void_p, c.c_int64,
                                             c.c_void_p]
        lib.ffs_comm_unique_id.restype = c.c_int
        lib.ffs_comm_unique_id.argtypes = [c.c_void_p]
        lib.ffs_comm_create.restype = c.c_int
        lib.ffs_comm_create.argtypes = [c.c_int, c.c_int, c.c_int, c.c_void_p, c.POINTER(c.c_void_p)]
        lib.ffs_gather_results.restype = c.c_int
        lib.ffs_gather_results.argtypes = [c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p]
        lib.ffs_comm_destroy.restype = c.c_int
        lib.ffs_comm_destroy.argtypes = [c.c_void_p]
        lib.ffs_plan_set_algorithm.restype = c.c_int
        lib.ffs_plan_set_algorithm.argtypes = [c.c_void_p, c.c_int]
        lib.ffs_plan_runs_stats.restype = c.c_int
        lib.ffs_plan_runs_stats.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
        lib.ffs_plan_dispatch_report.restype = c.c_int
        lib.ffs_plan_dispatch_report.argtypes = [c.c_void_p, c.c_void_p]
        lib.ffs_plan_profile.restype = c.c_int
        lib.ffs_plan_profile.argtypes = [c.c_void_p, c.c_int]
        lib.ffs_plan_profile_read.restype = c.c_int
        lib.ffs_plan_profile_read.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p]
        lib.ffs_split_plan_create.restype = c.c_int
        lib.ffs_split_plan_create.argtypes = [c.c_int, c.c_int, c.c_int64, c.c_int64, c.c_int64, c.POINTER(c.c_void_p)]
        lib.ffs_split_plan_destroy.restype = c.c_int
        lib.ffs_split_plan_destroy.argtypes = [c.c_void_p]
        lib.ffs_split_plan_workspace_bytes.restype = c.c_int64
        lib.ffs_split_plan_workspace_bytes.argtypes = [c.c_void_p]
        lib.ffs_align_split_batch.restype = c.c_int
        lib.ffs_align_split_batch.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                              c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64,
                                              c.c_double, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
        lib.ffs_align_split_report_batch.restype = c.c_int
        lib.ffs_align_split_report_batch.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                                     c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64,
                                                     c.c_double, c.c_int, c.c_int64, c.c_void_p, c.c_void_p, c.c_void_p,
                                                     c.c_void_p, c.c_void_p, c.c_void_p]
        lib.ffs_split_refine_batch.restype = c.c_int
        lib.ffs_split_refine_batch.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                               c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p,
                                               c.c_int64, c.c_double, c.c_void_p, c.c_void_p, c.c_void_p]
        lib.ffs_cue_report_batch.restype = c.c_int
        lib.ffs_cue_report_batch.argtypes = [c.c_void_p, c.c_int] + [c.c_void_p] * 8 + [
            c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_void_p, c.c_void_p]
        lib.ffs_cue_retime_batch.restype = c.c_int
        lib.ffs_cue_retime_batch.argtypes = [c.c_void_p, c.c_int] + [c.c_void_p] * 8 + [
            c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int64, c.c_int64, c.c_int,
            c.c_void_p, c.c_void_p, c.c_void_p]
        lib.ffs_drift_refine_batch.restype = c.c_int
        lib.ffs_drift_refine_batch.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                               c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p,
                                               c.c_void_p, c.c_int64, c.c_double, c.c_void_p, c.c_void_p, c.c_void_p]
        lib.ffs_split_range_plan_create.restype = c.c_int
        lib.ffs_split_range_plan_create.argtypes = [c.c_int, c.c_int, c.c_int64, c.c_int64, c.c_int64,
                                                    c.POINTER(c.c_void_p)]
        lib.ffs_split_range_plan_destroy.restype = c.c_int
        lib.ffs_split_range_plan_destroy.argtypes = [c.c_void_p]
        lib.ffs_split_range_plan_workspace_bytes.restype = c.c_int64
        lib.ffs_split_range_plan_workspace_bytes.argtypes = [c.c_void_p]
        lib.ffs_align_split_range_batch.restype = c.c_int
        lib.ffs_align_split_range_batch.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                                    c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p,
                                                    c.c_void_p, c.c_double, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
        lib.ffs_split_range_report_batch.restype = c.c_int
        lib.ffs_split_range_report_batch.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                                     c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p,
                                                     c.c_void_p, c.c_void_p, c.c_int, c.c_int64, c.c_void_p, c.c_void_p,
                                                     c.c_void_p]
        lib.ffs_drift_plan_create.restype = c.c_int
        lib.ffs_drift_plan_create.argtypes = [c.c_int, c.c_int, c.c_int64, c.c_int64, c.c_int64, c.POINTER(c.c_void_p)]
        lib.ffs_drift_plan_destroy.restype = c.c_int
        lib.ffs_drift_plan_destroy.argtypes = [c.c_void_p]
        lib.ffs_drift_plan_workspace_bytes.restype = c.c_int64
        lib.ffs_drift_plan_workspace_bytes.argtypes = [c.c_void_p]
        lib.ffs_align_drift_batch.restype = c.c_int
        lib.ffs_align_drift_batch.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                              c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64,
                                              c.c_double, c.c_int, c.c_double, c.c_void_p, c.c_void_p, c.c_void_p,
                                              c.c_void_p, c.c_void_p]
        lib.ffs_align_drift_report_batch.restype = c.c_int
        lib.ffs_align_drift_report_batch.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                                     c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64,
                                                     c.c_double, c.c_int, c.c_double, c.c_int, c.c_int64, c.c_void_p,
                                                     c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                                     c.c_void_p]
        lib.ffs_align_drift_smooth_batch.restype = c.c_int
        lib.ffs_align_drift_smooth_batch.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                                     c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64,
                                                     c.c_double, c.c_int, c.c_double, c.c_int, c.c_int, c.c_double,
                                                     c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                                     c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
        lib.ffs_drift_range_plan_create.restype = c.c_int
        lib.ffs_drift_range_plan_create.argtypes = [c.c_int, c.c_int, c.c_int64, c.c_int64, c.c_int64, c.c_int,
                                                    c.POINTER(c.c_void_p)]
        lib.ffs_drift_range_plan_destroy.restype = c.c_int
        lib.ffs_drift_range_plan_destroy.argtypes = [c.c_void_p]
        lib.ffs_drift_range_plan_workspace_bytes.restype = c.c_int64
        lib.ffs_drift_range_plan_workspace_bytes.argtypes = [c.c_void_p]
        lib.ffs_align_drift_range_batch.restype = c.c_int
        lib.ffs_align_drift_range_batch.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                                    c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p,
                                                    c.c_void_p, c.c_double, c.c_int, c.c_double, c.c_void_p, c.c_void_p,
                                                    c.c_void_p, c.c_void_p, c.c_void_p]
        lib.ffs_align_drift_range_smooth_batch.restype = c.c_int
        lib.ffs_align_drift_range_smooth_batch.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p,
                                                           c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                                           c.c_int64, c.c_void_p, c.c_void_p, c.c_double, c.c_int,
                                                           c.c_double, c.c_int, c.c_int, c.c_double, c.c_void_p,
                                                           c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                                           c.c_void_p, c.c_void_p, c.c_void_p]
        lib.ffs_drift_range_report_batch.restype = c.c_int
        lib.ffs_drift_range_report_batch.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                                     c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p,
                                                     c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_int64, c.c_void_p,
                                                     c.c_void_p, c.c_void_p]
        lib.ffs_quality_plan_create.restype = c.c_int
        lib.ffs_quality_plan_create.argtypes = [c.c_int, c.c_int, c.c_int64, c.c_int64, c.POINTER(c.c_void_p)]
        lib.ffs_quality_plan_destroy.restype = c.c_int
        lib.ffs_quality_plan_destroy.argtypes = [c.c_void_p]
        lib.ffs_quality_plan_workspace_bytes.restype = c.c_int64
        lib.ffs_quality_plan_workspace_bytes.argtypes = [c.c_void_p]
        lib.ffs_align_quality_batch.restype = c.c_int
        lib.ffs_align_quality_batch.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                                c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int,
                                                c.c_int64, c.c_void_p, c.c_void_p]
        lib.ffs_match_plan_create.restype = c.c_int
        lib.ffs_match_plan_create.argtypes = [c.c_int, c.c_int, c.c_int64, c.c_int64, c.c_int64, c.POINTER(c.c_void_p)]
        lib.ffs_match_plan_destroy.restype = c.c_int
        lib.ffs_match_plan_destroy.argtypes = [c.c_void_p]
        lib.ffs_match_plan_workspace_bytes.restype = c.c_int64
        lib.ffs_match_plan_workspace_bytes.argtypes = [c.c_void_p]
        lib.ffs_match_quality_batch.restype = c.c_int
        lib.ffs_match_quality_batch.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                                c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int,
                                                c.c_void_p, c.c_void_p, c.c_int64, c.c_int, c.c_int64, c.c_int,
                                                c.c_void_p, c.c_void_p]
        lib.ffs_sweep_peaks.restype = c.c_int
        lib.ffs_sweep_peaks.argtypes = [c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_int64, c.c_void_p, c.c_void_p]
        lib.ffs_surrogate_lists.restype = c.c_int
        lib.ffs_surrogate_lists.argtypes = [c.c_void_p] * 5 + [c.c_int64, c.c_int, c.c_int, c.c_void_p, c.c_int64,
                                                                c.c_void_p, c.c_void_p]
        lib.ffs_null_stats.restype = c.c_int
        lib.ffs_null_stats.argtypes = [c.c_void_p, c.c_int, c.c_int, c.c_void_p, c.c_void_p]
        lib.ffs_subsample_lists.restype = c.c_int
        lib.ffs_subsample_lists.argtypes = lib.ffs_surrogate_lists.argtypes
        lib.ffs_offset_stats.restype = c.c_int
        lib.ffs_offset_stats.argtypes = [c.c_void_p, c.c_int, c.c_int, c.c_int64, c.c_void_p, c.c_void_p]
        lib.ffs_prog_plan_create.restype = c.c_int
        lib.ffs_prog_plan_create.argtypes = [c.c_int, c.c_int, c.c_int, c.c_int64, c.c_int64, c.c_int64, c.POINTER(c.c_void_p)]
        lib.ffs_prog_plan_destroy.restype = c.c_int
        lib.ffs_prog_plan_destroy.argtypes = [c.c_void_p]
        lib.ffs_prog_plan_workspace_bytes.restype = c.c_int64
        lib.ffs_prog_plan_workspace_bytes.argtypes = [c.c_void_p]
        lib.ffs_prog_open.restype = c.c_int
        lib.ffs_prog_open.argtypes = [c.c_void_p, c.c_int] + [c.c_void_p] * 10
        lib.ffs_prog_append.restype = c.c_int
        lib.ffs_prog_append.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int,
                                        c.c_int64, c.c_void_p, c.c_void_p, c.c_void_p]
        lib.ffs_prog_reference.restype = c.c_int
        lib.ffs_prog_reference.argtypes = [c.c_void_p, c.c_int, c.POINTER(c.c_void_p), c.POINTER(c.c_int64)]
        lib.ffs_prog_close.restype = c.c_int
        lib.ffs_prog_close.argtypes = [c.c_void_p, c.c_int, c.c_void_p]
        lib.ffs_prog_open_sampled.restype = c.c_int
        lib.ffs_prog_open_sampled.argtypes = [c.c_void_p, c.c_int] + [c.c_void_p] * 11
        lib.ffs_prog_append_at.restype = c.c_int
        lib.ffs_prog_append_at.argtypes = [c.c_void_p, c.c_int] + [c.c_void_p] * 5 + [c.c_int, c.c_int64, c.c_void_p,
                                                                                     c.c_void_p, c.c_void_p]
        lib.ffs_prog_known.restype = c.c_int
        lib.ffs_prog_known.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_int, c.POINTER(c.c_int)]
        lib.ffs_prog_plan_sampled_bytes.restype = c.c_int64
        lib.ffs_prog_plan_sampled_bytes.argtypes = [c.c_void_p]
        lib.ffs_last_error.restype = c.c_char_p
        lib.ffs_last_error.argtypes = []
        lib.ffs_version.restype = c.c_int
        lib.ffs_version.argtypes = []
        _lib = lib
        return _lib


def check(code: int) -> None:
    if code != 0:
        raise NativeError(code, load().ffs_last_error().decode("utf-8", "replace"))


def fft_length(ref_len: int, sub_len: int) -> int:
    return int(load().ffs_fft_length(int(ref_len), int(sub_len)))


def plan_length(ref_len: int, sub_len: int, max_offset_samples: Optional[int]) -> int:
    """Transform length the device needs: the reference's N without a lag window, possibly shorter
    (alias-free for the windowed lags) with one."""
    mo = -1 if max_offset_samples is None else int(max_offset_samples)
    return int(load().ffs_plan_length(int(ref_len), int(sub_len), mo))


_gpu_seen = None  # torch, once a device has been seen (torch.cuda.is_available() costs ~2.5 us a call, three per solve)


def require_gpu():
    """Return torch after checking a HIP device is visible (the product path needs one)."""
    global _gpu_seen
    if _gpu_seen is not None:
        return _gpu_seen
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError(
            "ffsubsync_amd needs an AMD Instinct GPU (ROCm/HIP device) -- none is visible and there is no CPU fallback"
        )
    _gpu_seen = torch
    return torch


def current_stream_ptr(torch) -> int:
    """Raw hipStream_t of torch's current stream on the current device."""
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    if raw is not None:  # (no Stream object: ~1 us instead of ~7)
        return int(raw(torch.cuda.current_device()))
    return int(torch.cuda.current_stream().cuda_stream)


class Plan:
    """Owns one ``ffs_plan`` (twiddle tables + HBM workspace for one transform length)."""

    def __init__(self, n_fft: int, pairs_in_flight: int = 2, max_cand: int = 8, device: Optional[int] = None) -> None:
        torch = require_gpu()
        self.lib = load()
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.n_fft = int(n_fft)
        self.pairs_in_flight = int(pairs_in_flight)
        self.max_cand = int(max_cand)
        handle = ctypes.c_void_p()
        check(self.lib.ffs_plan_create(self.device, self.n_fft, self.pairs_in_flight, self.max_cand, ctypes.byref(handle)))
        self.handle = handle

    @property
    def workspace_bytes(self) -> int:
        return int(self.lib.ffs_plan_workspace_bytes(self.handle))

    def set_algorithm(self, algorithm, _from_env: bool = False) -> None:
        """"auto" (default: run-boundary path for short boundary lists, transforms otherwise), "fft" (transforms only) or
        "runs" (run-boundary path without the coincidence budget); identical results either way.  The choice belongs to
        whoever owns the plan: a plan obtained from ``get_plan`` (a per-thread cache shared between callers) gets
        FFS_ALGORITHM re-applied at every hand-out."""
        check(self.lib.ffs_plan_set_algorithm(self.handle, algorithm_code(algorithm)))
        if not _from_env:
            self._algorithm_explicit = True

    def runs_stats(self):
        """(calls that tried the run-boundary path, their sub-batches, sub-batches that went through the transforms)."""
        v = (ctypes.c_int64 * 4)()
        check(self.lib.ffs_plan_runs_stats(self.handle, ctypes.byref(v, 0), ctypes.byref(v, 8), ctypes.byref(v, 16), None))
        return int(v[0]), int(v[1]), int(v[2])

    def runs_boundaries_last_call(self) -> int:
        """Boundary-list entries of all vectors of the most recent run-boundary call."""
        v = ctypes.c_int64()
        check(self.lib.ffs_plan_runs_stats(self.handle, None, None, None, ctypes.byref(v)))
        return int(v.value)

    def dispatch_report(self) -> dict:
        """What the most recent solve launched for its transform sub-batches (``ffs_plan_dispatch_report``): a dict of
        DISPATCH_FIELDS, all zero when nothing went through the transforms."""
        v = (ctypes.c_int32 * len(DISPATCH_FIELDS))()
        check(self.lib.ffs_plan_dispatch_report(self.handle, ctypes.byref(v)))
        return {k: int(v[i]) for i, k in enumerate(DISPATCH_FIELDS)}

    def profile(self, enable: bool) -> None:
        check(self.lib.ffs_plan_profile(self.handle, 1 if enable else 0))

    def profile_read(self):
        """{kernel name: (total ms, launches)} accumulated since the last read (synchronises)."""
        ms = np.zeros(len(KERNEL_NAMES), dtype=np.float64)
        n = np.zeros(len(KERNEL_NAMES), dtype=np.int64)
        check(self.lib.ffs_plan_profile_read(self.handle, ms.ctypes.data, n.ctypes.data))
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(KERNEL_NAMES)}

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.ffs_plan_destroy(self.handle)
            self.handle = None

    def __del__(self) -> None:  # pragma: no cover - interpreter shutdown ordering
        try:
            self.close()
        except Exception:
            pass

    def align_batch(self, n_pairs: int, n_cand: int, dtype, vec_ptr: np.ndarray, vec_len: np.ndarray,
                    vec_lo: np.ndarray, vec_hi: np.ndarray, max_offset_samples: Optional[int],
                    filter_max_offset: Optional[int], cand_out, pair_out, stream: Optional[int] = None,
                    vec_max_boundaries: Optional[np.ndarray] = None) -> None:
        """Asynchronous batched solve; ``cand_out``/``pair_out`` are uint8 CUDA tensors of
        n_pairs*n_cand*24 and n_pairs*24 bytes.  Host arrays are consumed before returning.
        ``dtype``: one FFS_DTYPE_* for every vector, or a (reference type, candidate type) tuple / an array with one
        entry per vector (``ffs_align_batch_runs``: e.g. a float64 reference against bit-packed candidates, or
        boundary lists, FFS_DTYPE_RUNS).  ``vec_max_boundaries``: host-known upper bounds of the lists' lengths (int32 per
        vector, 0 = unknown): with all of them known and within the coincidence budget the call does not wait for the
        device."""
        torch = require_gpu()
        n_vec = n_pairs * (1 + n_cand)
        vec_ptr = np.ascontiguousarray(vec_ptr, dtype=np.uint64)
        vec_len = np.ascontiguousarray(vec_len, dtype=np.int64)
        vec_lo = np.ascontiguousarray(vec_lo, dtype=np.float64)
        vec_hi = np.ascontiguousarray(vec_hi, dtype=np.float64)
        if not (vec_ptr.size == vec_len.size == vec_lo.size == vec_hi.size == n_vec):
            raise ValueError("descriptor arrays must have n_pairs*(1+n_cand) entries")
        if cand_out.numel() * cand_out.element_size() < n_pairs * n_cand * 24 or \
                pair_out.numel() * pair_out.element_size() < n_pairs * 24:
            raise ValueError("result buffers too small")
        st = current_stream_ptr(torch) if stream is None else stream
        if not isinstance(dtype, (int, np.integer)):
            if isinstance(dtype, tuple) and len(dtype) == 2:
                dtype = np.tile(np.array([dtype[0]] + [dtype[1]] * n_cand, dtype=np.int32), n_pairs)
            vec_dtype = np.ascontiguousarray(dtype, dtype=np.int32)
            if vec_dtype.size != n_vec:
                raise ValueError("one element type per vector")
            bound = None
            if vec_max_boundaries is not None:
                bound = np.ascontiguousarray(vec_max_boundaries, dtype=np.int32)
                if bound.size != n_vec:
                    raise ValueError("one boundary bound per vector")
            check(self.lib.ffs_align_batch_runs(
                self.handle, n_pairs, n_cand, vec_dtype.ctypes.data,
                vec_ptr.ctypes.data, vec_len.ctypes.data, vec_lo.ctypes.data, vec_hi.ctypes.data,
                None if bound is None else bound.ctypes.data,
                -1 if max_offset_samples is None else int(max_offset_samples),
                -1 if filter_max_offset is None else int(filter_max_offset),
                cand_out.data_ptr(), pair_out.data_ptr(), st,
            ))
            return
        check(self.lib.ffs_align_batch(
            self.handle, n_pairs, n_cand, int(dtype),
            vec_ptr.ctypes.data, vec_len.ctypes.data, vec_lo.ctypes.data, vec_hi.ctypes.data,
            -1 if max_offset_samples is None else int(max_offset_samples),
            -1 if filter_max_offset is None else int(filter_max_offset),
            cand_out.data_ptr(), pair_out.data_ptr(), st,
        ))

    def correlate_full(self, dtype: int, ref, ref_levels, a, a_levels, b=None, b_levels=(0.0, 1.0), lens=None):
        """Raw fp32 correlation arrays out_a[m], out_b[m] (m = lag mod n_fft) as CUDA tensors.  ``lens`` =
        (R, Sa[, Sb]) in samples when the tensors are bit-packed (default: the tensors' element counts)."""
        torch = require_gpu()
        out_a = torch.empty(self.n_fft, dtype=torch.float32, device=ref.device)
        out_b = torch.empty(self.n_fft, dtype=torch.float32, device=ref.device) if b is not None else None
        n_ref, n_a = (ref.numel(), a.numel()) if lens is None else (int(lens[0]), int(lens[1]))
        n_b = 0 if b is None else (b.numel() if lens is None else int(lens[2]))
        check(self.lib.ffs_correlate_full(
            self.handle, dtype,
            ref.data_ptr(), n_ref, float(ref_levels[0]), float(ref_levels[1]),
            a.data_ptr(), n_a, float(a_levels[0]), float(a_levels[1]),
            b.data_ptr() if b is not None else None, n_b,
            float(b_levels[0]), float(b_levels[1]),
            out_a.data_ptr(), out_b.data_ptr() if out_b is not None else None, current_stream_ptr(torch),
        ))
        return out_a, out_b


class _PlanCache(threading.local):
    """Per-thread plan cache (a plan may be driven by one host thread at a time; the reference runs
    detectors/aligners from a small thread pool, speech_transformers.py:872-873).  Thread-local storage
    dies with its thread, so a worker that exits releases its plans (``Plan.__del__`` destroys them);
    within a thread the cache is an LRU bounded by an HBM budget."""

    def __init__(self) -> None:
        self.plans: "Dict[Tuple[int, int, int, int], Plan]" = {}
        self.order: list = []


_plan_cache = _PlanCache()
PLAN_CACHE_BYTES = int(os.environ.get("FFS_PLAN_CACHE_BYTES", str(8 << 30)))  # per thread


def get_plan(n_fft: int, pairs_in_flight: int = 1, max_cand: int = 8, device: Optional[int] = None) -> Plan:
    """Cached plan for (device, n_fft, pairs_in_flight, max_cand) of the calling thread."""
    torch = require_gpu()
    dev = torch.cuda.current_device() if device is None else int(device)
    key = (dev, int(n_fft), int(pairs_in_flight), int(max_cand))
    cache = _plan_cache
    plan = cache.plans.get(key)
    if plan is not None and getattr(plan, "handle", None) is None:  # closed behind the cache's back: forget it
        del cache.plans[key]
        cache.order.remove(key)
        plan = None
    if plan is None:
        plan = Plan(n_fft, pairs_in_flight, max_cand, dev)  # hipMalloc + table upload: no lock held
        cache.plans[key] = plan
    else:
        cache.order.remove(key)
    cache.order.append(key)
    # Cached plans are SHARED between unrelated callers of the thread: every hand-out re-applies FFS_ALGORITHM (auto | fft |
    # runs; results are identical either way), so a Plan.set_algorithm() by one user of a cached plan lasts until the next
    # get_plan() for that key and never leaks into another caller's solves.  To pin an algorithm, own the plan
    # (``Plan(...)`` / ``BatchAligner(algorithm=...)``).
    plan.set_algorithm(env_algorithm(), _from_env=True)
    plan._algorithm_explicit = False
    # evict least recently used plans beyond the budget (never the one just asked for)
    total = sum(p.workspace_bytes for p in cache.plans.values())
    while total > PLAN_CACHE_BYTES and len(cache.order) > 1:
        old = cache.order.pop(0)
        victim = cache.plans.pop(old)
        total -= victim.workspace_bytes
        victim.close()
    return plan


def clear_plan_cache() -> None:
    """Destroy the calling thread's cached plans (frees their HBM)."""
    for plan in _plan_cache.plans.values():
        plan.close()
    _plan_cache.plans.clear()
    _plan_cache.order.clear()


def vad_energy(pcm, frame_len: int, threshold_db: float, non_speech_label: float):
    """labels (float32 CUDA tensor) for an int16 CUDA tensor of mono PCM."""
    torch = require_gpu()
    n = pcm.numel()
    n_frames = (n + frame_len - 1) // frame_len
    labels = torch.empty(n_frames, dtype=torch.float32, device=pcm.device)
    if n:
        check(load().ffs_vad_energy(pcm.data_ptr(), n, int(frame_len), float(threshold_db), float(non_speech_label),
                                    labels.data_ptr(), current_stream_ptr(torch)))
    return labels


def vad_energy_bits(pcm, frame_len: int, threshold_db: float, out=None, first_frame: int = 0):
    """Bit-packed labels (int32 CUDA words, FFS_DTYPE_U1 order) for an int16 CUDA tensor of mono PCM.
    ``out`` / ``first_frame``: write into an existing zero-initialised word tensor at a frame offset that is a
    multiple of 8 (chunk-by-chunk sweeps of one file); returns (words, n_frames)."""
    torch = require_gpu()
    n = pcm.numel()
    n_frames = (n + frame_len - 1) // frame_len
    if first_frame % 8:
        raise ValueError("first_frame must be a multiple of 8")
    if out is None:
        out = torch.zeros((first_frame + n_frames + 31) // 32, dtype=torch.int32, device=pcm.device)
    elif out.numel() * out.element_size() * 8 < first_frame + n_frames:
        raise ValueError("output word buffer too small")
    elif out.device != pcm.device or not out.is_contiguous():
        raise ValueError("output word buffer must be contiguous and on the PCM's device")
    if n:
        check(load().ffs_vad_energy_bits(pcm.data_ptr(), n, int(frame_len), float(threshold_db),
                                         out.data_ptr() + first_frame // 8, current_stream_ptr(torch)))
    return out, n_frames


def vad_tokenize(valid, chunk_frames: int, min_length: int, max_length: int, max_continuous_silence: int,
                 non_speech_label: float):
    """auditok-style token smoothing of a float32 CUDA validity vector (see ffs_vad_tokenize)."""
    torch = require_gpu()
    out = torch.empty_like(valid)
    if valid.numel():
        check(load().ffs_vad_tokenize(valid.data_ptr(), valid.numel(), int(chunk_frames), int(math.ceil(min_length)),
                                      int(max_length), int(math.ceil(max_continuous_silence)), float(non_speech_label), out.data_ptr(),
                                      current_stream_ptr(torch)))
    return out


def speech_bounds(frames):
    """(first, last) index with frames > 0.5 for a float32 CUDA tensor, or (None, None)."""
    torch = require_gpu()
    out = torch.empty(2, dtype=torch.int64, device=frames.device)
    check(load().ffs_speech_bounds(frames.data_ptr() if frames.numel() else None, frames.numel(), out.data_ptr(),
                                   current_stream_ptr(torch)))
    lo, hi = (int(v) for v in out.cpu())
    return (None, None) if hi < 0 else (lo, hi)


def _record_out(out, torch, n_files: int, record_bytes: int, device):
    """The output buffer of a per-file reduction: ``out`` if it holds n_files records, else a fresh uint8 tensor."""
    if out is None:
        return torch.empty(max(n_files, 1) * record_bytes, dtype=torch.uint8, device=device)
    if _nbytes(out) < n_files * record_bytes:
        raise ValueError("output buffer too small")
    return out


def sweep_peaks(records, first, n_files: int, top_k: int, exclusion_steps: int, out=None):
    """``ffs_sweep_peaks`` on the current stream: ``records`` a CUDA tensor of ffs_cand_result records (24 bytes each),
    ``first`` an int64 CUDA tensor of n_files + 1 ascending point indices; returns the uint8 CUDA tensor of n_files
    ``SWEEP_PROFILE_DTYPE`` records (``out``, if given, is written in place)."""
    torch = require_gpu()
    n_files = int(n_files)
    if first.dtype != torch.int64 or first.numel() < n_files + 1 or not first.is_contiguous():
        raise ValueError("first must be a contiguous int64 tensor of n_files + 1 entries")
    out = _record_out(out, torch, n_files, SWEEP_PROFILE_BYTES, first.device)
    check(load().ffs_sweep_peaks(records.data_ptr(), first.data_ptr(), n_files, int(top_k), int(exclusion_steps),
                                 out.data_ptr(), current_stream_ptr(torch)))
    return out


def _resampled_lists(fn, list_ptr, n_bound, seeds, out_off, out_cap, k: int, block: int, out, status) -> None:
    """The list export named ``fn`` (``ffs_surrogate_lists`` / ``ffs_subsample_lists``: the same argument shapes) on the
    current stream."""
    torch = require_gpu()
    list_ptr = np.ascontiguousarray(list_ptr, dtype=np.uint64)
    n_bound = np.ascontiguousarray(n_bound, dtype=np.int32)
    seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
    out_off = np.ascontiguousarray(out_off, dtype=np.int64)
    out_cap = np.ascontiguousarray(out_cap, dtype=np.int64)
    n_vec = list_ptr.size
    if not (n_bound.size == seeds.size == out_off.size == out_cap.size == n_vec):
        raise ValueError("the vector tables must have the same length")
    if status.dtype != torch.int32 or status.numel() < n_vec or not status.is_contiguous():
        raise ValueError("status must be a contiguous int32 tensor with one entry per vector")
    check(getattr(load(), fn)(list_ptr.ctypes.data, n_bound.ctypes.data, seeds.ctypes.data, out_off.ctypes.data,
                              out_cap.ctypes.data, n_vec, int(k), int(block), out.data_ptr(), _nbytes(out), status.data_ptr(),
                              current_stream_ptr(torch)))


def _record_stats(fn, records, n_files: int, k: int, record_bytes: int, what: str, *extra, out=None):
    """The reduction named ``fn`` (``ffs_null_stats`` / ``ffs_offset_stats``) of n_files * (k + 1) solve records on the
    current stream; ``extra``: its arguments between k and the output, ``what``: the name of k in the message."""
    torch = require_gpu()
    n_files, k = int(n_files), int(k)
    if n_files < 0 or k < 0 or _nbytes(records) < n_files * (k + 1) * 24:
        raise ValueError("the table holds fewer than n_files * (%s + 1) records" % what)
    out = _record_out(out, torch, n_files, record_bytes, records.device)
    check(getattr(load(), fn)(records.data_ptr(), n_files, k, *extra, out.data_ptr(), current_stream_ptr(torch)))
    return out


def surrogate_lists(list_ptr, n_bound, seeds, out_off, out_cap, n_surrogates: int, block_units: int, out, status) -> None:
    """``ffs_surrogate_lists`` on the current stream: per vector the device pointer of its ``ffs_runs_list``, a host-known
    bound of its length, its uint32 seed, the byte offset in ``out`` (uint8 / int32 CUDA tensor) of the first of its
    ``n_surrogates`` back-to-back blocks and their capacity in entries; ``status``: int32 CUDA tensor, one per vector."""
    _resampled_lists("ffs_surrogate_lists", list_ptr, n_bound, seeds, out_off, out_cap, n_surrogates, block_units, out, status)


def null_stats(records, n_files: int, n_surrogates: int, out=None):
    """``ffs_null_stats`` on the current stream: ``records`` a CUDA tensor of n_files * (n_surrogates + 1)
    ffs_cand_result records (24 bytes each; per file the real list's solve, then the surrogates'); returns the uint8 CUDA
    tensor of n_files ``NULL_RESULT_DTYPE`` records (``out``, if given, is written in place)."""
    return _record_stats("ffs_null_stats", records, n_files, n_surrogates, NULL_RESULT_BYTES, "n_surrogates", out=out)


def subsample_lists(list_ptr, n_bound, seeds, out_off, out_cap, n_subsamples: int, block_runs: int, out, status) -> None:
    """``ffs_subsample_lists`` on the current stream: the arguments of ``surrogate_lists``, with ``n_subsamples`` thinned
    lists per vector and blocks of ``block_runs`` runs."""
    _resampled_lists("ffs_subsample_lists", list_ptr, n_bound, seeds, out_off, out_cap, n_subsamples, block_runs, out, status)


def offset_stats(records, n_files: int, n_subsamples: int, tol: int, out=None):
    """``ffs_offset_stats`` on the current stream: ``records`` a CUDA tensor of n_files * (n_subsamples + 1)
    ffs_cand_result records (24 bytes each; per file the real list's solve, then the subsamples'); returns the uint8 CUDA
    tensor of n_files ``STABILITY_RESULT_DTYPE`` records (``out``, if given, is written in place)."""
    return _record_stats("ffs_offset_stats", records, n_files, n_subsamples, STABILITY_RESULT_BYTES, "n_subsamples", int(tol),
                         out=out)


def _us_arrays(start_us, end_us, is_metadata):
    start_us = np.ascontiguousarray(start_us, dtype=np.int64)
    end_us = np.ascontiguousarray(end_us, dtype=np.int64)
    if start_us.shape != end_us.shape:
        raise ValueError("start_us and end_us must have the same length")
    meta = None if is_metadata is None else np.ascontiguousarray(is_metadata, dtype=np.uint8)
    return start_us, end_us, meta


def raster_length(end_us, ratio: float, sample_rate: float) -> int:
    end_us = np.ascontiguousarray(end_us, dtype=np.int64)
    return int(load().ffs_raster_length(end_us.ctypes.data, end_us.size, float(ratio), float(sample_rate)))


def raster_intervals(start_us, end_us, is_metadata, ratio, sample_rate, start_seconds, out_len) -> np.ndarray:
    """Host-only: [n, 2] int32 array of the clamped [start, end) sample intervals."""
    start_us, end_us, meta = _us_arrays(start_us, end_us, is_metadata)
    iv = np.zeros((start_us.size + 1, 2), dtype=np.int32)
    n = load().ffs_raster_intervals(start_us.ctypes.data, end_us.ctypes.data, None if meta is None else meta.ctypes.data,
                                    start_us.size, float(ratio), float(sample_rate), float(start_seconds), int(out_len),
                                    iv.ctypes.data)
    return iv[:n]


def rasterize_subtitles(start_us, end_us, is_metadata, ratio, sample_rate=100.0, start_seconds=0.0, packed=False):
    """The subtitle track rescaled by ``ratio`` as a CUDA tensor: 0/1 bytes (uint8[n]), or with
    ``packed`` one bit per sample (int32[ceil(n/32)], FFS_DTYPE_U1) -- returns (tensor, n) then."""
    torch = require_gpu()
    start_us, end_us, meta = _us_arrays(start_us, end_us, is_metadata)
    n = raster_length(end_us, ratio, sample_rate)
    fn = load().ffs_rasterize_subtitles_bits if packed else load().ffs_rasterize_subtitles
    out = torch.empty((n + 31) // 32, dtype=torch.int32, device="cuda") if packed else \
        torch.empty(n, dtype=torch.uint8, device="cuda")
    check(fn(start_us.ctypes.data, end_us.ctypes.data, None if meta is None else meta.ctypes.data, start_us.size,
             float(ratio), float(sample_rate), float(start_seconds), out.data_ptr(), n, current_stream_ptr(torch)))
    return (out, n) if packed else out


def raster_lengths(track_end_us_max, ratio, sample_rate=100.0) -> np.ndarray:
    """Host-only: raster lengths of many vectors at once (``ffs_raster_lengths``): vector v is a track whose largest
    end time is ``track_end_us_max[v]`` microseconds, scaled by ``ratio[v]``."""
    ends = np.ascontiguousarray(track_end_us_max, dtype=np.int64)
    ratio = np.ascontiguousarray(ratio, dtype=np.float64)
    if ends.shape != ratio.shape:
        raise ValueError("one ratio per vector")
    out = np.zeros(ends.size, dtype=np.int64)
    check(load().ffs_raster_lengths(ends.ctypes.data, ratio.ctypes.data, ends.size, float(sample_rate), out.ctypes.data))
    return out


def rasterize_batch_bits(start_us, end_us, is_metadata, vec_sub_first, vec_sub_count, vec_ratio, vec_out_word, vec_len,
                         out, sample_rate=100.0, start_seconds=0.0) -> None:
    """``ffs_rasterize_batch_bits``: every vector of a batch from ONE call, interval arithmetic on the device.  The
    tracks are concatenated in ``start_us`` / ``end_us`` / ``is_metadata``; vector v covers subtitles
    [vec_sub_first[v], +vec_sub_count[v]) scaled by vec_ratio[v] and lands as vec_len[v] bits at word vec_out_word[v]
    of ``out`` (int32 / uint8 CUDA tensor, zeroed by the call)."""
    torch = require_gpu()
    start_us, end_us, meta = _us_arrays(start_us, end_us, is_metadata)
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
    first, count, word, length = i64(vec_sub_first), i64(vec_sub_count), i64(vec_out_word), i64(vec_len)
    ratio = np.ascontiguousarray(vec_ratio, dtype=np.float64)
    n_vec = first.size
    if not (count.size == word.size == length.size == ratio.size == n_vec):
        raise ValueError("the vector tables must have the same length")
    out_words = out.numel() * out.element_size() // 4
    check(load().ffs_rasterize_batch_bits(start_us.ctypes.data, end_us.ctypes.data, None if meta is None else meta.ctypes.data,
                                          start_us.size, first.ctypes.data, count.ctypes.data, ratio.ctypes.data,
                                          word.ctypes.data, length.ctypes.data, n_vec, float(sample_rate),
                                          float(start_seconds), out.data_ptr(), out_words, current_stream_ptr(torch)))


def runs_list_bytes(cap: int) -> int:
    """Bytes of an ``ffs_runs_list`` block with room for ``cap`` entries (16-byte header + 8 bytes per entry)."""
    return 16 + 8 * int(cap)


def rasterize_batch_runs(start_us, end_us, is_metadata, vec_sub_first, vec_sub_count, vec_ratio, vec_out_off, vec_cap,
                         vec_len, out, sample_rate=100.0, start_seconds=0.0) -> None:
    """``ffs_rasterize_batch_runs``: every vector of a batch as its BOUNDARY LIST (FFS_DTYPE_RUNS), no bitmap.  Vector v
    covers subtitles [vec_sub_first[v], +vec_sub_count[v]) scaled by vec_ratio[v]; its list block starts at byte
    vec_out_off[v] of ``out`` (CUDA tensor; offsets multiples of 8) and holds up to vec_cap[v] >= 2 * count + 1 entries.
    ``start_us`` / ``end_us`` / ``is_metadata``: host arrays, or int64 / int64 / uint8 CUDA tensors (tracks uploaded once,
    sorted by start time: nothing of them is copied per call)."""
    torch = require_gpu()
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
    if hasattr(start_us, "data_ptr"):  # device-resident tables
        first, count, off, cap, length = i64(vec_sub_first), i64(vec_sub_count), i64(vec_out_off), i64(vec_cap), i64(vec_len)
        ratio = np.ascontiguousarray(vec_ratio, dtype=np.float64)
        n_vec = first.size
        if not (count.size == off.size == cap.size == length.size == ratio.size == n_vec):
            raise ValueError("the vector tables must have the same length")
        check(load().ffs_rasterize_batch_runs(start_us.data_ptr(), end_us.data_ptr(),
                                              None if is_metadata is None else is_metadata.data_ptr(), start_us.numel(),
                                              first.ctypes.data, count.ctypes.data, ratio.ctypes.data, off.ctypes.data,
                                              cap.ctypes.data, length.ctypes.data, n_vec, float(sample_rate),
                                              float(start_seconds), out.data_ptr(), out.numel() * out.element_size(),
                                              current_stream_ptr(torch)))
        return
    start_us, end_us, meta = _us_arrays(start_us, end_us, is_metadata)
    first, count, off, cap, length = i64(vec_sub_first), i64(vec_sub_count), i64(vec_out_off), i64(vec_cap), i64(vec_len)
    ratio = np.ascontiguousarray(vec_ratio, dtype=np.float64)
    n_vec = first.size
    if not (count.size == off.size == cap.size == length.size == ratio.size == n_vec):
        raise ValueError("the vector tables must have the same length")
    check(load().ffs_rasterize_batch_runs(start_us.ctypes.data, end_us.ctypes.data, None if meta is None else meta.ctypes.data,
                                          start_us.size, first.ctypes.data, count.ctypes.data, ratio.ctypes.data,
                                          off.ctypes.data, cap.ctypes.data, length.ctypes.data, n_vec, float(sample_rate),
                                          float(start_seconds), out.data_ptr(), out.numel() * out.element_size(),
                                          current_stream_ptr(torch)))


def runs_from_bits(words, n: int, cap: Optional[int] = None, out=None):
    """Boundary list (``ffs_runs_list`` block, int32 CUDA tensor of 4 + 2 * cap words) of a FFS_DTYPE_U1 vector of ``n``
    samples: one pass over the bits.  ``cap`` defaults to room for every possible boundary count below 32 768."""
    torch = require_gpu()
    cap = 32768 if cap is None else int(cap)
    if out is None:
        out = torch.empty(4 + 2 * cap, dtype=torch.int32, device=words.device)
    elif out.numel() * out.element_size() < runs_list_bytes(cap):
        raise ValueError("list block too small")
    check(load().ffs_runs_from_bits(words.data_ptr(), int(n), out.data_ptr(), cap, current_stream_ptr(torch)))
    return out


def runs_from_bits_batch(bits_ptr, lens, list_ptr, caps) -> None:
    """``ffs_runs_from_bits_batch``: n vectors (device pointers to FFS_DTYPE_U1 words, lengths in samples) into n list
    blocks (device pointers, capacities in entries) with one launch."""
    torch = require_gpu()
    bits_ptr = np.ascontiguousarray(bits_ptr, dtype=np.uint64)
    list_ptr = np.ascontiguousarray(list_ptr, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.int64)
    caps = np.ascontiguousarray(caps, dtype=np.int64)
    if not (bits_ptr.size == list_ptr.size == lens.size == caps.size):
        raise ValueError("the vector tables must have the same length")
    check(load().ffs_runs_from_bits_batch(bits_ptr.ctypes.data, lens.ctypes.data, list_ptr.ctypes.data, caps.ctypes.data,
                                          bits_ptr.size, current_stream_ptr(torch)))


def runs_to_bits(block, n: int, out=None):
    """FFS_DTYPE_U1 words (int32 CUDA tensor) of the ``n``-sample vector an ``ffs_runs_list`` block describes (written
    into ``out`` when given: at least ``packed_words(n)`` int32)."""
    torch = require_gpu()
    if out is None:
        out = torch.empty(packed_words(n), dtype=torch.int32, device=block.device)
    assert out.dtype == torch.int32 and out.numel() >= packed_words(n)
    check(load().ffs_runs_to_bits(block.data_ptr(), int(n), out.data_ptr(), current_stream_ptr(torch)))
    return out


def runs_list_host(block) -> Tuple[np.ndarray, np.ndarray, int]:
    """(positions, ones_before, ones) of a list block, on the host (tests, diagnostics)."""
    raw = block.view(require_gpu().int32).cpu().numpy()
    n, ones = int(raw[0]), int(raw[1])
    e = raw[4:4 + 2 * n].reshape(n, 2)
    return e[:, 0].copy(), e[:, 1].copy(), ones


def two_level_pack(values: np.ndarray):
    """Host-only (``ffs_two_level_pack``): (lo, hi, packed) for a contiguous float64 vector whose samples take two
    finite levels -- ``packed`` = the samples as little-endian bits (uint8[4 * ceil(n/32)], bit i = (values[i] == hi))
    -- or None when they do not."""
    assert values.dtype == np.float64 and values.flags.c_contiguous and values.ndim == 1 and values.size > 0
    levels = np.zeros(2, dtype=np.float64)
    words = np.empty((values.size + 31) // 32, dtype=np.uint32)
    rc = load().ffs_two_level_pack(values.ctypes.data, values.size, levels.ctypes.data, levels[1:].ctypes.data,
                                   words.ctypes.data)
    if rc < 0:
        check(rc)
    return (float(levels[0]), float(levels[1]), words.view(np.uint8)) if rc == 1 else None


def packed_words(n: int) -> int:
    return (int(n) + 31) // 32


def pack_bits(src, threshold: float = 0.5, out=None):
    """FFS_DTYPE_U1 image (int32 CUDA tensor of ceil(n/32) words) of a two-level CUDA vector:
    uint8 -> bit = (byte != 0); float32 -> bit = (x > threshold)."""
    torch = require_gpu()
    n = src.numel()
    if src.dtype == torch.uint8:
        dt = FFS_DTYPE_U8
    elif src.dtype == torch.float32:
        dt = FFS_DTYPE_F32
    else:
        raise TypeError("pack_bits needs a uint8 or float32 tensor, got %s" % src.dtype)
    if out is None:
        out = torch.empty(packed_words(n), dtype=torch.int32, device=src.device)
    elif out.numel() * out.element_size() < packed_words(n) * 4:
        raise ValueError("output too small")
    if n:
        check(load().ffs_pack_bits(src.data_ptr(), dt, n, float(threshold), out.data_ptr(), current_stream_ptr(torch)))
    return out


def unpack_bits(words, n: int):
    """uint8 0/1 CUDA tensor of the first n samples of a FFS_DTYPE_U1 vector (torch ops; diagnostics and
    the boundary scan -- the hot kernels read the packed words directly)."""
    torch = require_gpu()
    w = words.view(torch.int32).reshape(-1)
    shifts = torch.arange(32, device=w.device, dtype=torch.int32)
    return ((w[:, None] >> shifts[None, :]) & 1).to(torch.uint8).reshape(-1)[:n]


def scatter_segments(labels, src_off, dst_start, seg_len, out_len: int):
    """float32 CUDA vector of ``out_len`` zeros with labels[src_off[i]:src_off[i]+seg_len[i]] copied to
    dst_start[i] for every sampled window (see ffs_scatter_segments)."""
    torch = require_gpu()
    src_off = np.ascontiguousarray(src_off, dtype=np.int64)
    dst_start = np.ascontiguousarray(dst_start, dtype=np.int64)
    seg_len = np.ascontiguousarray(seg_len, dtype=np.int64)
    if not (src_off.size == dst_start.size == seg_len.size):
        raise ValueError("segment arrays must have the same length")
    if src_off.size and int((src_off + seg_len).max()) > labels.numel():
        raise ValueError("segment reaches beyond the label buffer")
    out = torch.empty(int(out_len), dtype=torch.float32, device=labels.device)
    check(load().ffs_scatter_segments(labels.data_ptr() if labels.numel() else None, src_off.ctypes.data,
                                      dst_start.ctypes.data, seg_len.ctypes.data, int(src_off.size), out.data_ptr(),
                                      int(out_len), current_stream_ptr(torch)))
    return out


def _pair_buffers(ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, *extra):
    """The per-pair host arrays of a side-plan batch call as contiguous buffers: uint64 pointers, int64 lengths, float64
    levels, then ``extra`` int64 arrays.  Returns (n_pairs, their addresses, the buffers); keep the buffers alive over
    the call."""
    kinds = (np.uint64, np.int64, np.float64, np.float64) * 2 + (np.int64,) * len(extra)
    bufs = [np.ascontiguousarray(a, dtype=t)
            for a, t in zip((ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi) + extra, kinds)]
    n = bufs[0].size
    if not all(b.size == n for b in bufs):
        raise ValueError("one descriptor entry per pair")
    return n, [b.ctypes.data for b in bufs], bufs


def _nbytes(tensor) -> int:
    return tensor.numel() * tensor.element_size()


def _check_block_records(n, counts_out, records_out, record_bytes, offsets, *per_block, what="output buffer too small"):
    """The size tests of a call that writes ``n`` counts and one record of ``record_bytes`` per entry of ``offsets`` (the
    n_pairs * max_b block offsets), and reads or writes the ``per_block`` tensors at as many entries."""
    if (counts_out.numel() < n or _nbytes(records_out) < offsets.numel() * record_bytes
            or any(t.numel() < offsets.numel() for t in per_block)):
        raise ValueError(what)


class _SidePlan:
    """Handle lifetime of the plans beside the headline aligner.  A subclass names its C entry points (``_create``,
    ``_destroy``, ``_workspace``) and its size limits (``_limits``) in the order ``_create`` takes them: they become
    attributes, and ``fits`` takes them in the same order."""

    _create = _destroy = _workspace = ""
    _limits: Tuple[str, ...] = ()

    def __init__(self, dims, device: Optional[int]) -> None:
        self._dims = tuple(int(d) for d in dims)
        for name, value in zip(self._limits, self._dims):
            setattr(self, name, value)
        torch = require_gpu()
        self.lib = load()
        self.device = torch.cuda.current_device() if device is None else int(device)
        handle = ctypes.c_void_p()
        check(getattr(self.lib, self._create)(self.device, *self._dims, ctypes.byref(handle)))
        self.handle = handle

    @property
    def workspace_bytes(self) -> int:
        return int(getattr(self.lib, self._workspace)(self.handle))

    def fits(self, *dims) -> bool:
        return all(have >= want for have, want in zip(self._dims, dims))

    @staticmethod
    def _stream(stream: Optional[int]):
        return current_stream_ptr(require_gpu()) if stream is None else stream

    def close(self) -> None:
        if getattr(self, "handle", None):
            getattr(self.lib, self._destroy)(self.handle)
            self.handle = None

    def __del__(self) -> None:  # pragma: no cover - interpreter shutdown ordering
        try:
            self.close()
        except Exception:
            pass


class _BlockPlan(_SidePlan):
    """A side plan sized by pairs in flight, blocks, lags and samples."""

    _limits = ("pairs_in_flight", "max_blocks", "max_lags", "max_samples")

    def __init__(self, pairs_in_flight: int, max_blocks: int, max_lags: int, max_samples: int,
                 device: Optional[int] = None) -> None:
        super().__init__((pairs_in_flight, max_blocks, max_lags, max_samples), device)


class SplitPlan(_BlockPlan):
    """Owns one ``ffs_split_plan``: the workspace of the split-aware aligner (``split_align.py``) for
    ``pairs_in_flight`` problems of up to ``max_samples`` subtitle samples, ``max_blocks`` blocks and ``max_lags`` = 2W
    lags."""

    _create, _destroy, _workspace = "ffs_split_plan_create", "ffs_split_plan_destroy", "ffs_split_plan_workspace_bytes"

    def align(self, ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, block_samples: int,
              max_offset_samples: int, split_penalty: float, offsets_out, scores_out, totals_out,
              stream: Optional[int] = None) -> None:
        """``ffs_align_split_batch`` on host descriptor arrays (one entry per pair) into int32 / float64 / float64 CUDA
        tensors of n_pairs * max_b, n_pairs * max_b and n_pairs entries (asynchronous)."""
        n, ptrs, _bufs = _pair_buffers(ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi)
        check(self.lib.ffs_align_split_batch(self.handle, n, *ptrs, int(block_samples), int(max_offset_samples),
                                             float(split_penalty), offsets_out.data_ptr(), scores_out.data_ptr(),
                                             totals_out.data_ptr(), self._stream(stream)))

    def align_report(self, ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, block_samples: int,
                     max_offset_samples: int, split_penalty: float, top_k: int, exclusion_samples: int, offsets_out,
                     scores_out, totals_out, report_out, n_pieces_out, stream: Optional[int] = None) -> None:
        """``ffs_align_split_report_batch``: ``align``'s outputs plus a uint8 CUDA tensor of n_pairs * max_b * 224 bytes
        of piece reports and an int32 one of n_pairs piece counts (asynchronous)."""
        n, ptrs, _bufs = _pair_buffers(ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi)
        _check_block_records(n, n_pieces_out, report_out, PIECE_REPORT_BYTES, offsets_out)
        check(self.lib.ffs_align_split_report_batch(self.handle, n, *ptrs, int(block_samples), int(max_offset_samples),
                                                    float(split_penalty), int(top_k), int(exclusion_samples),
                                                    offsets_out.data_ptr(), scores_out.data_ptr(), totals_out.data_ptr(),
                                                    report_out.data_ptr(), n_pieces_out.data_ptr(), self._stream(stream)))

    def refine(self, ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, block_samples: int,
               offsets, radius_samples: int, unmatched_margin: float, refine_out, n_breaks_out,
               stream: Optional[int] = None) -> None:
        """``ffs_split_refine_batch``: the int32 CUDA tensor of n_pairs * max_b block offsets (as ``align`` wrote them)
        into a uint8 CUDA tensor of n_pairs * max_b * 88 bytes of break records and an int32 one of n_pairs break counts
        (asynchronous); ``unmatched_margin`` NaN = a single cut."""
        n, ptrs, _bufs = _pair_buffers(ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi)
        _check_block_records(n, n_breaks_out, refine_out, BREAK_REFINE_BYTES, offsets)
        check(self.lib.ffs_split_refine_batch(self.handle, n, *ptrs, int(block_samples), offsets.data_ptr(),
                                              int(radius_samples), float(unmatched_margin), refine_out.data_ptr(),
                                              n_breaks_out.data_ptr(), self._stream(stream)))

    def drift_refine(self, ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, block_samples: int,
                     offsets, jumps, radius_samples: int, unmatched_margin: float, refine_out, n_jumps_out,
                     stream: Optional[int] = None) -> None:
        """``ffs_drift_refine_batch``: ``refine`` along a drift path -- the int32 CUDA tensor of n_pairs * max_b block
        offsets and the uint8 one of as many jump flags (as ``DriftPlan.align`` or a smooth fit wrote them) into break
        records at the jumps and an int32 tensor of n_pairs jump counts (asynchronous)."""
        n, ptrs, _bufs = _pair_buffers(ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi)
        _check_block_records(n, n_jumps_out, refine_out, BREAK_REFINE_BYTES, offsets, jumps, what="buffer too small")
        check(self.lib.ffs_drift_refine_batch(self.handle, n, *ptrs, int(block_samples), offsets.data_ptr(),
                                              jumps.data_ptr(), int(radius_samples), float(unmatched_margin),
                                              refine_out.data_ptr(), n_jumps_out.data_ptr(), self._stream(stream)))

    def cue_report(self, ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, cues, cue_first, cue_count,
                   radius_samples: int, context_samples: int, report_out, stream: Optional[int] = None) -> None:
        """``ffs_cue_report_batch``: the uint8 CUDA tensor ``cues`` of 24-byte ``CUE_DTYPE`` entries, pair p's being the
        ``cue_count[p]`` entries from ``cue_first[p]`` on, into a uint8 CUDA tensor of one 120-byte record per table
        entry (asynchronous)."""
        n_cues = cues.numel() * cues.element_size() // CUE_BYTES
        n, ptrs, _bufs = _pair_buffers(ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, cue_first,
                                       cue_count)
        if _nbytes(report_out) < n_cues * CUE_REPORT_BYTES:
            raise ValueError("output buffer too small")
        check(self.lib.ffs_cue_report_batch(self.handle, n, *ptrs[:8], cues.data_ptr(), n_cues, ptrs[8], ptrs[9],
                                            int(radius_samples), int(context_samples), report_out.data_ptr(),
                                            self._stream(stream)))

    def cue_retime(self, ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, cues, cue_first, cue_count,
                   radius_samples: int, context_samples: int, penalty_q: int, jump_q: int, flags: int, retime_out,
                   summary_out, stream: Optional[int] = None) -> None:
        """``ffs_cue_retime_batch``: the cue table as ``cue_report`` takes it, into a uint8 CUDA tensor of one 64-byte
        ``CUE_RETIME_DTYPE`` record per table entry and one of a 40-byte ``RETIME_SUMMARY_DTYPE`` record per pair
        (asynchronous)."""
        n_cues = cues.numel() * cues.element_size() // CUE_BYTES
        n, ptrs, _bufs = _pair_buffers(ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, cue_first,
                                       cue_count)
        if _nbytes(retime_out) < n_cues * CUE_RETIME_BYTES or _nbytes(summary_out) < n * RETIME_SUMMARY_BYTES:
            raise ValueError("output buffer too small")
        check(self.lib.ffs_cue_retime_batch(self.handle, n, *ptrs[:8], cues.data_ptr() if n_cues else None, n_cues,
                                            ptrs[8], ptrs[9], int(radius_samples), int(context_samples), int(penalty_q),
                                            int(jump_q), int(flags), retime_out.data_ptr() if n_cues else None,
                                            summary_out.data_ptr(), self._stream(stream)))


def range_band_row(max_step: int, knot_blocks: int, radius: int) -> int:
    """uint16 cells of one block's band row in the range smooth fit (``range_band_row`` of
    csrc/ffs_drift_range_smooth.h)."""
    return int(max_step) * ((3 * int(knot_blocks) + 1) // 2) + 2 * int(radius) + 1


MAX_DRIFT_STEP = 7  # DRIFT_MAX_STEP (csrc/ffs_drift.h): the 4-bit code holds STAY, 14 moves and JUMP


class DriftPlan(_BlockPlan):
    """Owns one ``ffs_drift_plan``: the workspace of the drift-tolerant aligner (``drift_align.py``) for
    ``pairs_in_flight`` problems of up to ``max_samples`` subtitle samples, ``max_blocks`` blocks and ``max_lags`` = 2W
    lags."""

    _create, _destroy, _workspace = "ffs_drift_plan_create", "ffs_drift_plan_destroy", "ffs_drift_plan_workspace_bytes"

    def align(self, ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, block_samples: int,
              max_offset_samples: int, split_penalty: float, max_step: int, step_cost: float, offsets_out, scores_out,
              jumps_out, totals_out, stream: Optional[int] = None) -> None:
        """``ffs_align_drift_batch`` on host descriptor arrays (one entry per pair) into int32 / float64 / uint8 /
        float64 CUDA tensors of n_pairs * max_b (three times) and n_pairs entries (asynchronous)."""
        n, ptrs, _bufs = _pair_buffers(ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi)
        check(self.lib.ffs_align_drift_batch(self.handle, n, *ptrs, int(block_samples), int(max_offset_samples),
                                             float(split_penalty), int(max_step), float(step_cost),
                                             offsets_out.data_ptr(), scores_out.data_ptr(), jumps_out.data_ptr(),
                                             totals_out.data_ptr(), self._stream(stream)))

    def report(self, ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, block_samples: int,
               max_offset_samples: int, split_penalty: float, max_step: int, step_cost: float, top_k: int,
               exclusion_samples: int, offsets_out, scores_out, jumps_out, totals_out, report_out, n_segments_out,
               stream: Optional[int] = None) -> None:
        """``ffs_align_drift_report_batch``: ``align``'s outputs plus a uint8 CUDA tensor of n_pairs * max_b * 264
        bytes of segment reports and an int32 one of n_pairs segment counts.  The call reads each sub-batch's segment
        counts back, so it waits for the stream."""
        n, ptrs, _bufs = _pair_buffers(ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi)
        _check_block_records(n, n_segments_out, report_out, SEGMENT_REPORT_BYTES, offsets_out)
        check(self.lib.ffs_align_drift_report_batch(self.handle, n, *ptrs, int(block_samples), int(max_offset_samples),
                                                    float(split_penalty), int(max_step), float(step_cost), int(top_k),
                                                    int(exclusion_samples), offsets_out.data_ptr(),
                                                    scores_out.data_ptr(), jumps_out.data_ptr(), totals_out.data_ptr(),
                                                    report_out.data_ptr(), n_segments_out.data_ptr(),
                                                    self._stream(stream)))

    def smooth(self, ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, block_samples: int,
               max_offset_samples: int, split_penalty: float, max_step: int, step_cost: float, knot_blocks: int,
               radius: int, bend_cost: float, offsets_out, scores_out, jumps_out, totals_out, smooth_out, knot_out,
               segments_out, n_segments_out, stream: Optional[int] = None) -> None:
        """``ffs_align_drift_smooth_batch``: ``align``'s outputs plus int32 smooth offsets and uint8 knot flags of
        n_pairs * max_b entries, a CUDA tensor of n_pairs * max_b * 32 bytes of segment records and an int32 one of
        n_pairs segment counts (asynchronous)."""
        n, ptrs, _bufs = _pair_buffers(ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi)
        _check_block_records(n, n_segments_out, segments_out, SMOOTH_SEGMENT_BYTES, offsets_out, smooth_out, knot_out)
        check(self.lib.ffs_align_drift_smooth_batch(self.handle, n, *ptrs, int(block_samples), int(max_offset_samples),
                                                    float(split_penalty), int(max_step), float(step_cost),
                                                    int(knot_blocks), int(radius), float(bend_cost),
                                                    offsets_out.data_ptr(), scores_out.data_ptr(), jumps_out.data_ptr(),
                                                    totals_out.data_ptr(), smooth_out.data_ptr(), knot_out.data_ptr(),
                                                    segments_out.data_ptr(), n_segments_out.data_ptr(),
                                                    self._stream(stream)))


class SplitRangePlan(_BlockPlan):
    """Owns one ``ffs_split_range_plan``: the workspace of the lag-range split aligner (``cut_align.py``) for
    ``pairs_in_flight`` problems of up to ``max_samples`` samples per vector, ``max_blocks`` blocks and ``max_lags``
    lags."""

    _create = "ffs_split_range_plan_create"
    _destroy, _workspace = "ffs_split_range_plan_destroy", "ffs_split_range_plan_workspace_bytes"

    def align(self, ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, block_samples: int, lag_lo,
              lag_hi, split_penalty: float, offsets_out, scores_out, totals_out, stream: Optional[int] = None) -> None:
        """``ffs_align_split_range_batch`` on host descriptor arrays (one entry per pair, ``lag_lo`` / ``lag_hi``
        included) into int32 / float64 / float64 CUDA tensors of n_pairs * max_b, n_pairs * max_b and n_pairs entries
        (asynchronous)."""
        n, ptrs, _bufs = _pair_buffers(ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, lag_lo, lag_hi)
        check(self.lib.ffs_align_split_range_batch(self.handle, n, *ptrs[:8], int(block_samples), *ptrs[8:],
                                                   float(split_penalty), offsets_out.data_ptr(), scores_out.data_ptr(),
                                                   totals_out.data_ptr(), self._stream(stream)))

    def report(self, ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, block_samples: int, lag_lo,
               lag_hi, offsets, top_k: int, exclusion_samples: int, report_out, n_pieces_out,
               stream: Optional[int] = None) -> None:
        """``ffs_split_range_report_batch``: the piece reports of the int32 CUDA tensor of n_pairs * max_b block offsets
        (as ``align`` wrote them) over each pair's range into a uint8 CUDA tensor of n_pairs * max_b * 224 bytes and an
        int32 one of n_pairs piece counts.  The call waits for the stream's earlier work (it reads the offsets back)."""
        n, ptrs, _bufs = _pair_buffers(ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, lag_lo, lag_hi)
        _check_block_records(n, n_pieces_out, report_out, PIECE_REPORT_BYTES, offsets)
        check(self.lib.ffs_split_range_report_batch(self.handle, n, *ptrs[:8], int(block_samples), *ptrs[8:],
                                                    offsets.data_ptr(), int(top_k), int(exclusion_samples),
                                                    report_out.data_ptr(), n_pieces_out.data_ptr(), self._stream(stream)))


class DriftRangePlan(_SidePlan):
    """Owns one ``ffs_drift_range_plan``: the workspace of the lag-range drift aligner (``drift_range.py``) for
    ``pairs_in_flight`` problems of up to ``max_samples`` samples per vector, ``max_blocks`` blocks, ``max_lags`` lags
    and calls at ``max_step`` up to ``max_step_cap``."""

    _create = "ffs_drift_range_plan_create"
    _destroy, _workspace = "ffs_drift_range_plan_destroy", "ffs_drift_range_plan_workspace_bytes"
    _limits = _BlockPlan._limits + ("max_step_cap",)

    def __init__(self, pairs_in_flight: int, max_blocks: int, max_lags: int, max_samples: int, max_step_cap: int,
                 device: Optional[int] = None) -> None:
        super().__init__((pairs_in_flight, max_blocks, max_lags, max_samples, max_step_cap), device)

    def align(self, ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, block_samples: int, lag_lo,
              lag_hi, split_penalty: float, max_step: int, step_cost: float, offsets_out, scores_out, jumps_out,
              totals_out, stream: Optional[int] = None) -> None:
        """``ffs_align_drift_range_batch`` on host descriptor arrays (one entry per pair, ``lag_lo`` / ``lag_hi``
        included) into int32 / float64 / uint8 / float64 CUDA tensors of n_pairs * max_b (three times) and n_pairs
        entries (asynchronous)."""
        n, ptrs, _bufs = _pair_buffers(ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, lag_lo, lag_hi)
        check(self.lib.ffs_align_drift_range_batch(self.handle, n, *ptrs[:8], int(block_samples), *ptrs[8:],
                                                   float(split_penalty), int(max_step), float(step_cost),
                                                   offsets_out.data_ptr(), scores_out.data_ptr(), jumps_out.data_ptr(),
                                                   totals_out.data_ptr(), self._stream(stream)))

    def smooth_bytes(self) -> int:
        """What the first ``smooth`` call adds to ``workspace_bytes``: ``SMOOTH_BLOCK_BYTES`` of fit tables and a band
        row of ``range_band_row(max_step_cap, 256, 16)`` uint16 counts per block (``max_blocks`` rounded up to 16) and
        pair in flight, the back-pointers and the interval counts each padded to 64 bytes."""
        n, mb = self.pairs_in_flight, -(-self.max_blocks // 16) * 16
        pad64 = lambda x: -(-x // 64) * 64
        return (n * mb * (SMOOTH_MAX_STATES * 8 + 36 + 2 * range_band_row(self.max_step_cap, SMOOTH_MAX_KNOT_BLOCKS,
                                                                          SMOOTH_MAX_RADIUS))
                + pad64(n * mb * SMOOTH_MAX_STATES) + pad64(n * 4))

    def smooth(self, ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, block_samples: int, lag_lo,
               lag_hi, split_penalty: float, max_step: int, step_cost: float, knot_blocks: int, radius: int,
               bend_cost: float, offsets_out, scores_out, jumps_out, totals_out, smooth_out, knot_out, segments_out,
               n_segments_out, stream: Optional[int] = None) -> None:
        """``ffs_align_drift_range_smooth_batch``: ``align``'s outputs plus int32 smooth offsets and uint8 knot flags of
        n_pairs * max_b entries, a CUDA tensor of n_pairs * max_b * 32 bytes of segment records and an int32 one of
        n_pairs segment counts (asynchronous)."""
        n, ptrs, _bufs = _pair_buffers(ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, lag_lo, lag_hi)
        _check_block_records(n, n_segments_out, segments_out, SMOOTH_SEGMENT_BYTES, offsets_out, smooth_out, knot_out)
        check(self.lib.ffs_align_drift_range_smooth_batch(self.handle, n, *ptrs[:8], int(block_samples), *ptrs[8:],
                                                          float(split_penalty), int(max_step), float(step_cost),
                                                          int(knot_blocks), int(radius), float(bend_cost),
                                                          offsets_out.data_ptr(), scores_out.data_ptr(),
                                                          jumps_out.data_ptr(), totals_out.data_ptr(),
                                                          smooth_out.data_ptr(), knot_out.data_ptr(),
                                                          segments_out.data_ptr(), n_segments_out.data_ptr(),
                                                          self._stream(stream)))

    def report_bytes(self) -> int:
        """What the first ``report`` call adds to ``workspace_bytes``: 8 rows of ``max_lags`` + 1 cells (padded to 64)
        of 12 bytes per pair in flight, and the work-item table."""
        lpad = -(-(self.max_lags + 1) // 64) * 64
        words = -(-self.max_samples // 32)
        items = 2 * (-(-words // RPATH_CHUNK_WORDS) + self.max_blocks)
        return self.pairs_in_flight * (RPATH_ROUND_SEGMENTS * lpad * 12 + items * 32)

    def report(self, ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, block_samples: int, lag_lo,
               lag_hi, offsets, jumps, top_k: int, exclusion_samples: int, report_out, n_segments_out,
               stream: Optional[int] = None) -> None:
        """``ffs_drift_range_report_batch``: the segment path reports of the int32 / uint8 CUDA tensors of
        n_pairs * max_b block offsets and jump flags (as ``align`` wrote them) over each pair's range into a CUDA
        tensor of n_pairs * max_b * 264 bytes and an int32 one of n_pairs segment counts.  The call waits for the
        stream's earlier work (it reads the path back)."""
        n, ptrs, _bufs = _pair_buffers(ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, lag_lo, lag_hi)
        _check_block_records(n, n_segments_out, report_out, SEGMENT_REPORT_BYTES, offsets, jumps)
        check(self.lib.ffs_drift_range_report_batch(self.handle, n, *ptrs[:8], int(block_samples), *ptrs[8:],
                                                    offsets.data_ptr(), jumps.data_ptr(), int(top_k),
                                                    int(exclusion_samples), report_out.data_ptr(),
                                                    n_segments_out.data_ptr(), self._stream(stream)))


class QualityPlan(_SidePlan):
    """Owns one ``ffs_quality_plan``: the workspace of the alignment quality report (``quality.py``) for
    ``pairs_in_flight`` problems of up to ``max_samples`` samples per vector and ``max_lags`` lags, plus (made on first
    use) a bit buffer that boundary-list inputs are expanded into."""

    _create, _destroy, _workspace = "ffs_quality_plan_create", "ffs_quality_plan_destroy", "ffs_quality_plan_workspace_bytes"

    _limits = ("pairs_in_flight", "max_lags", "max_samples")

    def __init__(self, pairs_in_flight: int, max_lags: int, max_samples: int, device: Optional[int] = None) -> None:
        self.scratch = None  # int32 CUDA tensor: FFS_DTYPE_U1 images of FFS_DTYPE_RUNS vectors
        super().__init__((pairs_in_flight, max_lags, max_samples), device)

    def scratch_words(self, n_words: int):
        """The plan's bit buffer, grown to at least ``n_words`` int32 words."""
        torch = require_gpu()
        if self.scratch is None or self.scratch.numel() < n_words:
            self.scratch = torch.empty(int(n_words), dtype=torch.int32, device=torch.device("cuda", self.device))
        return self.scratch

    def report(self, ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, max_offset_samples,
               top_k: int, exclusion_samples: int, out, stream: Optional[int] = None) -> None:
        """``ffs_align_quality_batch`` on host descriptor arrays (one entry per pair) into a uint8 CUDA tensor of
        n_pairs * 160 bytes (asynchronous).  ``max_offset_samples`` None = no window."""
        n, ptrs, _bufs = _pair_buffers(ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi)
        if _nbytes(out) < n * QUALITY_RESULT_BYTES:
            raise ValueError("output buffer too small")
        mo = -1 if max_offset_samples is None else int(max_offset_samples)
        check(self.lib.ffs_align_quality_batch(self.handle, n, *ptrs, mo, int(top_k), int(exclusion_samples),
                                               out.data_ptr(), self._stream(stream)))

    def close(self) -> None:
        super().close()
        self.scratch = None


def match_algorithm_code(algorithm) -> int:
    """FFS_MATCH_* code of "auto" / "runs" / "bits" (any case, surrounding blanks ignored) or of a code itself."""
    if isinstance(algorithm, (int, np.integer)) and not isinstance(algorithm, bool) and int(algorithm) in MATCH_ALGORITHMS.values():
        return int(algorithm)
    name = algorithm.strip().lower() if isinstance(algorithm, str) else None
    if name not in MATCH_ALGORITHMS:
        raise ValueError("unknown algorithm %r: expected one of %s" % (algorithm, ", ".join(sorted(MATCH_ALGORITHMS))))
    return MATCH_ALGORITHMS[name]


class MatchPlan(_SidePlan):
    """Owns one ``ffs_match_plan``: the workspace of the all-pairs quality report from boundary lists (``match.py``) for
    ``pairs_in_flight`` pairs of up to ``max_lags`` lags and ``max_vectors`` vectors (references and subtitle vectors
    together) of up to ``max_samples`` samples."""

    _create, _destroy, _workspace = "ffs_match_plan_create", "ffs_match_plan_destroy", "ffs_match_plan_workspace_bytes"

    _limits = ("pairs_in_flight", "max_lags", "max_samples", "max_vectors")

    def __init__(self, pairs_in_flight: int, max_lags: int, max_samples: int, max_vectors: int,
                 device: Optional[int] = None) -> None:
        super().__init__((pairs_in_flight, max_lags, max_samples, max_vectors), device)

    def report(self, ref_list, ref_len, ref_lo, ref_hi, sub_list, sub_len, sub_lo, sub_hi, pair_ref, pair_sub,
               max_offset_samples, top_k: int, exclusion_samples: int, out, algorithm="auto",
               stream: Optional[int] = None) -> None:
        """``ffs_match_quality_batch``: host tables of the references and of the subtitle vectors (device pointers of
        their ``ffs_runs_list`` blocks, lengths, two levels) and the index pairs, into a uint8 CUDA tensor of
        n_pairs * 160 bytes.  ``max_offset_samples`` None = no window."""
        kinds = (np.uint64, np.int64, np.float64, np.float64)
        rt = [np.ascontiguousarray(a, dtype=t) for a, t in zip((ref_list, ref_len, ref_lo, ref_hi), kinds)]
        stb = [np.ascontiguousarray(a, dtype=t) for a, t in zip((sub_list, sub_len, sub_lo, sub_hi), kinds)]
        if not all(b.size == rt[0].size for b in rt) or not all(b.size == stb[0].size for b in stb):
            raise ValueError("one table entry per vector")
        pr = np.ascontiguousarray(pair_ref, dtype=np.int32)
        ps = np.ascontiguousarray(pair_sub, dtype=np.int32)
        if pr.size != ps.size:
            raise ValueError("one reference index and one subtitle index per pair")
        if _nbytes(out) < pr.size * QUALITY_RESULT_BYTES:
            raise ValueError("output buffer too small")
        mo = -1 if max_offset_samples is None else int(max_offset_samples)
        check(self.lib.ffs_match_quality_batch(self.handle, rt[0].size, *[b.ctypes.data for b in rt], stb[0].size,
                                               *[b.ctypes.data for b in stb], pr.size, pr.ctypes.data, ps.ctypes.data, mo,
                                               int(top_k), int(exclusion_samples), match_algorithm_code(algorithm),
                                               out.data_ptr(), self._stream(stream)))


class ProgPlan(_SidePlan):
    """Owns one ``ffs_prog_plan``: ``max_slots`` files of a progressive solve (``progressive.py``), each a growing
    reference prefix of up to ``max_ref_samples`` against up to ``max_cand`` candidates of up to ``max_sub_samples``
    over up to ``max_lags`` lags.  Every call is queued on the stream; the host arrays are copied before it returns."""

    _create, _destroy, _workspace = "ffs_prog_plan_create", "ffs_prog_plan_destroy", "ffs_prog_plan_workspace_bytes"

    _limits = ("max_slots", "max_cand", "max_lags", "max_ref_samples", "max_sub_samples")

    def __init__(self, max_slots: int, max_cand: int, max_lags: int, max_ref_samples: int, max_sub_samples: int,
                 device: Optional[int] = None) -> None:
        super().__init__((max_slots, max_cand, max_lags, max_ref_samples, max_sub_samples), device)

    _OPEN_KINDS = (np.int32, np.int32, np.uint64, np.int64, np.float64, np.float64, np.float64, np.float64, np.int64)

    def _open(self, native, columns, kinds, stream) -> None:
        """Either open: the host columns in their dtypes (columns 2 to 5 are the candidate tables), one native call."""
        bufs = [np.ascontiguousarray(a, dtype=t) for a, t in zip(columns, kinds)]
        n = bufs[0].size
        if not all(b.size == (n * self.max_cand if 2 <= i <= 5 else n) for i, b in enumerate(bufs)):
            raise ValueError("one entry per slot, max_cand candidate entries per slot")
        check(native(self.handle, n, *[b.ctypes.data for b in bufs], self._stream(stream)))

    def _append(self, native, columns, kinds, top_k, exclusion_samples, cand_out, state_out, stream) -> None:
        """Either append: one entry per slot in every host column, room in both outputs, one native call."""
        bufs = [np.ascontiguousarray(a, dtype=t) for a, t in zip(columns, kinds)]
        n = bufs[0].size
        if not all(b.size == n for b in bufs):
            raise ValueError("one entry per slot")
        if _nbytes(cand_out) < n * self.max_cand * QUALITY_RESULT_BYTES or _nbytes(state_out) < n * PROG_STATE_BYTES:
            raise ValueError("output buffer too small")
        check(native(self.handle, n, *[b.ctypes.data for b in bufs], int(top_k), int(exclusion_samples),
                     cand_out.data_ptr(), state_out.data_ptr(), self._stream(stream)))

    def open(self, slot, n_cand, sub_ptr, sub_len, sub_lo, sub_hi, ref_lo, ref_hi, max_offset_samples,
             stream: Optional[int] = None) -> None:
        """``ffs_prog_open``: one entry per slot, and [n, max_cand] candidate tables (rows padded with anything)."""
        self._open(self.lib.ffs_prog_open, (slot, n_cand, sub_ptr, sub_len, sub_lo, sub_hi, ref_lo, ref_hi, max_offset_samples),
                   self._OPEN_KINDS, stream)

    def append(self, slot, chunk_ptr, first_bit, n_new, top_k: int, exclusion_samples: int, cand_out, state_out,
               stream: Optional[int] = None) -> None:
        """``ffs_prog_append`` into uint8 CUDA tensors of n * max_cand * 160 and n * 64 bytes (asynchronous)."""
        self._append(self.lib.ffs_prog_append, (slot, chunk_ptr, first_bit, n_new), (np.int32, np.uint64, np.int32, np.int64),
                     top_k, exclusion_samples, cand_out, state_out, stream)

    def reference(self, slot: int) -> Tuple[int, int]:
        """``ffs_prog_reference``: (device address of the plan's bits of the consumed prefix, its length)."""
        ptr, length = ctypes.c_void_p(), ctypes.c_int64()
        check(self.lib.ffs_prog_reference(self.handle, int(slot), ctypes.byref(ptr), ctypes.byref(length)))
        return int(ptr.value), int(length.value)

    def close_slots(self, slot) -> None:
        """``ffs_prog_close``."""
        buf = np.ascontiguousarray(slot, dtype=np.int32)
        check(self.lib.ffs_prog_close(self.handle, buf.size, buf.ctypes.data))

    def open_sampled(self, slot, n_cand, sub_ptr, sub_len, sub_lo, sub_hi, ref_lo, ref_hi, max_offset_samples, ref_total,
                     stream: Optional[int] = None) -> None:
        """``ffs_prog_open_sampled``: ``open`` plus the declared reference length of every slot."""
        self._open(self.lib.ffs_prog_open_sampled,
                   (slot, n_cand, sub_ptr, sub_len, sub_lo, sub_hi, ref_lo, ref_hi, max_offset_samples, ref_total),
                   self._OPEN_KINDS + (np.int64,), stream)

    def append_at(self, slot, chunk_ptr, first_bit, position, n_new, top_k: int, exclusion_samples: int, cand_out, state_out,
                  stream: Optional[int] = None) -> None:
        """``ffs_prog_append_at`` into uint8 CUDA tensors of n * max_cand * 160 and n * 64 bytes (asynchronous)."""
        self._append(self.lib.ffs_prog_append_at, (slot, chunk_ptr, first_bit, position, n_new),
                     (np.int32, np.uint64, np.int32, np.int64, np.int64), top_k, exclusion_samples, cand_out, state_out, stream)

    def known(self, slot: int):
        """``ffs_prog_known``: the merged known intervals of a sampled slot as an int64 array [n, 2], ascending."""
        buf, n = np.zeros((PROG_MAX_INTERVALS, 2), np.int64), ctypes.c_int()
        check(self.lib.ffs_prog_known(self.handle, int(slot), buf.ctypes.data, PROG_MAX_INTERVALS, ctypes.byref(n)))
        return buf[:n.value].copy()

    def sampled_bytes(self) -> int:
        """``ffs_prog_plan_sampled_bytes``."""
        return int(self.lib.ffs_prog_plan_sampled_bytes(self.handle))


class SidePlanCache:
    """The cached side plan of each (device, role) for one plan class: ``get`` hands it back while it ``fits`` the call
    and otherwise closes it and makes one of the call's size."""

    def __init__(self, plan_class) -> None:
        self.plan_class = plan_class
        self.plans: dict = {}

    def get(self, *dims, role: Optional[str] = None):
        dev = require_gpu().cuda.current_device()
        key = (dev, role)
        plan = self.plans.get(key)
        if plan is None or plan.handle is None or not plan.fits(*dims):
            if plan is not None:
                plan.close()
            plan = self.plans[key] = self.plan_class(*dims, device=dev)
        return plan

    def clear(self) -> None:
        for plan in self.plans.values():
            plan.close()
        self.plans.clear()


class Comm:
    """RCCL communicator behind ``ffs_gather_results`` (one per process / GPU).  ``unique_id()`` on rank 0,
    publish the 128 bytes (e.g. through torch.distributed's store), then ``Comm(rank, world, id)`` everywhere."""

    @staticmethod
    def unique_id() -> bytes:
        buf = ctypes.create_string_buffer(128)
        check(load().ffs_comm_unique_id(buf))
        return buf.raw

    def __init__(self, rank: int, world: int, uid: bytes, device: Optional[int] = None) -> None:
        torch = require_gpu()
        self.lib = load()
        self.rank, self.world = int(rank), int(world)
        self.device = torch.cuda.current_device() if device is None else int(device)
        if len(uid) != 128:
            raise ValueError("unique id must be 128 bytes")
        handle = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(uid, 128)
        check(self.lib.ffs_comm_create(self.device, self.rank, self.world, buf, ctypes.byref(handle)))
        self.handle = handle

    def gather_pair_results(self, local, out=None):
        """All-gather this rank's uint8 tensor of n*24 result bytes; returns world*n*24 bytes in rank order."""
        torch = require_gpu()
        n_local = local.numel() // 24
        if out is None:
            out = torch.empty(self.world * n_local * 24, dtype=torch.uint8, device=local.device)
        check(self.lib.ffs_gather_results(self.handle, local.data_ptr(), n_local, out.data_ptr(), current_stream_ptr(torch)))
        return out

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.ffs_comm_destroy(self.handle)
            self.handle = None

    def __del__(self) -> None:  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass
