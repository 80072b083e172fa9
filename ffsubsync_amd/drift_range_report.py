"""Range drift you can trust: a quality report for every segment of a drift solve over any lag range, and a decision
per file.

``cut_drift_sync`` rewrites every cue from a path found among about 10^9 (block, lag) cells, and nothing says whether a
segment, a jump or the drift it followed is real; a subtitle of another film still gets a tidy path.  ``drift_report``
evaluates a segment ALONG its path, but only inside the +-131 072-sample window of ``drift_align``, from that solve's
stored block counts; the range solve (``drift_range``) stores none.  Here the same record (``ffs_segment_report``,
``drift_report.SegmentQuality`` through the unchanged ``from_record``) is computed as a post-pass over a finished path
over its pair's lag range [lag_lo, lag_hi], n11 counted exactly from the bits (``csrc/ffs_drift_range_report.h``): the
path curve over every shift that keeps the whole path inside the range, its moments and peaks, the curve at the shifts
that would continue a neighbouring segment without a jump, and the best constant lag among those the path visits.

``checked_cut_drift_sync`` applies ``cut_drift_sync``'s cue times only when ``drift_report.assess_drift`` finds no
reason under THIS module's defaults (the full range needs its own: DESIGN 3.17), and otherwise hands the problem to
``cut_report.checked_cut_sync``.  Parity is against the in-repo numpy model ``tests/drift_range_report_model.py``, bit
for bit, and against the independent reference ``tests/report_reference.py``.  Every existing entry point is unchanged.
"""
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native, cut_report, quality, split_refine
from .constants import SAMPLE_RATE, candidate_ratios
from .cut_align import DEFAULT_CUT_PENALTY, full_range, lag_arrays, solve_ratios_windowless, validate_range
from .cut_align import validate_args as validate_cut_args
from .cut_report import _records
from .drift_align import (DEFAULT_MAX_STEP, DriftResult, Segment, drift_outputs, drift_results, map_cues_drift,
                          validate_drift_args)
from .drift_range import DEFAULT_RANGE_STEP_COST, workspace_per_pair
from .drift_report import DriftReport, SegmentQuality, assess_drift, from_record, jump_support
from .side_call import BlockCall, pairs_for_budget, record_lists
from .split_align import DEFAULT_BLOCK_SAMPLES, _check_batch

DEFAULT_TOP_K = quality.DEFAULT_TOP_K
DEFAULT_EXCLUSION_SAMPLES = quality.DEFAULT_EXCLUSION_SAMPLES
ROUND_SEGMENTS = _native.RPATH_ROUND_SEGMENTS  # segment rows per pair and round of the device report
# Chosen on the CPU model over the full range (profiles/drift_range_report_calibration.py -> .json;
# SYNTHETIC data only: one-hour problems of workloads/cut_drift.py, K = 1024, P = 8192, max_step 2, step_cost 64,
# E = 300).  Segment psr: wrong pairs 4.57 .. 6.50, every other class 12.3 .. 30.4.  Jump gain: wrong pairs 2.89 .. 6.83,
# the other classes 8.53 .. 26.9 (3.9's 6.0 for breaks would pass 7 jumps of wrong pairs).  Drift gain of stepping
# segments: invented steps (clean files at step_cost 32) 0.009 .. 0.018, real drift with three steps or more 0.119 ..
# 8.32 (3.11's 0.5 would refuse 11 real segments here: one-hour segments between inserts take 3 .. 28 steps).
DEFAULT_MIN_SEGMENT_PSR = 9.0
DEFAULT_MIN_GAIN = 8.0
DEFAULT_MIN_DRIFT_GAIN = 0.05


@dataclass
class CheckedCutDriftResult:
    decision: str  # "drift", or checked_cut_sync's "cut", "single" or "untrusted"
    reasons: List[str]  # why the drift solve (and whatever else was tried) is not trusted; empty for "drift"
    ratio: float  # framerate ratio picked by the windowless seven-ratio solve
    ratio_index: int
    global_offset: int  # that solve's single offset (samples)
    lag_range: Tuple[int, int]  # the drift solve's lag range
    segments: List[Segment]  # the range drift DP's segments (what cut_drift_sync returns)
    total: float
    segment_quality: List[SegmentQuality]
    supported: List[bool]  # per jump (between segments i and i+1)
    cue_start_us: np.ndarray  # output cue times (int64 microseconds) of the decision
    cue_end_us: np.ndarray
    cue_segment: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))  # piece index / -1 when not "drift"
    fallback: Optional[cut_report.CheckedCutResult] = None  # checked_cut_sync's result when not "drift"


def validate_args(block_samples, split_penalty, max_step, step_cost, top_k, exclusion_samples) -> None:
    """Host-side checks of the call parameters (ValueError before any native call)."""
    validate_cut_args(block_samples, split_penalty)
    validate_drift_args(max_step, step_cost)
    quality.validate_args(None, top_k, exclusion_samples)


_plans = _native.SidePlanCache(_native.DriftRangePlan)


def _get_plan(n_pairs: int, max_blocks: int, max_lags: int, max_samples: int, max_step: int,
              pairs_in_flight: Optional[int]):
    """The report's own plan (drift_range's never grows), sized for the rows its first report call adds: 8 rows of 12
    bytes per lag and pair."""
    if pairs_in_flight is None:  # drift_range's workspace plus the rows (~138 MB per 2 h full-range pair) in ~12 GiB
        per_pair = (workspace_per_pair(max_blocks, max_lags, max_samples, max_step)
                    + ROUND_SEGMENTS * (max_lags + 65) * 12.0 + (max_samples / 8192.0 + 2 * max_blocks + 2) * 32.0)
        pairs_in_flight = pairs_for_budget(n_pairs, per_pair)
    return _plans.get(pairs_in_flight, max_blocks, max_lags, max_samples, max_step)


def clear_plan_cache() -> None:
    _plans.clear()


def drift_range_path_report_batch(batch, results_or_offsets_and_jumps, lag_ranges=None,
                                  block_samples: int = DEFAULT_BLOCK_SAMPLES, top_k: int = DEFAULT_TOP_K,
                                  exclusion_samples: int = DEFAULT_EXCLUSION_SAMPLES,
                                  pairs_in_flight: Optional[int] = None, raw: bool = False):
    """The segment path reports of GIVEN paths over ``lag_ranges`` (as ``drift_range.drift_align_range_batch`` takes
    them): one ``DriftResult`` per pair, or a pair (block offsets, jump flags) of one array of B_p entries per pair;
    every offset inside its pair's range.  Returns one list of ``SegmentQuality`` per pair, or with ``raw``
    (``_native.SEGMENT_REPORT_DTYPE`` records [n_pairs, max_b], segment counts)."""
    validate_args(block_samples, 0.0, 0, 0.0, top_k, exclusion_samples)
    _check_batch(batch)
    lo, hi = lag_arrays(batch, lag_ranges)
    call = BlockCall(batch, block_samples)
    given = results_or_offsets_and_jumps
    if isinstance(given, tuple) and len(given) == 2 and not isinstance(given[0], DriftResult):
        all_offs, all_jumps = given
    else:
        all_offs, all_jumps = [r.block_offsets for r in given], [r.block_jump for r in given]
    if len(all_offs) != call.n or len(all_jumps) != call.n:
        raise ValueError("one path per pair")
    all_offs = [np.asarray(o, dtype=np.int64) for o in all_offs]
    all_jumps = [np.asarray(j) != 0 for j in all_jumps]
    what = lambda p, _size, blocks: ("pair %d: %d block offsets and %d jump flags for %d blocks"
                                     % (p, min(all_offs[p].size, blocks), min(all_jumps[p].size, blocks), blocks))
    path = call.place(what, (all_offs, np.int32), (all_jumps, np.uint8), clip=True)
    plan = _get_plan(call.n, call.max_b, *call.lag_dims(lo, hi), 0, pairs_in_flight)
    recs, counts = _records(call, plan, _native.SEGMENT_REPORT_DTYPE, lo, hi, path, top_k, exclusion_samples)
    if raw:
        return recs, counts
    return record_lists(recs, counts, from_record)


def drift_range_report_batch(batch, lag_ranges=None, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                             split_penalty: float = DEFAULT_CUT_PENALTY, max_step: int = DEFAULT_MAX_STEP,
                             step_cost: float = DEFAULT_RANGE_STEP_COST, top_k: int = DEFAULT_TOP_K,
                             exclusion_samples: int = DEFAULT_EXCLUSION_SAMPLES, pairs_in_flight: Optional[int] = None,
                             raw: bool = False):
    """``drift_range.drift_align_range_batch`` (same inputs, same checks, bit-identical result) plus the path report of
    every segment over the pair's lag range, on one plan.  Returns one ``drift_report.DriftReport`` per pair, or with
    ``raw`` (DriftResults, ``_native.SEGMENT_REPORT_DTYPE`` records [n_pairs, max_b], segment counts)."""
    validate_args(block_samples, split_penalty, max_step, step_cost, top_k, exclusion_samples)
    _check_batch(batch)
    lo, hi = lag_arrays(batch, lag_ranges)
    call = BlockCall(batch, block_samples)
    plan = _get_plan(call.n, call.max_b, *call.lag_dims(lo, hi), int(max_step), pairs_in_flight)
    offs, scores, jumps, totals = drift_outputs(call)
    plan.align(*call.pair_arrays(), call.k, lo, hi, float(split_penalty), int(max_step), float(step_cost), offs, scores,
               jumps, totals)
    recs, counts = _records(call, plan, _native.SEGMENT_REPORT_DTYPE, lo, hi, (offs, jumps), top_k, exclusion_samples)
    res = drift_results(offs, scores, jumps, totals, call.n_blocks, call.k, call.sub_len)
    if raw:
        return res, recs, counts
    return [DriftReport(r, q) for r, q in zip(res, record_lists(recs, counts, from_record))]


def checked_cut_drift_sync(problems, lag_range=None, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                           split_penalty: float = DEFAULT_CUT_PENALTY, max_step: int = DEFAULT_MAX_STEP,
                           step_cost: float = DEFAULT_RANGE_STEP_COST, top_k: int = DEFAULT_TOP_K,
                           exclusion_samples: int = DEFAULT_EXCLUSION_SAMPLES,
                           min_segment_psr: float = DEFAULT_MIN_SEGMENT_PSR, min_gain: float = DEFAULT_MIN_GAIN,
                           min_drift_gain: float = DEFAULT_MIN_DRIFT_GAIN,
                           min_piece_psr: float = cut_report.DEFAULT_MIN_PIECE_PSR,
                           min_piece_gain: float = cut_report.DEFAULT_MIN_GAIN,
                           min_coverage: float = cut_report.DEFAULT_MIN_COVERAGE,
                           radius_samples: int = split_refine.DEFAULT_RADIUS_SAMPLES,
                           unmatched_margin: Optional[float] = split_refine.DEFAULT_UNMATCHED_MARGIN,
                           sample_rate: int = SAMPLE_RATE,
                           ratios: Optional[Sequence[float]] = None) -> List[CheckedCutDriftResult]:
    """``drift_range.cut_drift_sync`` with a decision per problem (``problems`` as it takes them):

    - "drift": every segment passes ``min_segment_psr``, every jump is supported by ``min_gain`` and every segment that
      took a step has ``drift_gain`` >= ``min_drift_gain`` -- the cue times of ``cut_drift_sync``;
    - otherwise whatever ``cut_report.checked_cut_sync`` decides for that problem ("cut", "single" or "untrusted", with
      ``min_piece_psr`` / ``min_piece_gain`` / ``min_coverage`` / ``radius_samples`` / ``unmatched_margin``): its cue
      times, its reasons appended to the drift solve's.  Only the problems not decided "drift" are sent there."""
    validate_args(block_samples, split_penalty, max_step, step_cost, top_k, exclusion_samples)
    split_refine.validate_args(block_samples, radius_samples, unmatched_margin)
    validate_thresholds(min_segment_psr, min_gain, min_drift_gain)
    cut_report.validate_thresholds(min_piece_psr, min_piece_gain, min_coverage)
    if lag_range is not None:
        lag_range = validate_range(lag_range)
    ratios = list(candidate_ratios() if ratios is None else ratios)
    db, best, pres = solve_ratios_windowless(problems, ratios, sample_rate)
    chosen = db.select_candidates(best)
    reps = drift_range_report_batch(chosen, lag_range, block_samples, split_penalty, max_step, step_cost, top_k,
                                    exclusion_samples)
    out: List[CheckedCutDriftResult] = []
    rest = []
    for p, ((_, (start_us, end_us, _meta)), rep) in enumerate(zip(problems, reps)):
        ratio = ratios[int(best[p])]
        reasons = assess_drift(rep.segments, min_segment_psr, min_gain, min_drift_gain)
        cs = ce = which = np.zeros(0, np.int64)
        if reasons:
            rest.append(p)
        else:
            cs, ce, which = map_cues_drift(start_us, end_us, ratio, rep.drift, block_samples, sample_rate)
        rng = lag_range if lag_range is not None else full_range(chosen.lens[p, 0], chosen.lens[p, 1])
        out.append(CheckedCutDriftResult("drift", reasons, ratio, int(best[p]), int(pres[p]["offset"]), rng,
                                         rep.drift.segments, rep.drift.total, rep.segments,
                                         jump_support(rep.segments, min_gain), cs, ce, which))
    if rest:
        fall = cut_report.checked_cut_sync([problems[p] for p in rest], lag_range, block_samples, split_penalty,
                                           radius_samples, unmatched_margin, sample_rate, ratios, top_k,
                                           exclusion_samples, min_piece_psr, min_piece_gain, min_coverage)
        for p, f in zip(rest, fall):
            r = out[p]
            r.decision, r.reasons, r.fallback = f.decision, r.reasons + f.reasons, f
            r.cue_start_us, r.cue_end_us, r.cue_segment = f.cue_start_us, f.cue_end_us, f.cue_piece
    return out


def validate_thresholds(min_segment_psr, min_gain, min_drift_gain) -> None:
    """Host-side checks of the drift decision's thresholds (ValueError)."""
    for name, v in (("min_segment_psr", min_segment_psr), ("min_gain", min_gain), ("min_drift_gain", min_drift_gain)):
        if not cut_report._real(v):
            raise ValueError("%s=%r: need a number (not NaN)" % (name, v))


def decide_drift(segments: Sequence[SegmentQuality], min_segment_psr: float = DEFAULT_MIN_SEGMENT_PSR,
                 min_gain: float = DEFAULT_MIN_GAIN,
                 min_drift_gain: float = DEFAULT_MIN_DRIFT_GAIN) -> Tuple[bool, List[str]]:
    """(whether ``checked_cut_drift_sync`` applies the drift solve, ``assess_drift``'s reasons) under this module's
    defaults."""
    validate_thresholds(min_segment_psr, min_gain, min_drift_gain)
    reasons = assess_drift(segments, min_segment_psr, min_gain, min_drift_gain)
    return not reasons, reasons
