"""Drift alignment you can trust: a quality report for every segment of a drift solve, evaluated ALONG its path.

A drift solve (``drift_align``) returns segments, the DP's total and block scores, and nothing that says whether a
segment is real, whether a jump between two segments is real, or whether the drift it followed is in the data or was
invented by a cheap ``step_cost``.  The piece reports (``split_report``) score a stretch at ONE lag; a drifting stretch
has no single lag, and its constant-lag curve is smeared over the lags its path visits.  This module reports, per
segment, the correlation curve of the segment's own samples over every SHIFT of its whole path that stays inside the
lag window -- computed exactly on the device from the drift solve's block counts (``csrc/ffs_drift_report.h``) in the
same call -- and derives:

    psr        = (peak1 - mean) / std                how far the best shift stands above the path curve
    margin     = (peak1 - peak2) / std               ... above the best shift >= E samples away
    gain_prev  = (own - prev) / std                  how much the segment prefers its own path to the path moved so
    gain_next  = (own - next) / std                  that it continues a neighbour without a jump
    drift_gain = (own - flat) / std                  how much the path beats the best CONSTANT lag among those it visits

A jump between segments i and i+1 is SUPPORTED when both sides prefer their own path: gain_next_i >= g and
gain_prev_{i+1} >= g (a NaN score -- the neighbour's path does not fit the window -- compares false).  A segment that
took a step but whose ``drift_gain`` is below the floor claims drift without evidence.  ``own_score`` is one fp64
expression of the segment's summed counts, so it is NOT in general the sum of the block scores (different rounding);
with 0/1 levels every term is an integer and the two are equal.

``checked_drift_sync`` applies the drift solve only when every segment and jump passes, and otherwise hands the
problem to ``split_report.checked_split_sync``.  Parity is against the in-repo numpy model
``tests/drift_report_model.py``, bit for bit.  ``drift_sync``, ``drift_align_batch`` and every existing entry point
are unchanged.
"""
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native, quality, split_report
from .constants import SAMPLE_RATE, candidate_ratios
from .drift_align import (DEFAULT_MAX_STEP, DEFAULT_STEP_COST, DriftResult, Segment, drift_outputs, drift_results,
                          map_cues_drift, validate_drift_args)
from .side_call import BlockCall, pairs_for_budget, record_lists
from .split_align import DEFAULT_BLOCK_SAMPLES, DEFAULT_SPLIT_PENALTY, _check_batch, solve_ratios

DEFAULT_TOP_K = quality.DEFAULT_TOP_K
DEFAULT_EXCLUSION_SAMPLES = quality.DEFAULT_EXCLUSION_SAMPLES
# Chosen on the CPU model (profiles/drift_report_calibration.py -> .json; SYNTHETIC data only, two-hour
# problems of workloads/drift.py, K = 1024, P = 8192, E = 300): see the table there for the class ranges each default
# sits between and the windows it holds for.
DEFAULT_MIN_SEGMENT_PSR = 6.0
DEFAULT_MIN_GAIN = 8.0
DEFAULT_MIN_DRIFT_GAIN = 0.5


@dataclass
class SegmentQuality:
    first_block: int
    end_block: int
    start_sample: int  # subtitle samples [start_sample, end_sample)
    end_sample: int
    first_offset: int  # offsets (samples) of the first and last block, and the least / greatest over the blocks
    last_offset: int
    min_offset: int
    max_offset: int
    own_score: float  # p(0): the path curve at the path itself
    prev_score: float  # p at the shift that continues the previous segment; NaN without it or outside the shift set
    next_score: float
    flat_score: float  # the best constant lag in [min_offset, max_offset] over the segment's samples
    flat_offset: int
    peaks: List[Tuple[float, int]]  # (score, shift in samples), the maximum first; shift 0 is the path itself
    mean: float
    std: float  # population standard deviation of the path curve over its n_lags shifts
    n_lags: int
    psr: float  # (peak1 - mean) / std; 0 when std == 0
    margin: float  # (peak1 - peak2) / std; +inf with one peak; 0 when std == 0
    gain_prev: float  # (own - prev) / std; NaN when prev is NaN, 0 when std == 0
    gain_next: float
    drift_gain: float  # (own - flat) / std; 0 when std == 0
    flags: int  # _native.QUALITY_FLAT / SEGMENT_OWN_NOT_PEAK

    @property
    def flat(self) -> bool:
        return bool(self.flags & _native.QUALITY_FLAT)

    @property
    def own_is_peak(self) -> bool:
        return not self.flags & _native.SEGMENT_OWN_NOT_PEAK

    @property
    def stepped(self) -> bool:
        return self.min_offset != self.max_offset


@dataclass
class DriftReport:
    drift: DriftResult  # what drift_align_batch returns for the pair, bit for bit
    segments: List[SegmentQuality]  # one per drift.segments entry, in order


@dataclass
class CheckedDriftResult:
    decision: str  # "drift", or checked_split_sync's "split", "single" or "untrusted"
    reasons: List[str]  # why the drift solve (and whatever else was tried) is not trusted; empty for "drift"
    ratio: float  # framerate ratio picked by the seven-ratio solve
    ratio_index: int
    global_offset: int  # that solve's single offset (samples)
    segments: List[Segment]  # the drift DP's segments (what drift_sync returns)
    segment_quality: List[SegmentQuality]
    supported: List[bool]  # per jump (between segments i and i+1)
    cue_start_us: np.ndarray  # output cue times (int64 microseconds) of the decision
    cue_end_us: np.ndarray
    cue_segment: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))  # piece index / -1 when not "drift"
    fallback: Optional[split_report.CheckedSplitResult] = None  # checked_split_sync's result when not "drift"


def validate_args(block_samples, max_offset_samples, split_penalty, max_step, step_cost, top_k, exclusion_samples) -> None:
    """Host-side checks of the call parameters (ValueError before any native call)."""
    split_report.validate_args(block_samples, max_offset_samples, split_penalty, top_k, exclusion_samples)
    validate_drift_args(max_step, step_cost)


def from_record(rec) -> SegmentQuality:
    """SegmentQuality of one ``_native.SEGMENT_REPORT_DTYPE`` record, with psr, margin and the gains derived on the
    host."""
    peaks = [(float(rec["peak_score"][i]), int(rec["peak_shift"][i])) for i in range(int(rec["n_peaks"]))]
    mean, std = float(rec["mean"]), float(rec["std"])
    own, prev, nxt = float(rec["own_score"]), float(rec["prev_score"]), float(rec["next_score"])
    flat_score = float(rec["flat_score"])
    psr, margin, flags, (gain_prev, gain_next) = quality.derive(peaks, mean, std, int(rec["flags"]), own, (prev, nxt))
    drift_gain = 0.0 if std == 0 or not peaks else (own - flat_score) / std
    return SegmentQuality(int(rec["first_block"]), int(rec["end_block"]), int(rec["start_sample"]),
                          int(rec["end_sample"]), int(rec["first_offset"]), int(rec["last_offset"]),
                          int(rec["min_offset"]), int(rec["max_offset"]), own, prev, nxt, flat_score,
                          int(rec["flat_offset"]), peaks, mean, std, int(rec["n_lags"]), psr, margin, gain_prev,
                          gain_next, drift_gain, flags)


def jump_support(segments: Sequence[SegmentQuality], min_gain: float = DEFAULT_MIN_GAIN) -> List[bool]:
    """Per jump (between segments i and i+1): both sides prefer their own path by at least ``min_gain`` std."""
    return [bool(a.gain_next >= min_gain and b.gain_prev >= min_gain) for a, b in zip(segments[:-1], segments[1:])]


def assess_drift(segments: Sequence[SegmentQuality], min_segment_psr: float = DEFAULT_MIN_SEGMENT_PSR,
                 min_gain: float = DEFAULT_MIN_GAIN, min_drift_gain: float = DEFAULT_MIN_DRIFT_GAIN) -> List[str]:
    """Reasons not to trust a drift solve, worded like ``split_report.assess_split``; an empty list means trust it.
    A segment took a step (o_b != o_{b-1} inside it) exactly when min_offset != max_offset."""
    reasons: List[str] = []
    for i, q in enumerate(segments):
        if q.flat:
            reasons.append("segment %d: flat correlation (std 0)" % i)
        elif q.psr < min_segment_psr:
            reasons.append("segment %d: psr %.1f < %.1f" % (i, q.psr, min_segment_psr))
    for i, (a, b) in enumerate(zip(segments[:-1], segments[1:])):
        if not (a.gain_next >= min_gain and b.gain_prev >= min_gain):
            reasons.append("jump %d (block %d): gain %.1f / %.1f < %.1f" % (i, b.first_block, a.gain_next, b.gain_prev,
                                                                             min_gain))
    for i, q in enumerate(segments):
        if q.stepped and not q.drift_gain >= min_drift_gain:
            reasons.append("segment %d: drift gain %.1f < %.1f" % (i, q.drift_gain, min_drift_gain))
    return reasons


_plans = _native.SidePlanCache(_native.DriftPlan)


def _get_plan(n_pairs: int, max_blocks: int, max_lags: int, max_samples: int, pairs_in_flight: Optional[int]):
    """The cached report plan of this device (its own: drift_align's plan never grows)."""
    if pairs_in_flight is None:  # drift_align's ~2.7 bytes per (block, lag), plus 8 fp64 rows of lags
        per_pair = max_blocks * (max_lags + 64) * 2.7 + (max_lags + 64) * 64 + 1
        pairs_in_flight = pairs_for_budget(n_pairs, per_pair)
    return _plans.get(pairs_in_flight, max_blocks, max_lags, max_samples)


def clear_plan_cache() -> None:
    _plans.clear()


def drift_report_batch(batch, max_offset_samples: int, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                       split_penalty: float = DEFAULT_SPLIT_PENALTY, max_step: int = DEFAULT_MAX_STEP,
                       step_cost: float = DEFAULT_STEP_COST, top_k: int = DEFAULT_TOP_K,
                       exclusion_samples: int = DEFAULT_EXCLUSION_SAMPLES, pairs_in_flight: Optional[int] = None,
                       raw: bool = False):
    """``drift_align.drift_align_batch`` (same inputs, same checks, bit-identical result) plus the path report of every
    segment, in one device call.  Returns one ``DriftReport`` per pair, or with ``raw`` (DriftResults,
    ``_native.SEGMENT_REPORT_DTYPE`` records [n_pairs, max_b], segment counts)."""
    validate_args(block_samples, max_offset_samples, split_penalty, max_step, step_cost, top_k, exclusion_samples)
    _check_batch(batch)
    call = BlockCall(batch, block_samples)
    w = int(max_offset_samples)
    plan = _get_plan(call.n, call.max_b, 2 * w, int(call.sub_len.max()), pairs_in_flight)
    outs = drift_outputs(call)
    rep, counts = call.records(_native.SEGMENT_REPORT_DTYPE), call.per_pair(np.int32)
    plan.report(*call.pair_arrays(), call.k, w, float(split_penalty), int(max_step), float(step_cost), int(top_k),
                int(exclusion_samples), *outs, rep, counts)
    res = drift_results(*outs, call.n_blocks, call.k, call.sub_len)
    recs, counts_h = call.read_records(rep, _native.SEGMENT_REPORT_DTYPE), counts.cpu().numpy()
    if raw:
        return res, recs, counts_h
    return [DriftReport(r, q) for r, q in zip(res, record_lists(recs, counts_h, from_record))]


def checked_drift_sync(problems, max_offset_seconds: float = 600, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                       split_penalty: float = DEFAULT_SPLIT_PENALTY, max_step: int = DEFAULT_MAX_STEP,
                       step_cost: float = DEFAULT_STEP_COST, top_k: int = DEFAULT_TOP_K,
                       exclusion_samples: int = DEFAULT_EXCLUSION_SAMPLES,
                       min_segment_psr: float = DEFAULT_MIN_SEGMENT_PSR, min_gain: float = DEFAULT_MIN_GAIN,
                       min_drift_gain: float = DEFAULT_MIN_DRIFT_GAIN,
                       min_piece_psr: float = split_report.DEFAULT_MIN_PIECE_PSR,
                       min_piece_gain: float = split_report.DEFAULT_MIN_GAIN, min_psr: float = quality.DEFAULT_MIN_PSR,
                       min_margin: float = quality.DEFAULT_MIN_MARGIN, sample_rate: int = SAMPLE_RATE,
                       ratios: Optional[Sequence[float]] = None) -> List[CheckedDriftResult]:
    """``drift_align.drift_sync`` with a decision per problem (``problems`` as it takes them):

    - "drift": every segment passes ``min_segment_psr``, every jump is supported by ``min_gain`` and every segment that
      took a step has ``drift_gain`` >= ``min_drift_gain`` -- the cue times of ``drift_sync``;
    - otherwise whatever ``split_report.checked_split_sync`` decides for that problem ("split", "single" or
      "untrusted", with ``min_piece_psr`` / ``min_piece_gain`` / ``min_psr`` / ``min_margin``): its cue times, its
      reasons appended to the drift solve's.  Only the problems not decided "drift" are sent there."""
    w = int(round(max_offset_seconds * sample_rate))
    validate_args(block_samples, w, split_penalty, max_step, step_cost, top_k, exclusion_samples)
    ratios = list(candidate_ratios() if ratios is None else ratios)
    db, best, pres = solve_ratios(problems, w, ratios, sample_rate)
    reps = drift_report_batch(db.select_candidates(best), w, block_samples, split_penalty, max_step, step_cost, top_k,
                              exclusion_samples)
    out: List[Optional[CheckedDriftResult]] = []
    rest = []
    for p, ((_, (start_us, end_us, _meta)), rep) in enumerate(zip(problems, reps)):
        ratio = ratios[int(best[p])]
        reasons = assess_drift(rep.segments, min_segment_psr, min_gain, min_drift_gain)
        cs = ce = which = np.zeros(0, np.int64)
        if reasons:
            rest.append(p)
        else:
            cs, ce, which = map_cues_drift(start_us, end_us, ratio, rep.drift, block_samples, sample_rate)
        out.append(CheckedDriftResult("drift", reasons, ratio, int(best[p]), int(pres[p]["offset"]), rep.drift.segments,
                                      rep.segments, jump_support(rep.segments, min_gain), cs, ce, which))
    if rest:
        fall = split_report.checked_split_sync([problems[p] for p in rest], max_offset_seconds, block_samples,
                                               split_penalty, top_k, exclusion_samples, min_piece_psr, min_piece_gain,
                                               min_psr, min_margin, sample_rate, ratios)
        for p, f in zip(rest, fall):
            r = out[p]
            r.decision, r.reasons, r.fallback = f.decision, r.reasons + f.reasons, f
            r.cue_start_us, r.cue_end_us, r.cue_segment = f.cue_start_us, f.cue_end_us, f.cue_piece
    return out
