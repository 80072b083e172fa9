"""Smooth drift alignment: each segment of a drift solve fitted as a polyline of knots.

``drift_align`` follows a residual framerate ratio or a wandering clock with a staircase: its DP pays ``step_cost`` for
every sample of movement, so the path lags behind a steady drift, and ``map_cues_drift`` shifts a cue by the integer
offset of its block.  Here every segment's path is replaced by a polyline through a knot every ``knot_blocks`` blocks.
The knots' lags are searched within ``radius`` samples of the path, every line between two knots is scored on the same
block counts the DP used (its blocks' counts summed, scored once), and only BENDING is penalised (``bend_cost`` per
sample of slope change per ``knot_blocks`` blocks): a straight line of any slope costs nothing, and a clean file stays
where it is because every departure from a straight path bends at least twice.  The search is an exact Viterbi pass
on the device (``csrc/ffs_drift_smooth.h``) in the same call as the drift solve; ``map_cues_smooth`` then interpolates
between knot block centres, so the output has no steps inside a segment.

Upstream has no equivalent, so parity is against the in-repo numpy model (``tests/drift_smooth_model.py``), bit for bit.
The drift solve inside is ``drift_align_batch``'s, bit for bit; ``drift_sync``, ``checked_drift_sync`` and every
existing entry point are unchanged.  Limits: the fit cannot move a knot further than ``radius`` from the DP's path, so
where the path itself is far from the truth (file ends of strongly wobbling clocks) the error stays.
"""
import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from .constants import SAMPLE_RATE, candidate_ratios
from .drift_align import (DEFAULT_MAX_STEP, DEFAULT_STEP_COST, DriftResult, DriftSyncResult, drift_outputs,
                          drift_results, validate_drift_args)
from .side_call import BlockCall, pairs_for_budget
from .split_align import (DEFAULT_BLOCK_SAMPLES, DEFAULT_SPLIT_PENALTY, _check_batch, _scaled_us, solve_ratios,
                          validate_args)

# Chosen on the CPU model by profiles/drift_smooth_calibration.py over workloads/drift.py
# (profiles/drift_smooth_calibration.json): the smallest power-of-two bend cost at which every one of the 40
# clean pairs keeps smooth_offset == block_offset on every block (and does so at every larger cost tried), then the
# (knot_blocks, radius) with the lowest mean block error on the drifting set.  The calibration data are SYNTHETIC.
DEFAULT_KNOT_BLOCKS = 16
DEFAULT_RADIUS = 16
DEFAULT_BEND_COST = 64.0


@dataclass
class SmoothSegment:
    """The fitted polyline of one segment [first_block, end_block) of the drift solve."""

    first_block: int
    end_block: int
    knots: List[Tuple[int, int]]  # (block, offset in samples), in block order; one entry for a one-block segment
    fit_total: float  # line scores minus bend costs, the Viterbi maximum
    line_score: float
    bend_total: float
    ratios: List[float]  # per interval between two knots: 1 + (c_{i+1} - c_i) / (n_i * block_samples)


@dataclass
class SmoothResult:
    drift: DriftResult  # what drift_align_batch returns for the pair, bit for bit
    smooth_offsets: np.ndarray  # int32 [B]: the fitted lag of every block
    knot: np.ndarray  # uint8 [B]: 1 where the block is a knot
    segments: List[SmoothSegment]  # one per drift.segments entry, in order


@dataclass
class SmoothSyncResult(DriftSyncResult):
    smooth_segments: List[SmoothSegment] = field(default_factory=list)


def validate_smooth_args(knot_blocks, radius, bend_cost) -> None:
    """Host-side checks of the three fit parameters (ValueError before any native call)."""
    for name, v, lo, hi in (("knot_blocks", knot_blocks, 1, _native.SMOOTH_MAX_KNOT_BLOCKS),
                            ("radius", radius, 0, _native.SMOOTH_MAX_RADIUS)):
        try:
            i = int(v)
        except (TypeError, ValueError, OverflowError):
            i = None
        if i is None or i != v or not lo <= i <= hi:
            raise ValueError("%s=%r: need an integer in [%d, %d]" % (name, v, lo, hi))
    try:
        lam = float(bend_cost)
    except (TypeError, ValueError):
        lam = math.nan
    if math.isnan(lam) or math.isinf(lam) or lam < 0:
        raise ValueError("bend_cost=%r: need a finite number >= 0" % (bend_cost,))


def smooth_segments_from_blocks(drift: DriftResult, smooth_offsets, knot, records,
                                block_samples: int = DEFAULT_BLOCK_SAMPLES) -> List[SmoothSegment]:
    """SmoothSegments of one pair from its per-block outputs and ``_native.SMOOTH_SEGMENT_DTYPE`` records."""
    out = []
    for seg, rec in zip(drift.segments, records):
        blocks = [b for b in range(seg.first_block, seg.end_block) if knot[b]]
        if len(blocks) != int(rec["n_knots"]):
            raise ValueError("segment at block %d: %d knot flags, record says %d" % (seg.first_block, len(blocks),
                                                                                    int(rec["n_knots"])))
        knots = [(b, int(smooth_offsets[b])) for b in blocks]
        ratios = [1.0 + (c1 - c0) / float((b1 - b0) * block_samples) for (b0, c0), (b1, c1) in zip(knots[:-1], knots[1:])]
        out.append(SmoothSegment(seg.first_block, seg.end_block, knots, float(rec["fit_total"]), float(rec["line_score"]),
                                 float(rec["bend_total"]), ratios))
    return out


_plans = _native.SidePlanCache(_native.DriftPlan)


def _get_plan(n_pairs: int, max_blocks: int, max_lags: int, max_samples: int, pairs_in_flight: Optional[int]):
    """The cached smooth plan of this device (its own: drift_align's plan never grows)."""
    if pairs_in_flight is None:  # drift_align's ~2.7 bytes per (block, lag), plus the fit's tables per block
        per_pair = max_blocks * (max_lags + 64) * 2.7 + max_blocks * _native.SMOOTH_BLOCK_BYTES + 1
        pairs_in_flight = pairs_for_budget(n_pairs, per_pair)
    return _plans.get(pairs_in_flight, max_blocks, max_lags, max_samples)


def clear_plan_cache() -> None:
    _plans.clear()


def smooth_align_batch(batch, max_offset_samples: int, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                       split_penalty: float = DEFAULT_SPLIT_PENALTY, max_step: int = DEFAULT_MAX_STEP,
                       step_cost: float = DEFAULT_STEP_COST, knot_blocks: int = DEFAULT_KNOT_BLOCKS,
                       radius: int = DEFAULT_RADIUS, bend_cost: float = DEFAULT_BEND_COST,
                       pairs_in_flight: Optional[int] = None, raw: bool = False):
    """``drift_align.drift_align_batch`` (same inputs, same checks, bit-identical result) plus the smooth fit of every
    segment, in one asynchronous device call.  Returns one ``SmoothResult`` per pair, or with ``raw`` (DriftResults,
    smooth offsets [n_pairs, max_b] int32, knot flags [n_pairs, max_b] uint8, ``_native.SMOOTH_SEGMENT_DTYPE`` records
    [n_pairs, max_b], segment counts)."""
    validate_args(block_samples, max_offset_samples, split_penalty)
    validate_drift_args(max_step, step_cost)
    validate_smooth_args(knot_blocks, radius, bend_cost)
    _check_batch(batch)
    call = BlockCall(batch, block_samples)
    w = int(max_offset_samples)
    plan = _get_plan(call.n, call.max_b, 2 * w, int(call.sub_len.max()), pairs_in_flight)
    return _smooth(call, plan, (w,), (float(split_penalty), int(max_step), float(step_cost), int(knot_blocks), int(radius),
                                      float(bend_cost)), raw)


def _smooth(call: BlockCall, plan, window_args, fit_args, raw: bool):
    """The device call and read-back of both smooth entry points, this one and ``drift_range_smooth``'s:
    ``plan.smooth`` with the lag set as the plan takes it (``window_args``: (W,) or (lag_lo, lag_hi)), then the cost
    and fit parameters ``fit_args``."""
    outs = drift_outputs(call)
    smooth, knot = call.per_block(np.int32), call.per_block(np.uint8)
    rec, counts = call.records(_native.SMOOTH_SEGMENT_DTYPE), call.per_pair(np.int32)
    plan.smooth(*call.pair_arrays(), call.k, *window_args, *fit_args, *outs, smooth, knot, rec, counts)
    res = drift_results(*outs, call.n_blocks, call.k, call.sub_len)
    smooth_h, knot_h = call.read_blocks(smooth), call.read_blocks(knot)
    recs, counts_h = call.read_records(rec, _native.SMOOTH_SEGMENT_DTYPE), counts.cpu().numpy()
    if raw:
        return res, smooth_h, knot_h, recs, counts_h
    out = []
    for p, r in enumerate(res):
        nb = int(call.n_blocks[p])
        if int(counts_h[p]) != len(r.segments):
            raise RuntimeError("pair %d: %d segments on the device, %d on the host" % (p, int(counts_h[p]), len(r.segments)))
        so, kn = smooth_h[p, :nb].copy(), knot_h[p, :nb].copy()
        out.append(SmoothResult(r, so, kn, smooth_segments_from_blocks(r, so, kn, recs[p, :len(r.segments)], call.k)))
    return out


def polyline_shift(segment: SmoothSegment, sample: float, block_samples: int = DEFAULT_BLOCK_SAMPLES) -> float:
    """The segment's polyline at ``sample`` (fp64 samples): linear between knot block centres (k_i + 1/2) K, continued
    with the end intervals' slopes outside them; the offset itself for a one-knot segment."""
    knots = segment.knots
    if len(knots) == 1:
        return float(knots[0][1])
    x = [(b + 0.5) * block_samples for b, _ in knots]
    i = int(np.searchsorted(np.array(x[1:-1]), sample, side="right"))  # interval: clamped to the first and the last
    c0, c1 = knots[i][1], knots[i + 1][1]
    return c0 + (c1 - c0) * ((sample - x[i]) / (x[i + 1] - x[i]))


def map_cues_smooth(start_us, end_us, ratio: float, result: SmoothResult, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                    sample_rate: int = SAMPLE_RATE):
    """Output times of every cue: scaled by ``ratio`` as ``split_align.map_cues`` scales it, its scaled start sample
    found by the same rounding, its segment by the block that holds that sample (clamped to the file); the shift is the
    segment's polyline at that sample (``polyline_shift``), converted to whole microseconds once, half to even.  Start
    and end of a cue get the same shift.  Returns (start_us, end_us, segment index) int64 arrays."""
    from datetime import timedelta

    segs = result.segments
    if not segs:
        raise ValueError("no segments")
    first = np.array([s.first_block for s in segs], dtype=np.int64)
    n_blocks = segs[-1].end_block
    n = len(start_us)
    out_s, out_e, which = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        s_us, e_us = _scaled_us(start_us[i], ratio), _scaled_us(end_us[i], ratio)
        sample = int(round(timedelta(microseconds=s_us).total_seconds() * sample_rate))
        block = min(max(sample // block_samples, 0), n_blocks - 1)
        k = int(np.searchsorted(first, block, side="right")) - 1
        shift_us = int(round(polyline_shift(segs[k], float(sample), block_samples) * 1e6 / sample_rate))
        out_s[i] = s_us + shift_us
        out_e[i] = e_us + shift_us
        which[i] = k
    return out_s, out_e, which


def smooth_sync(problems, max_offset_seconds: float = 600, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                split_penalty: float = DEFAULT_SPLIT_PENALTY, max_step: int = DEFAULT_MAX_STEP,
                step_cost: float = DEFAULT_STEP_COST, knot_blocks: int = DEFAULT_KNOT_BLOCKS,
                radius: int = DEFAULT_RADIUS, bend_cost: float = DEFAULT_BEND_COST, sample_rate: int = SAMPLE_RATE,
                ratios: Optional[Sequence[float]] = None) -> List[SmoothSyncResult]:
    """``drift_align.drift_sync`` with the smooth fit in the middle: the seven-ratio solve, the drift DP and the knot fit
    of every segment in one device call, and every cue's output time from the fitted polyline."""
    w = int(round(max_offset_seconds * sample_rate))
    validate_args(block_samples, w, split_penalty)
    validate_drift_args(max_step, step_cost)
    validate_smooth_args(knot_blocks, radius, bend_cost)
    ratios = list(candidate_ratios() if ratios is None else ratios)
    db, best, pres = solve_ratios(problems, w, ratios, sample_rate)
    results = smooth_align_batch(db.select_candidates(best), w, block_samples, split_penalty, max_step, step_cost,
                                 knot_blocks, radius, bend_cost)
    out = []
    for p, ((_, (start_us, end_us, _meta)), res) in enumerate(zip(problems, results)):
        ratio = ratios[int(best[p])]
        cs, ce, which = map_cues_smooth(start_us, end_us, ratio, res, block_samples, sample_rate)
        out.append(SmoothSyncResult(ratio, int(best[p]), int(pres[p]["offset"]), res.drift.segments, res.drift.total, cs, ce,
                                    which, res.segments))
    return out
