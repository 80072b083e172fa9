"""Smooth drift alignment over any lag range: the polyline fit for subtitles made for another cut AND re-encoded.

``cut_drift_sync`` is the only solver for such files, and its output is a staircase: the range drift DP pays
``step_cost`` for every sample of movement, so its path lags behind a steady drift, and ``map_cues_drift`` shifts a cue
by the whole-sample offset of its block.  ``drift_smooth`` cures that inside +-131 072 samples by fitting each
segment's path as a polyline of knots on the stored block counts; the range solve stores no counts.  Here the same fit
runs behind the range solve, in the same device call (``csrc/ffs_drift_range_smooth.h``): n11 is counted again in a
band of a few dozen lags around the solved path, and a knot candidate is valid where it lies inside the pair's lag
range.  Everything else -- segments, knot blocks, digital lines, the bend cost, the Viterbi pass, the tie rule -- is
``drift_smooth``'s.

Parity is against the in-repo numpy model ``tests/drift_range_smooth_model.py``, bit for bit; the four drift outputs
equal ``drift_align_range_batch``'s, and at [-W+1, W] all eight outputs equal ``smooth_align_batch``'s.
``cut_drift_sync``, ``smooth_sync`` and every existing entry point are unchanged.
"""
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _native
from .constants import SAMPLE_RATE, candidate_ratios
from .cut_align import (DEFAULT_CUT_PENALTY, full_range, lag_arrays, solve_ratios_windowless, validate_args,
                        validate_range)
from .drift_align import DEFAULT_MAX_STEP, validate_drift_args
from .drift_range import DEFAULT_RANGE_STEP_COST, CutDriftSyncResult, workspace_per_pair
from .drift_smooth import SmoothSegment, _smooth, map_cues_smooth, validate_smooth_args
from .side_call import BlockCall, pairs_for_budget
from .split_align import DEFAULT_BLOCK_SAMPLES, _check_batch

# UNCALIBRATED: these are drift_smooth's defaults.  profiles/drift_range_smooth_calibration.py applied drift_smooth's
# rule on the CPU model over workloads/cut_drift.py (profiles/drift_range_smooth_calibration.json) and it
# chose nothing: at every (knot_blocks, radius) tried some clean problem leaves its path at every bend cost -- a whole
# segment moves by one sample where two neighbouring lags tie, or a short segment tilts along a straight line; neither
# bends, so neither costs anything.  At these
# values the model's mean block error falls from 5.73 to 3.69 samples on the drifting set (one of 16 problems gets
# worse) and from 3.35 to 0.77 on the steep set (every one of 8 gains).  The calibration data are SYNTHETIC.
DEFAULT_RANGE_KNOT_BLOCKS = 16
DEFAULT_RANGE_RADIUS = 16
DEFAULT_RANGE_BEND_COST = 64.0


@dataclass
class SmoothCutSyncResult(CutDriftSyncResult):
    smooth_segments: List[SmoothSegment] = field(default_factory=list)
    smooth_offsets: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))  # int32 [B]: every block's fitted lag


_plans = _native.SidePlanCache(_native.DriftRangePlan)


def _get_plan(n_pairs: int, max_blocks: int, max_lags: int, max_samples: int, max_step: int,
              pairs_in_flight: Optional[int]):
    """The cached smooth plan of this device (its own: drift_range's plan never grows)."""
    if pairs_in_flight is None:  # drift_range's bound, plus the fit's tables and band rows per block
        per_pair = (workspace_per_pair(max_blocks, max_lags, max_samples, max_step)
                    + (max_blocks + 15) * (_native.SMOOTH_BLOCK_BYTES + 2 * _native.range_band_row(
                        max_step, _native.SMOOTH_MAX_KNOT_BLOCKS, _native.SMOOTH_MAX_RADIUS)))
        pairs_in_flight = pairs_for_budget(n_pairs, per_pair)
    return _plans.get(pairs_in_flight, max_blocks, max_lags, max_samples, max_step)


def clear_plan_cache() -> None:
    _plans.clear()


def smooth_align_range_batch(batch, lag_ranges=None, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                             split_penalty: float = DEFAULT_CUT_PENALTY, max_step: int = DEFAULT_MAX_STEP,
                             step_cost: float = DEFAULT_RANGE_STEP_COST, knot_blocks: int = DEFAULT_RANGE_KNOT_BLOCKS,
                             radius: int = DEFAULT_RANGE_RADIUS, bend_cost: float = DEFAULT_RANGE_BEND_COST,
                             pairs_in_flight: Optional[int] = None, raw: bool = False):
    """``drift_range.drift_align_range_batch`` (same inputs, same checks, bit-identical result) plus the smooth fit of
    every segment, in one asynchronous device call.  Returns one ``drift_smooth.SmoothResult`` per pair, or with ``raw``
    (DriftResults, smooth offsets [n_pairs, max_b] int32, knot flags [n_pairs, max_b] uint8,
    ``_native.SMOOTH_SEGMENT_DTYPE`` records [n_pairs, max_b], segment counts)."""
    validate_args(block_samples, split_penalty)
    validate_drift_args(max_step, step_cost)
    validate_smooth_args(knot_blocks, radius, bend_cost)
    _check_batch(batch)
    lo, hi = lag_arrays(batch, lag_ranges)
    call = BlockCall(batch, block_samples)
    plan = _get_plan(call.n, call.max_b, *call.lag_dims(lo, hi), int(max_step), pairs_in_flight)
    return _smooth(call, plan, (lo, hi), (float(split_penalty), int(max_step), float(step_cost), int(knot_blocks),
                                          int(radius), float(bend_cost)), raw)


def smooth_cut_sync(problems, lag_range=None, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                    split_penalty: float = DEFAULT_CUT_PENALTY, max_step: int = DEFAULT_MAX_STEP,
                    step_cost: float = DEFAULT_RANGE_STEP_COST, knot_blocks: int = DEFAULT_RANGE_KNOT_BLOCKS,
                    radius: int = DEFAULT_RANGE_RADIUS, bend_cost: float = DEFAULT_RANGE_BEND_COST,
                    sample_rate: int = SAMPLE_RATE, ratios: Optional[Sequence[float]] = None) -> List[SmoothCutSyncResult]:
    """``drift_range.cut_drift_sync`` with the smooth fit in the middle: the windowless seven-ratio solve, the range drift
    solve and the knot fit of every segment in one device call, and every cue's output time from the fitted polyline
    (``drift_smooth.map_cues_smooth``)."""
    validate_args(block_samples, split_penalty)
    validate_drift_args(max_step, step_cost)
    validate_smooth_args(knot_blocks, radius, bend_cost)
    if lag_range is not None:
        lag_range = validate_range(lag_range)
    ratios = list(candidate_ratios() if ratios is None else ratios)
    db, best, pres = solve_ratios_windowless(problems, ratios, sample_rate)
    chosen = db.select_candidates(best)
    results = smooth_align_range_batch(chosen, lag_range, block_samples, split_penalty, max_step, step_cost, knot_blocks,
                                       radius, bend_cost)
    out = []
    for p, ((_, (start_us, end_us, _meta)), res) in enumerate(zip(problems, results)):
        ratio = ratios[int(best[p])]
        cs, ce, which = map_cues_smooth(start_us, end_us, ratio, res, block_samples, sample_rate)
        rng = lag_range if lag_range is not None else full_range(chosen.lens[p, 0], chosen.lens[p, 1])
        d = res.drift
        out.append(SmoothCutSyncResult(ratio, int(best[p]), int(pres[p]["offset"]), rng, d.segments, d.total,
                                       d.block_offsets, d.block_jump, cs, ce, which, res.segments, res.smooth_offsets))
    return out
