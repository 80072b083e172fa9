"""Drift-tolerant alignment over any lag range: subtitles made for another cut of the video AND re-encoded.

``cut_align`` follows offsets of tens of minutes, but its DP knows only STAY and JUMP: a residual framerate ratio of a
few 1e-4 on top of another cut moves the offset by a sample or two per block, and the range split follows that ramp
with one constant per piece.  ``drift_align`` follows the ramp, inside +-131 072 samples.  Here ``drift_align``'s DP
(steps of up to ``max_step`` samples between blocks at ``step_cost`` per sample, jumps at ``split_penalty``) runs over
``cut_align``'s lag set: a per-pair range [lag_lo, lag_hi], up to the full overlap range, on
``csrc/ffs_drift_range.h`` -- one launch per block step, the lag row spread over many workgroups.

``cut_drift_sync`` chains the seven-ratio solve with no window, the range drift solve and the per-cue output at block
granularity; ``drift_range_smooth.smooth_cut_sync`` adds the polyline fit over a range,
``drift_refine.refined_cut_drift_sync`` sample-exact jumps and unmatched cues (3.16) and
``drift_range_report.checked_cut_drift_sync`` the segment report over a range and a decision per file (3.17).

Parity is against the in-repo numpy model ``tests/drift_range_model.py``, bit for bit; at ``max_step`` = 0 offsets,
scores and total equal ``split_align_range_batch``'s, at [-W+1, W] every output equals ``drift_align_batch``'s.
Every existing entry point is unchanged.
"""
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from .constants import SAMPLE_RATE, candidate_ratios
from .cut_align import (DEFAULT_CUT_PENALTY, full_range, lag_arrays, solve_ratios_windowless, validate_args,
                        validate_range)
from .drift_align import (DEFAULT_MAX_STEP, DriftResult, Segment, drift_outputs, drift_results, map_cues_drift,
                          validate_drift_args)
from .side_call import BlockCall, pairs_for_budget
from .split_align import DEFAULT_BLOCK_SAMPLES, _check_batch

# Chosen on the CPU model over the full range by profiles/drift_range_calibration.py over workloads/cut_drift.py
# (profiles/drift_range_calibration.json): the smallest power-of-two step cost at which every clean
# problem returns exactly the range split's block offsets, at max_step = 2.  The calibration data are SYNTHETIC.
DEFAULT_RANGE_STEP_COST = 64.0


@dataclass
class CutDriftSyncResult:
    ratio: float  # framerate ratio picked by the windowless seven-ratio solve
    ratio_index: int
    global_offset: int  # that solve's single offset (samples)
    lag_range: Tuple[int, int]  # the drift solve's lag range
    segments: List[Segment]
    total: float
    block_offsets: np.ndarray  # int32 [B]
    block_jump: np.ndarray  # uint8 [B]
    cue_start_us: np.ndarray  # output cue times (int64 microseconds): scaled, then shifted by the cue's block offset
    cue_end_us: np.ndarray
    cue_segment: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))


_plans = _native.SidePlanCache(_native.DriftRangePlan)


def code_planes(max_step: int) -> int:
    """Bit planes that hold the codes 0 .. 2 * max_step + 1 (``drift_range_planes`` of csrc/ffs_drift_range.h)."""
    return (2 * int(max_step) + 1).bit_length()


def workspace_per_pair(max_blocks: int, max_lags: int, max_samples: int, max_step: int) -> float:
    """Bytes of range drift workspace per pair in flight: code planes and two fp64 rows, ~400 MB for a 2 h full-range
    pair at max_step 2.  The smooth fit and the report add their own on top."""
    return max_blocks * (code_planes(max_step) * max_lags / 8.0 + 8) + max_lags * 16.0 + max_samples / 4.0 + 4096


def _get_plan(n_pairs: int, max_blocks: int, max_lags: int, max_samples: int, max_step: int,
              pairs_in_flight: Optional[int]):
    if pairs_in_flight is None:  # bound the workspace to ~12 GiB
        pairs_in_flight = pairs_for_budget(n_pairs, workspace_per_pair(max_blocks, max_lags, max_samples, max_step))
    return _plans.get(pairs_in_flight, max_blocks, max_lags, max_samples, max_step)


def clear_plan_cache() -> None:
    _plans.clear()


def drift_align_range_batch(batch, lag_ranges=None, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                            split_penalty: float = DEFAULT_CUT_PENALTY, max_step: int = DEFAULT_MAX_STEP,
                            step_cost: float = DEFAULT_RANGE_STEP_COST,
                            pairs_in_flight: Optional[int] = None) -> List[DriftResult]:
    """Drift-tolerant offsets of every pair of a ``batch.DeviceBatch`` with ONE candidate per pair, as
    ``drift_align.drift_align_batch``, over lags d in [lag_lo, lag_hi]: ``lag_ranges`` is one (lag_lo, lag_hi) for every
    pair, a list of one per pair, or None for each pair's full overlap range [-(S-1), R-1].  ``max_step`` = 0 is
    ``cut_align.split_align_range_batch``."""
    validate_args(block_samples, split_penalty)
    validate_drift_args(max_step, step_cost)
    _check_batch(batch)
    lo, hi = lag_arrays(batch, lag_ranges)
    call = BlockCall(batch, block_samples)
    plan = _get_plan(call.n, call.max_b, *call.lag_dims(lo, hi), int(max_step), pairs_in_flight)
    outs = drift_outputs(call)
    plan.align(*call.pair_arrays(), call.k, lo, hi, float(split_penalty), int(max_step), float(step_cost), *outs)
    return drift_results(*outs, call.n_blocks, call.k, call.sub_len)


def cut_drift_sync(problems, lag_range=None, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                   split_penalty: float = DEFAULT_CUT_PENALTY, max_step: int = DEFAULT_MAX_STEP,
                   step_cost: float = DEFAULT_RANGE_STEP_COST, sample_rate: int = SAMPLE_RATE,
                   ratios: Optional[Sequence[float]] = None) -> List[CutDriftSyncResult]:
    """Sync of subtitles made for another cut of the video whose timing also drifts.  ``problems``: list of (reference,
    track) as ``cut_align.cut_sync`` takes them.  Per problem: the framerate ratio from the windowless seven-ratio solve,
    the drift solve over ``lag_range`` (one (lag_lo, lag_hi) for every problem; None = each pair's full overlap range)
    and every cue's output time, shifted by the offset of the block that holds it."""
    validate_args(block_samples, split_penalty)
    validate_drift_args(max_step, step_cost)
    if lag_range is not None:
        lag_range = validate_range(lag_range)
    ratios = list(candidate_ratios() if ratios is None else ratios)
    db, best, pres = solve_ratios_windowless(problems, ratios, sample_rate)
    chosen = db.select_candidates(best)
    results = drift_align_range_batch(chosen, lag_range, block_samples, split_penalty, max_step, step_cost)
    out = []
    for p, ((_, (start_us, end_us, _meta)), res) in enumerate(zip(problems, results)):
        ratio = ratios[int(best[p])]
        cs, ce, which = map_cues_drift(start_us, end_us, ratio, res, block_samples, sample_rate)
        rng = lag_range if lag_range is not None else full_range(chosen.lens[p, 0], chosen.lens[p, 1])
        out.append(CutDriftSyncResult(ratio, int(best[p]), int(pres[p]["offset"]), rng, res.segments, res.total,
                                      res.block_offsets, res.block_jump, cs, ce, which))
    return out
