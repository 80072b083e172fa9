"""Sample-exact jumps of a drift solve, and the subtitle cues that a cut removed from the video.

The drift DPs (``drift_align``, ``drift_range``) place every jump on a block boundary (10.24 s at the default K), and
``map_cues_drift`` / ``map_cues_smooth`` give each cue the segment of the block that holds its start: a jump that is off
by up to a block moves the cues in between by the whole jump -- 20 to 30 minutes for another cut of a film -- and the
cues of a scene the video does not have get a neighbour's offset.  ``split_refine`` cures both for a piecewise-constant
path; it treats every change of offset as a break, and a drift path changes offset at almost every block.

This module refines the JUMPS of a drift path (``csrc/ffs_drift_refine.h``).  Near a jump only the two
neighbouring segments are in play, each scored along its own per-block lags (held at its end block's lag past the
coarse cut), so each jump gets two sample-exact cut points t1 <= t2 from exact integer counts, exactly as
``split_refine`` defines them: samples before t1 stay with the earlier segment, samples in [t1, t2) match neither
("unmatched"), samples from t2 on go to the later segment.  The call takes no lag window, so it serves ``drift_sync`` /
``smooth_sync`` and ``cut_drift_sync`` / ``smooth_cut_sync`` alike.

Parity is against the in-repo numpy model ``tests/drift_refine_model.py``, bit for bit; on a piecewise-constant path the
records equal ``split_refine.refine_breaks_batch``'s byte for byte.  Every existing entry point is unchanged.
"""
import math
from dataclasses import dataclass, field
from datetime import timedelta
from typing import List, Optional, Sequence

import numpy as np

from . import _native
from .constants import SAMPLE_RATE, candidate_ratios
from .cut_align import DEFAULT_CUT_PENALTY, full_range, solve_ratios_windowless, validate_range
from .cut_align import validate_args as validate_cut_args
from .drift_align import (DEFAULT_MAX_STEP, DEFAULT_STEP_COST, DriftResult, DriftSyncResult, drift_align_batch,
                          map_cues_drift, validate_drift_args)
from .drift_range import DEFAULT_RANGE_STEP_COST, CutDriftSyncResult, drift_align_range_batch
from .drift_range_smooth import (DEFAULT_RANGE_BEND_COST, DEFAULT_RANGE_KNOT_BLOCKS, DEFAULT_RANGE_RADIUS,
                                 SmoothCutSyncResult, smooth_align_range_batch)
from .drift_smooth import (DEFAULT_BEND_COST, DEFAULT_KNOT_BLOCKS, DEFAULT_RADIUS, SmoothResult, SmoothSyncResult,
                           map_cues_smooth, polyline_shift, smooth_align_batch, validate_smooth_args)
from .side_call import BlockCall, block_shape, no_workspace_split_plan, pad_rows, record_lists
from .split_align import (DEFAULT_BLOCK_SAMPLES, DEFAULT_SPLIT_PENALTY, _check_batch, _scaled_us, _td_us, solve_ratios,
                          validate_args)
from .split_refine import (DEFAULT_RADIUS_SAMPLES, DEFAULT_UNMATCHED_MARGIN, UNMATCHED_PIECE, RefinedBreak, from_record,
                           validate_args as validate_refine_args)

# split_refine's defaults (27 000 samples, 0.25), kept: profiles/drift_refine_calibration.py ran the CPU models over
# workloads/drift_cuts.py (profiles/drift_refine_calibration.json) and the table gives no reason to move
# them.  The calibration data are SYNTHETIC.

_plans = _native.SidePlanCache(_native.SplitPlan)


def _get_plan(n_pairs: int):
    """A split plan of this device that holds no split workspace, as ``split_refine``'s."""
    return no_workspace_split_plan(_plans, n_pairs)


def clear_plan_cache() -> None:
    _plans.clear()


def _path(result):
    """(DriftResult, the block offsets to refine along) of a DriftResult or a SmoothResult."""
    if isinstance(result, SmoothResult):
        return result.drift, result.smooth_offsets
    return result, result.block_offsets


def refine_jumps_batch(batch, results: Sequence, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                       radius_samples: int = DEFAULT_RADIUS_SAMPLES,
                       unmatched_margin: Optional[float] = DEFAULT_UNMATCHED_MARGIN, raw: bool = False):
    """Refine the jumps of the drift solves ``results`` (``DriftResult``s of ``drift_align_batch`` /
    ``drift_align_range_batch``, or ``SmoothResult``s of ``smooth_align_batch`` / ``smooth_align_range_batch``, of the
    same ``batch`` and ``block_samples``).  A ``SmoothResult`` refines along its ``smooth_offsets`` with the jumps of its
    ``.drift``.  Returns one ``split_refine.RefinedBreak`` list per pair, one entry per jump in order, or with ``raw``
    (``_native.BREAK_REFINE_DTYPE`` records [n_pairs, max_b], jump counts)."""
    validate_refine_args(block_samples, radius_samples, unmatched_margin)
    _check_batch(batch)
    k = int(block_samples)
    if len(results) != batch.n_pairs:
        raise ValueError("%d drift results for %d pairs" % (len(results), batch.n_pairs))
    paths = [_path(r) for r in results]
    all_offs, all_jumps = [np.asarray(o) for _, o in paths], [np.asarray(d.block_jump) != 0 for d, _ in paths]
    what = lambda p, _size, blocks: ("pair %d: %d block offsets and %d jump flags, %d blocks of %d samples"
                                     % (p, all_offs[p].size, all_jumps[p].size, blocks, k))
    path = pad_rows(block_shape(batch, k)[2], what, (all_offs, np.int32), (all_jumps, np.uint8))
    call = BlockCall(batch, k)
    rec_out, n_out = call.records(_native.BREAK_REFINE_DTYPE), call.per_pair(np.int32)
    plan = _get_plan(call.n)
    plan.drift_refine(*call.pair_arrays(), k, *call.upload(path), int(radius_samples),
                      math.nan if unmatched_margin is None else float(unmatched_margin), rec_out, n_out)
    recs, counts = call.read_records(rec_out, _native.BREAK_REFINE_DTYPE), n_out.cpu().numpy()
    if raw:
        return recs, counts
    return record_lists(recs, counts, from_record)


def _refined_cues(start_us, end_us, ratio, segments, breaks, sample_rate, shift_us):
    """The cue loop of both refined mappings: ``shift_us(k, sample, s_us)`` gives segment k's output start time."""
    if not segments:
        raise ValueError("no segments")
    if len(breaks) != len(segments) - 1:
        raise ValueError("%d refined jumps for %d segments" % (len(breaks), len(segments)))
    t1 = np.array([b.t1 for b in breaks], dtype=np.int64)
    t2 = np.array([b.t2 for b in breaks], dtype=np.int64)
    n = len(start_us)
    out_s, out_e, which = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    unmatched = np.zeros(n, bool)
    for i in range(n):
        s_us, e_us = _scaled_us(start_us[i], ratio), _scaled_us(end_us[i], ratio)
        sample = int(round(timedelta(microseconds=s_us).total_seconds() * sample_rate))
        k = int(np.searchsorted(t2, sample, side="right"))  # jumps passed: the segment, unless inside [t1, t2) of the next
        lost = k < len(breaks) and sample >= t1[k]
        out_s[i] = shift_us(k, sample, s_us)
        out_e[i] = e_us + (out_s[i] - s_us)
        which[i] = UNMATCHED_PIECE if lost else k
        unmatched[i] = lost
    return out_s, out_e, which, unmatched


def map_cues_drift_refined(start_us, end_us, ratio: float, result: DriftResult, breaks: Sequence[RefinedBreak],
                           block_samples: int = DEFAULT_BLOCK_SAMPLES, sample_rate: int = SAMPLE_RATE):
    """``drift_align.map_cues_drift`` with the refined cuts: the same scaling and start-sample rounding.  With x the
    scaled start sample and k the number of jumps with t2 <= x, the cue belongs to segment k and is unmatched when
    x >= t1 of jump k (segment ``UNMATCHED_PIECE``, times shifted as the earlier segment's).  Its shift is the offset of
    block clamp(x // K, first_block_k, end_block_k - 1): the lag the kernel scored that sample at.  ``breaks``: one per
    jump of ``result``, in order.  Returns (start_us, end_us, segment index, unmatched mask)."""
    segs, o, k_ = result.segments, np.asarray(result.block_offsets), int(block_samples)

    def shift_us(k, sample, s_us):
        b = min(max(sample // k_, segs[k].first_block), segs[k].end_block - 1)
        return _td_us(timedelta(microseconds=s_us) + timedelta(seconds=int(o[b]) / float(sample_rate)))

    return _refined_cues(start_us, end_us, ratio, segs, breaks, sample_rate, shift_us)


def map_cues_smooth_refined(start_us, end_us, ratio: float, result: SmoothResult, breaks: Sequence[RefinedBreak],
                            block_samples: int = DEFAULT_BLOCK_SAMPLES, sample_rate: int = SAMPLE_RATE):
    """``drift_smooth.map_cues_smooth`` with the refined cuts: segment and unmatched cues as
    ``map_cues_drift_refined``; the shift is the segment's polyline at the start sample (``polyline_shift``), which
    continues with its end slope past the segment's blocks -- a few samples from the held lag the kernel scored there."""
    segs, k_ = result.segments, int(block_samples)

    def shift_us(k, sample, s_us):
        return s_us + int(round(polyline_shift(segs[k], float(sample), k_) * 1e6 / sample_rate))

    return _refined_cues(start_us, end_us, ratio, segs, breaks, sample_rate, shift_us)


@dataclass
class RefinedDriftSyncResult(DriftSyncResult):
    breaks: List[RefinedBreak] = field(default_factory=list)  # one per jump; empty for a file of one segment
    cue_unmatched: np.ndarray = field(default_factory=lambda: np.zeros(0, bool))  # cues whose start lies in [t1, t2)


@dataclass
class RefinedSmoothSyncResult(SmoothSyncResult):
    breaks: List[RefinedBreak] = field(default_factory=list)
    cue_unmatched: np.ndarray = field(default_factory=lambda: np.zeros(0, bool))


@dataclass
class RefinedCutDriftSyncResult(CutDriftSyncResult):
    breaks: List[RefinedBreak] = field(default_factory=list)
    cue_unmatched: np.ndarray = field(default_factory=lambda: np.zeros(0, bool))


@dataclass
class RefinedSmoothCutSyncResult(SmoothCutSyncResult):
    breaks: List[RefinedBreak] = field(default_factory=list)
    cue_unmatched: np.ndarray = field(default_factory=lambda: np.zeros(0, bool))


def _refined_mappings(problems, chosen, results, ratios, best, block_samples, radius_samples, unmatched_margin,
                      sample_rate):
    """Per problem (start_us, end_us, segment, unmatched, breaks): the unrefined mapping for a file of one segment, the
    refined one otherwise."""
    multi = any(len(_path(r)[0].segments) > 1 for r in results)
    refined = refine_jumps_batch(chosen, results, block_samples, radius_samples, unmatched_margin) if multi else None
    out = []
    for p, ((_, (start_us, end_us, _meta)), res) in enumerate(zip(problems, results)):
        ratio = ratios[int(best[p])]
        smooth = isinstance(res, SmoothResult)
        if len(_path(res)[0].segments) == 1:
            cs, ce, which = (map_cues_smooth if smooth else map_cues_drift)(start_us, end_us, ratio, res, block_samples,
                                                                            sample_rate)
            out.append((cs, ce, which, np.zeros(len(cs), bool), []))
        else:
            mapper = map_cues_smooth_refined if smooth else map_cues_drift_refined
            out.append(mapper(start_us, end_us, ratio, res, refined[p], block_samples, sample_rate) + (refined[p],))
    return out


def refined_drift_sync(problems, max_offset_seconds: float = 600, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                       split_penalty: float = DEFAULT_SPLIT_PENALTY, max_step: int = DEFAULT_MAX_STEP,
                       step_cost: float = DEFAULT_STEP_COST, knot_blocks: int = DEFAULT_KNOT_BLOCKS,
                       radius: int = DEFAULT_RADIUS, bend_cost: float = DEFAULT_BEND_COST,
                       radius_samples: int = DEFAULT_RADIUS_SAMPLES,
                       unmatched_margin: Optional[float] = DEFAULT_UNMATCHED_MARGIN, sample_rate: int = SAMPLE_RATE,
                       ratios: Optional[Sequence[float]] = None, smooth: bool = True):
    """``drift_smooth.smooth_sync`` (``smooth`` False: ``drift_align.drift_sync``) with every jump refined and the cues
    mapped by the refined cuts.  A file of one segment returns exactly the unrefined entry point's fields, no breaks and
    no unmatched cue.  Returns ``RefinedSmoothSyncResult``s (``RefinedDriftSyncResult``s)."""
    w = int(round(max_offset_seconds * sample_rate))
    validate_args(block_samples, w, split_penalty)
    validate_drift_args(max_step, step_cost)
    if smooth:
        validate_smooth_args(knot_blocks, radius, bend_cost)
    validate_refine_args(block_samples, radius_samples, unmatched_margin)
    ratios = list(candidate_ratios() if ratios is None else ratios)
    db, best, pres = solve_ratios(problems, w, ratios, sample_rate)
    chosen = db.select_candidates(best)
    if smooth:
        results = smooth_align_batch(chosen, w, block_samples, split_penalty, max_step, step_cost, knot_blocks, radius,
                                     bend_cost)
    else:
        results = drift_align_batch(chosen, w, block_samples, split_penalty, max_step, step_cost)
    mapped = _refined_mappings(problems, chosen, results, ratios, best, block_samples, radius_samples, unmatched_margin,
                               sample_rate)
    out = []
    for p, (res, (cs, ce, which, um, breaks)) in enumerate(zip(results, mapped)):
        d = _path(res)[0]
        head = (ratios[int(best[p])], int(best[p]), int(pres[p]["offset"]), d.segments, d.total, cs, ce, which)
        if smooth:
            out.append(RefinedSmoothSyncResult(*head, res.segments, breaks, um))
        else:
            out.append(RefinedDriftSyncResult(*head, breaks, um))
    return out


def refined_cut_drift_sync(problems, lag_range=None, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                           split_penalty: float = DEFAULT_CUT_PENALTY, max_step: int = DEFAULT_MAX_STEP,
                           step_cost: float = DEFAULT_RANGE_STEP_COST, knot_blocks: int = DEFAULT_RANGE_KNOT_BLOCKS,
                           radius: int = DEFAULT_RANGE_RADIUS, bend_cost: float = DEFAULT_RANGE_BEND_COST,
                           radius_samples: int = DEFAULT_RADIUS_SAMPLES,
                           unmatched_margin: Optional[float] = DEFAULT_UNMATCHED_MARGIN, sample_rate: int = SAMPLE_RATE,
                           ratios: Optional[Sequence[float]] = None, smooth: bool = True):
    """``drift_range_smooth.smooth_cut_sync`` (``smooth`` False: ``drift_range.cut_drift_sync``) with every jump refined
    and the cues mapped by the refined cuts.  A file of one segment returns exactly the unrefined entry point's fields,
    no breaks and no unmatched cue.  Returns ``RefinedSmoothCutSyncResult``s (``RefinedCutDriftSyncResult``s)."""
    validate_cut_args(block_samples, split_penalty)
    validate_drift_args(max_step, step_cost)
    if smooth:
        validate_smooth_args(knot_blocks, radius, bend_cost)
    validate_refine_args(block_samples, radius_samples, unmatched_margin)
    if lag_range is not None:
        lag_range = validate_range(lag_range)
    ratios = list(candidate_ratios() if ratios is None else ratios)
    db, best, pres = solve_ratios_windowless(problems, ratios, sample_rate)
    chosen = db.select_candidates(best)
    if smooth:
        results = smooth_align_range_batch(chosen, lag_range, block_samples, split_penalty, max_step, step_cost,
                                           knot_blocks, radius, bend_cost)
    else:
        results = drift_align_range_batch(chosen, lag_range, block_samples, split_penalty, max_step, step_cost)
    mapped = _refined_mappings(problems, chosen, results, ratios, best, block_samples, radius_samples, unmatched_margin,
                               sample_rate)
    out = []
    for p, (res, (cs, ce, which, um, breaks)) in enumerate(zip(results, mapped)):
        d = _path(res)[0]
        rng = lag_range if lag_range is not None else full_range(chosen.lens[p, 0], chosen.lens[p, 1])
        head = (ratios[int(best[p])], int(best[p]), int(pres[p]["offset"]), rng, d.segments, d.total, d.block_offsets,
                d.block_jump, cs, ce, which)
        if smooth:
            out.append(RefinedSmoothCutSyncResult(*head, res.segments, res.smooth_offsets, breaks, um))
        else:
            out.append(RefinedCutDriftSyncResult(*head, breaks, um))
    return out
