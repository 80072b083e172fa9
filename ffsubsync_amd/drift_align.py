"""Drift-tolerant alignment: the split DP with small offset steps between blocks.

``split_align`` models a file's timing error as one framerate ratio out of seven, then a piecewise-CONSTANT offset.  A
residual ratio that is none of the seven (a re-encode at 1.0004) or a clock that wandered fits neither: the offset
moves by a sample or two per block, and a change of offset costs ``split_penalty`` whether it is one sample or ten
minutes.  Here a block may also take its offset from a lag up to ``max_step`` samples away from the previous block's,
at ``step_cost`` per sample (``csrc/ffs_drift.h``); real breaks are still found, as jumps.  A ``Segment`` is a maximal
run of blocks with no jump inside, with the drift it followed.

Upstream has no equivalent, so parity is against the in-repo numpy model (``tests/drift_model.py``), bit for bit; at
``max_step`` = 0 every output equals ``split_align_batch``'s.  Nothing existing changes.
"""
import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _native
from .constants import SAMPLE_RATE, candidate_ratios
from .side_call import BlockCall, pairs_for_budget
from .split_align import (DEFAULT_BLOCK_SAMPLES, DEFAULT_SPLIT_PENALTY, _check_batch, map_cues, pieces_from_blocks,
                          solve_ratios, split_outputs, validate_args)

# Chosen on the CPU model by profiles/drift_calibration.py over workloads/drift.py (profiles/drift_calibration.json):
# the smallest power-of-two step cost at which every clean pair returns exactly the split DP's block offsets (no
# invented drift), max_step = 2 (the wobble set shows no need for more).  The calibration data are SYNTHETIC.
DEFAULT_MAX_STEP = 2
DEFAULT_STEP_COST = 128.0


@dataclass
class Segment:
    """A maximal run of blocks [first_block, end_block) with no jump inside."""

    first_block: int
    end_block: int
    start_sample: int  # subtitle samples [start_sample, end_sample)
    end_sample: int
    first_offset: int  # offset (samples) of the first and of the last block
    last_offset: int
    score: float  # sum of the blocks' scores at their offsets, in block order from 0.0
    drift: float  # (last_offset - first_offset) / samples between the two blocks: the stretch's ratio is ~ 1 + drift


@dataclass
class DriftResult:
    segments: List[Segment]
    total: float  # the DP's maximum: block scores minus step costs minus P per jump
    block_offsets: np.ndarray  # int32 [B]
    block_scores: np.ndarray  # float64 [B]
    block_jump: np.ndarray  # uint8 [B]: 1 where block b >= 1 was entered by a jump


@dataclass
class DriftSyncResult:
    ratio: float  # framerate ratio picked by the seven-ratio solve
    ratio_index: int
    global_offset: int  # that solve's single offset (samples)
    segments: List[Segment]
    total: float
    cue_start_us: np.ndarray  # output cue times (int64 microseconds): scaled, then shifted by the cue's block offset
    cue_end_us: np.ndarray
    cue_segment: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))


def validate_drift_args(max_step, step_cost) -> None:
    """Host-side checks of the two drift parameters (ValueError before any native call)."""
    try:
        s = int(max_step)
    except (TypeError, ValueError, OverflowError):
        s = None
    if s is None or s != max_step or not 0 <= s <= _native.MAX_DRIFT_STEP:
        raise ValueError("max_step=%r: need an integer in [0, %d]" % (max_step, _native.MAX_DRIFT_STEP))
    q = float(step_cost)
    if math.isnan(q) or math.isinf(q) or q < 0:
        raise ValueError("step_cost=%r: need a finite number >= 0" % (step_cost,))


def segments_from_blocks(block_offsets, block_scores, block_jump, block_samples: int, sub_len: int) -> List[Segment]:
    """Maximal runs of blocks without a jump, with their sample ranges, scores (summed in block order from 0.0) and
    drift."""
    offs, jump = np.asarray(block_offsets), np.asarray(block_jump)
    out: List[Segment] = []
    b0 = 0
    for b in range(1, offs.size + 1):
        if b == offs.size or jump[b]:
            score = 0.0
            for x in block_scores[b0:b]:
                score += float(x)
            first, last = int(offs[b0]), int(offs[b - 1])
            drift = (last - first) / float((b - 1 - b0) * block_samples) if b - 1 > b0 else 0.0
            out.append(Segment(b0, b, b0 * block_samples, min(b * block_samples, sub_len), first, last, score, drift))
            b0 = b
    return out


_plans = _native.SidePlanCache(_native.DriftPlan)


def _get_plan(n_pairs: int, max_blocks: int, max_lags: int, max_samples: int, pairs_in_flight: Optional[int]):
    """The cached drift plan of this device."""
    if pairs_in_flight is None:  # ~2.5 bytes per (block, lag): uint16 counts and a 4-bit code; bound it to ~12 GiB
        per_pair = max_blocks * (max_lags + 64) * 2.7 + 1
        pairs_in_flight = pairs_for_budget(n_pairs, per_pair)
    return _plans.get(pairs_in_flight, max_blocks, max_lags, max_samples)


def clear_plan_cache() -> None:
    _plans.clear()


def drift_align_batch(batch, max_offset_samples: int, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                      split_penalty: float = DEFAULT_SPLIT_PENALTY, max_step: int = DEFAULT_MAX_STEP,
                      step_cost: float = DEFAULT_STEP_COST, pairs_in_flight: Optional[int] = None) -> List[DriftResult]:
    """Drift-tolerant offsets of every pair of a ``batch.DeviceBatch`` with ONE candidate per pair; batch rules, lag
    window and ``split_penalty`` as ``split_align_batch``.  A block may move up to ``max_step`` (0..7) samples against
    the block before it at ``step_cost`` per sample; ``max_step`` = 0 is ``split_align_batch``.  Returns one
    ``DriftResult`` per pair."""
    validate_args(block_samples, max_offset_samples, split_penalty)
    validate_drift_args(max_step, step_cost)
    _check_batch(batch)
    call = BlockCall(batch, block_samples)
    w = int(max_offset_samples)
    plan = _get_plan(call.n, call.max_b, 2 * w, int(call.sub_len.max()), pairs_in_flight)
    offs, scores, jumps, totals = drift_outputs(call)
    plan.align(*call.pair_arrays(), call.k, w, float(split_penalty), int(max_step), float(step_cost), offs, scores, jumps,
               totals)
    return drift_results(offs, scores, jumps, totals, call.n_blocks, call.k, call.sub_len)


def drift_outputs(call: BlockCall):
    """The device outputs of a drift call: ``split_outputs``' block offsets and scores, jump flags (n * max_b each)
    and totals (n), in the order the drift plans take them."""
    offs, scores, totals = split_outputs(call.n, call.max_b, call.dev)
    return offs, scores, call.per_block(np.uint8), totals


def drift_results(offs, scores, jumps, totals, n_blocks, block_samples: int, sub_len) -> List[DriftResult]:
    """One ``DriftResult`` per pair from the device outputs of a drift call (n_pairs * max_b block offsets, scores and
    jump flags, n_pairs totals) after the call."""
    n, max_b = len(n_blocks), int(max(n_blocks))
    offs_h = offs.cpu().numpy().reshape(n, max_b)
    scores_h = scores.cpu().numpy().reshape(n, max_b)
    jumps_h = jumps.cpu().numpy().reshape(n, max_b)
    totals_h = totals.cpu().numpy()
    out = []
    for p in range(n):
        nb = int(n_blocks[p])
        bo, bs, bj = offs_h[p, :nb].copy(), scores_h[p, :nb].copy(), jumps_h[p, :nb].copy()
        out.append(DriftResult(segments_from_blocks(bo, bs, bj, block_samples, int(sub_len[p])), float(totals_h[p]), bo, bs, bj))
    return out


def map_cues_drift(start_us, end_us, ratio: float, result: DriftResult, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                   sample_rate: int = SAMPLE_RATE):
    """Output times of every cue: scaled by ``ratio``, then shifted by the offset of the BLOCK that holds its scaled
    start sample.  That is exactly ``split_align.map_cues`` over the maximal runs of equal block offsets
    (``pieces_from_blocks``), so that is what runs; a jump always changes the offset, so every such run lies inside one
    segment.  Returns (start_us, end_us, segment index) int64 arrays."""
    sub_len = result.segments[-1].end_sample
    pieces = pieces_from_blocks(result.block_offsets, result.block_scores, block_samples, sub_len)
    out_s, out_e, which = map_cues(start_us, end_us, ratio, pieces, sample_rate)
    seg_first = np.array([s.first_block for s in result.segments], dtype=np.int64)
    piece_seg = np.searchsorted(seg_first, np.array([p.first_block for p in pieces], dtype=np.int64), side="right") - 1
    return out_s, out_e, piece_seg[which].astype(np.int64)


def drift_sync(problems, max_offset_seconds: float = 600, block_samples: int = DEFAULT_BLOCK_SAMPLES,
               split_penalty: float = DEFAULT_SPLIT_PENALTY, max_step: int = DEFAULT_MAX_STEP,
               step_cost: float = DEFAULT_STEP_COST, sample_rate: int = SAMPLE_RATE,
               ratios: Optional[Sequence[float]] = None) -> List[DriftSyncResult]:
    """``split_align.split_sync`` with the drift DP in the middle: per (reference, track) problem the framerate ratio
    from the seven-ratio batch solve over the same lag window, the winner rasterised on the device, the drift DP, and
    every cue's output time."""
    w = int(round(max_offset_seconds * sample_rate))
    validate_args(block_samples, w, split_penalty)
    validate_drift_args(max_step, step_cost)
    ratios = list(candidate_ratios() if ratios is None else ratios)
    db, best, pres = solve_ratios(problems, w, ratios, sample_rate)
    results = drift_align_batch(db.select_candidates(best), w, block_samples, split_penalty, max_step, step_cost)
    out = []
    for p, ((_, (start_us, end_us, _meta)), res) in enumerate(zip(problems, results)):
        ratio = ratios[int(best[p])]
        cs, ce, which = map_cues_drift(start_us, end_us, ratio, res, block_samples, sample_rate)
        out.append(DriftSyncResult(ratio, int(best[p]), int(pres[p]["offset"]), res.segments, res.total, cs, ce, which))
    return out
