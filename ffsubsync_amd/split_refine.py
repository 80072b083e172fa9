"""Sample-exact split breaks, and the subtitle cues that a cut removed from the video.

The split DP (``split_align``) places every break on a block boundary (10.24 s at the default K), and ``map_cues`` shifts
each cue by the piece that holds its start: a break that is off by up to a block moves the cues in between by the whole
jump.  For a stretch cut from the video, the cues of that stretch belong nowhere, yet get one neighbour's offset.

This module refines every break after the split (``csrc/ffs_split_refine.h``).  Near a break only the two
neighbouring offsets are in play, so each break gets two sample-exact cut points t1 <= t2 from exact integer counts:
subtitle samples before t1 keep the earlier piece's offset, samples in [t1, t2) match neither neighbour ("unmatched"),
and samples from t2 on take the later piece's offset.  ``unmatched_margin`` (beta) charges a little for claiming a sample
matches an offset without evidence; ``None`` gives one cut per break (t1 = t2).

Parity is against the in-repo numpy model ``tests/split_refine_model.py``, bit for bit.  ``split_align``,
``split_report`` and every existing entry point are unchanged.
"""
import math
from dataclasses import dataclass, field
from datetime import timedelta
from typing import List, Optional, Sequence

import numpy as np

from . import _native, quality, split_report
from .constants import SAMPLE_RATE
from .side_call import BlockCall, block_shape, no_workspace_split_plan, pad_rows, record_lists
from .split_align import (DEFAULT_BLOCK_SAMPLES, DEFAULT_SPLIT_PENALTY, Piece, SplitResult, _check_batch, _scaled_us,
                          _td_us, validate_block_samples)

# Chosen on the CPU model (profiles/split_refine_calibration.py; synthetic data only, 64 seeds, 2 h,
# +-10 min, K = 1024, the DP's own coarse breaks): the largest workload event is 240 s, so 270 s of radius covers a cut
# stretch that starts up to a block before or after the coarse break
DEFAULT_RADIUS_SAMPLES = 27000
DEFAULT_UNMATCHED_MARGIN = 0.25
UNMATCHED_PIECE = -2  # cue_piece of a cue whose start lies in [t1, t2) of a break


@dataclass
class RefinedBreak:
    block: int  # the DP's break block f: the coarse cut is at cut = f * K
    cut: int
    lo: int  # the search window [lo, hi] in subtitle samples
    hi: int
    t1: int  # samples [t1, t2) match neither neighbour; t1 == t2 for a single cut
    t2: int
    offset_prev: int  # the offsets of the pieces before and after the break (samples)
    offset_next: int
    coarse_score: float  # the objective's two-offset score at the coarse cut, A(cut) + B(cut)
    refined_score: float  # the objective at (t1, t2)
    flags: int  # _native.REFINE_CLIPPED / REFINE_AT_EDGE / REFINE_UNMATCHED

    @property
    def clipped(self) -> bool:
        return bool(self.flags & _native.REFINE_CLIPPED)

    @property
    def at_edge(self) -> bool:
        return bool(self.flags & _native.REFINE_AT_EDGE)


def from_record(rec) -> RefinedBreak:
    """RefinedBreak of one ``_native.BREAK_REFINE_DTYPE`` record."""
    return RefinedBreak(*(int(rec[f]) for f in ("block", "cut", "lo", "hi", "t1", "t2", "offset_prev", "offset_next")),
                        float(rec["coarse_score"]), float(rec["refined_score"]), int(rec["flags"]))


def validate_args(block_samples, radius_samples, unmatched_margin) -> None:
    """Host-side checks of the call parameters (ValueError before any native call)."""
    validate_block_samples(block_samples)
    r = int(radius_samples)
    if r != radius_samples or not 1 <= r <= _native.REFINE_MAX_RADIUS:
        raise ValueError("radius_samples=%r: need an integer in [1, %d]" % (radius_samples, _native.REFINE_MAX_RADIUS))
    if unmatched_margin is not None:
        b = float(unmatched_margin)
        if not (math.isfinite(b) and b >= 0):
            raise ValueError("unmatched_margin=%r: need a finite number >= 0, or None for a single cut" % (unmatched_margin,))


_plans = _native.SidePlanCache(_native.SplitPlan)


def _get_plan(n_pairs: int):
    """A split plan of this device that holds no split workspace: refine calls use its sub-batching and descriptors."""
    return no_workspace_split_plan(_plans, n_pairs)


def clear_plan_cache() -> None:
    _plans.clear()


def refine_breaks_batch(batch, split_results: Sequence[SplitResult], block_samples: int = DEFAULT_BLOCK_SAMPLES,
                        radius_samples: int = DEFAULT_RADIUS_SAMPLES,
                        unmatched_margin: Optional[float] = DEFAULT_UNMATCHED_MARGIN, raw: bool = False):
    """Refine the breaks of the split solves ``split_results`` (``split_align_batch`` or ``split_report_batch`` of the
    same ``batch`` and ``block_samples``): one ``RefinedBreak`` list per pair, in break order, or with ``raw``
    (``_native.BREAK_REFINE_DTYPE`` records [n_pairs, max_b], break counts)."""
    validate_args(block_samples, radius_samples, unmatched_margin)
    _check_batch(batch)
    k = int(block_samples)
    if len(split_results) != batch.n_pairs:
        raise ValueError("%d split results for %d pairs" % (len(split_results), batch.n_pairs))
    what = lambda p, size, blocks: "pair %d: %d block offsets, %d blocks of %d samples" % (p, size, blocks, k)
    path = pad_rows(block_shape(batch, k)[2], what, ([r.block_offsets for r in split_results], np.int32))
    call = BlockCall(batch, k)
    rec_out, n_out = call.records(_native.BREAK_REFINE_DTYPE), call.per_pair(np.int32)
    plan = _get_plan(call.n)
    plan.refine(*call.pair_arrays(), k, *call.upload(path), int(radius_samples),
                math.nan if unmatched_margin is None else float(unmatched_margin), rec_out, n_out)
    recs, counts = call.read_records(rec_out, _native.BREAK_REFINE_DTYPE), n_out.cpu().numpy()
    if raw:
        return recs, counts
    return record_lists(recs, counts, from_record)


def map_cues_refined(start_us, end_us, ratio: float, pieces: Sequence[Piece], breaks: Sequence[RefinedBreak],
                     sample_rate: int = SAMPLE_RATE):
    """``split_align.map_cues`` with the refined cuts: the same scaling and start-sample rounding; a cue whose start
    sample is before t1 of the next break stays with the earlier piece, a start in [t1, t2) is unmatched (piece
    ``UNMATCHED_PIECE``, times shifted by the earlier piece's offset), a start from t2 on goes to the later piece.
    ``breaks``: one per piece boundary, in order.  Returns (start_us, end_us, piece index, unmatched mask)."""
    if not pieces:
        raise ValueError("no pieces")
    if len(breaks) != len(pieces) - 1:
        raise ValueError("%d breaks for %d pieces" % (len(breaks), len(pieces)))
    t1 = np.array([b.t1 for b in breaks], dtype=np.int64)
    t2 = np.array([b.t2 for b in breaks], dtype=np.int64)
    n = len(start_us)
    out_s, out_e, which = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    unmatched = np.zeros(n, bool)
    for i in range(n):
        s_us, e_us = _scaled_us(start_us[i], ratio), _scaled_us(end_us[i], ratio)
        sample = int(round(timedelta(microseconds=s_us).total_seconds() * sample_rate))
        k = int(np.searchsorted(t2, sample, side="right"))  # breaks passed: the piece, unless inside [t1, t2) of the next
        lost = k < len(breaks) and sample >= t1[k]
        shift = timedelta(seconds=pieces[k].offset / float(sample_rate))
        out_s[i] = _td_us(timedelta(microseconds=s_us) + shift)
        out_e[i] = _td_us(timedelta(microseconds=e_us) + shift)
        which[i] = UNMATCHED_PIECE if lost else k
        unmatched[i] = lost
    return out_s, out_e, which, unmatched


@dataclass
class RefinedSplitResult(split_report.CheckedSplitResult):
    breaks: List[RefinedBreak] = field(default_factory=list)  # per break of a "split" decision; empty otherwise
    cue_unmatched: np.ndarray = field(default_factory=lambda: np.zeros(0, bool))  # cues whose start lies in [t1, t2)


def refined_split_sync(problems, max_offset_seconds: float = 600, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                       split_penalty: float = DEFAULT_SPLIT_PENALTY, radius_samples: int = DEFAULT_RADIUS_SAMPLES,
                       unmatched_margin: Optional[float] = DEFAULT_UNMATCHED_MARGIN, top_k: int = split_report.DEFAULT_TOP_K,
                       exclusion_samples: int = split_report.DEFAULT_EXCLUSION_SAMPLES,
                       min_piece_psr: float = split_report.DEFAULT_MIN_PIECE_PSR,
                       min_gain: float = split_report.DEFAULT_MIN_GAIN, min_psr: float = quality.DEFAULT_MIN_PSR,
                       min_margin: float = quality.DEFAULT_MIN_MARGIN, sample_rate: int = SAMPLE_RATE,
                       ratios: Optional[Sequence[float]] = None) -> List[RefinedSplitResult]:
    """``split_report.checked_split_sync`` with the same decisions; a "split" with more than one piece has its breaks
    refined and its cues mapped by the refined cuts (``map_cues_refined``).  "single" and "untrusted" results, and
    "split" results with one piece, are ``checked_split_sync``'s with no breaks and no unmatched cue."""
    validate_args(block_samples, radius_samples, unmatched_margin)
    checked, chosen, reps = split_report._checked_split_sync(problems, max_offset_seconds, block_samples, split_penalty,
                                                             top_k, exclusion_samples, min_piece_psr, min_gain, min_psr,
                                                             min_margin, sample_rate, ratios)
    todo = [p for p, c in enumerate(checked) if c.decision == "split" and len(c.pieces) > 1]
    refined = {}
    if todo:  # every pair in one call (pairs without breaks cost one table workgroup); only the splits' are used
        got = refine_breaks_batch(chosen, [r.split for r in reps], block_samples, radius_samples, unmatched_margin)
        refined = {p: got[p] for p in todo}
    out = []
    for p, c in enumerate(checked):
        r = RefinedSplitResult(**{f: getattr(c, f) for f in c.__dataclass_fields__})
        r.cue_unmatched = np.zeros(len(c.cue_start_us), bool)
        if p in refined:
            start_us, end_us = problems[p][1][0], problems[p][1][1]
            r.breaks = refined[p]
            r.cue_start_us, r.cue_end_us, r.cue_piece, r.cue_unmatched = map_cues_refined(start_us, end_us, c.ratio,
                                                                                          c.pieces, r.breaks, sample_rate)
        out.append(r)
    return out
