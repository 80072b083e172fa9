"""Split-aware alignment over any lag range: subtitles made for another cut of the same film or episode.

``split_align`` works inside a lag window symmetric around zero, at most 2W <= 262 144 lags (+-21.8 min at 100 Hz).  A
subtitle for the theatrical cut on the extended video (or the other way round) needs more: the offset is the total
length of the scenes one version adds up to that point, 10 to 50 minutes by the end of a film.  Here the split DP runs
over a per-pair lag range [lag_lo, lag_hi], up to the full overlap range [-(S-1), R-1], on ``csrc/ffs_split_range.h``:
one pair's lag row is spread over many workgroups, one launch per block step, block counts computed inside the step.

``cut_sync`` chains the seven-ratio solve with no window, the range split, ``split_refine``'s sample-exact breaks and
the per-cue output; cues of scenes the video does not have come out unmatched (piece -2).

Parity is against the in-repo numpy model ``tests/cut_model.py``, bit for bit; at [-W+1, W] the records equal
``split_align_batch``'s.  Every existing entry point is unchanged.
"""
import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native, split_refine
from .constants import SAMPLE_RATE, candidate_ratios
from .side_call import BlockCall, pairs_for_budget
from .split_align import (DEFAULT_BLOCK_SAMPLES, Piece, SplitResult, _check_batch, empty_error, split_outputs,
                          split_results, validate_block_samples)

# Chosen on the CPU model over the full range (profiles/cut_calibration.py; synthetic data only)
DEFAULT_CUT_PENALTY = 8192.0
MAX_RANGE_LAGS = 2 ** 31 - 1
INT32_MAX = 2 ** 31 - 1


@dataclass
class CutSyncResult:
    ratio: float  # framerate ratio picked by the windowless seven-ratio solve
    ratio_index: int
    global_offset: int  # that solve's single offset (samples)
    lag_range: Tuple[int, int]  # the split's lag range
    pieces: List[Piece]
    total: float
    breaks: List[split_refine.RefinedBreak]  # one per piece boundary
    cue_start_us: np.ndarray  # output cue times (int64 microseconds)
    cue_end_us: np.ndarray
    cue_piece: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))  # -2: unmatched
    cue_unmatched: np.ndarray = field(default_factory=lambda: np.zeros(0, bool))


def validate_args(block_samples, split_penalty) -> None:
    """Host-side checks of the call parameters (ValueError before any native call)."""
    validate_block_samples(block_samples)
    p = float(split_penalty)
    if math.isnan(p) or p < 0:
        raise ValueError("split_penalty=%r: need a number >= 0 (inf = never split)" % (split_penalty,))


def validate_range(lag_range) -> Tuple[int, int]:
    """(lag_lo, lag_hi) as ints: lag_lo <= lag_hi, both inside the int32 range, at most 2^31 - 1 lags."""
    try:
        lo, hi = lag_range
    except (TypeError, ValueError):
        raise ValueError("lag range %r: need a (lag_lo, lag_hi) pair" % (lag_range,))
    if int(lo) != lo or int(hi) != hi:
        raise ValueError("lag range %r: need integers" % (lag_range,))
    lo, hi = int(lo), int(hi)
    if lo > hi or lo < -INT32_MAX or hi > INT32_MAX or hi - lo + 1 > MAX_RANGE_LAGS:
        raise ValueError("lag range [%d, %d]: need -(2^31 - 1) <= lag_lo <= lag_hi <= 2^31 - 1 and at most 2^31 - 1 lags"
                         % (lo, hi))
    return lo, hi


def full_range(ref_len: int, sub_len: int) -> Tuple[int, int]:
    """[-(S-1), R-1]: every lag at which the subtitle vector overlaps the reference."""
    return -(int(sub_len) - 1), int(ref_len) - 1


_plans = _native.SidePlanCache(_native.SplitRangePlan)


def workspace_per_pair(max_blocks: int, max_lags: int, max_samples: int) -> float:
    """Bytes of range split workspace per pair in flight: stay bits and one fp64 row, ~140 MB for a 2 h full-range pair."""
    return max_blocks * (max_lags / 8.0 + 8) + max_lags * 8.0 + max_samples / 4.0 + 4096


def _get_plan(n_pairs: int, max_blocks: int, max_lags: int, max_samples: int, pairs_in_flight: Optional[int]):
    if pairs_in_flight is None:  # bound the workspace to ~12 GiB
        pairs_in_flight = pairs_for_budget(n_pairs, workspace_per_pair(max_blocks, max_lags, max_samples))
    return _plans.get(pairs_in_flight, max_blocks, max_lags, max_samples)


def clear_plan_cache() -> None:
    _plans.clear()


def lag_arrays(batch, lag_ranges) -> Tuple[np.ndarray, np.ndarray]:
    """(lag_lo, lag_hi) int64 arrays of one pair each: ``lag_ranges`` one (lag_lo, lag_hi) for every pair, a list of one
    per pair, or None for each pair's full overlap range [-(S-1), R-1] (ValueError for a bad range)."""
    n = batch.n_pairs
    ref_len, sub_len = batch.lens[:, 0].astype(np.int64), batch.lens[:, 1].astype(np.int64)
    if lag_ranges is None:
        ranges = [full_range(ref_len[p], sub_len[p]) for p in range(n)]
    elif len(lag_ranges) == 2 and all(np.ndim(x) == 0 for x in lag_ranges):
        ranges = [validate_range(lag_ranges)] * n
    else:
        if len(lag_ranges) != n:
            raise ValueError("%d lag ranges for %d pairs" % (len(lag_ranges), n))
        ranges = [validate_range(r) for r in lag_ranges]
    ranges = [validate_range(r) for r in ranges]
    return np.array([r[0] for r in ranges], np.int64), np.array([r[1] for r in ranges], np.int64)


def split_align_range_batch(batch, lag_ranges=None, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                            split_penalty: float = DEFAULT_CUT_PENALTY,
                            pairs_in_flight: Optional[int] = None) -> List[SplitResult]:
    """Piecewise offsets of every pair of a ``batch.DeviceBatch`` with ONE candidate per pair, as
    ``split_align.split_align_batch``, over lags d in [lag_lo, lag_hi]: ``lag_ranges`` is one (lag_lo, lag_hi) for
    every pair, a list of one per pair, or None for each pair's full overlap range [-(S-1), R-1]."""
    validate_args(block_samples, split_penalty)
    _check_batch(batch)
    lo, hi = lag_arrays(batch, lag_ranges)
    call = BlockCall(batch, block_samples)
    plan = _get_plan(call.n, call.max_b, *call.lag_dims(lo, hi), pairs_in_flight)
    outs = split_outputs(call.n, call.max_b, call.dev)
    plan.align(*call.pair_arrays(), call.k, lo, hi, float(split_penalty), *outs)
    return split_results(outs, call.n_blocks, call.k, call.sub_len)


def _device_refs(problems):
    """The references of (reference, track) problems as ``DeviceRaster``s, with the host checks of ``split_sync``."""
    from .subtitle_raster import DeviceRaster

    refs = []
    for ref, track in problems:
        if len(track[0]) == 0:
            raise empty_error(len(ref), 0)
        if not isinstance(ref, DeviceRaster):
            host = np.asarray(ref, dtype=np.float64).ravel()
            if host.size == 0:
                raise empty_error(0, 1)
            if np.unique(host).size > 2 or not np.all(np.isfinite(host)):
                raise ValueError("the reference must be a two-level vector")
            _native.require_gpu()
            ref = DeviceRaster.from_host(host, lists=False)
        elif ref.n == 0:
            raise empty_error(0, 1)
        refs.append(ref)
    return refs


def solve_ratios_windowless(problems, ratios: Sequence[float], sample_rate: int = SAMPLE_RATE):
    """``split_align.solve_ratios`` with no lag window: every track rasterised on the device at each ratio, one
    ``BatchAligner(max_offset_samples=None)`` solve over every lag with an overlap.  Returns (DeviceBatch, winning
    candidate index per problem, the solve's ffs_pair_result records)."""
    from . import batch as batch_mod
    from .subtitle_raster import rasterize_candidates

    refs = _device_refs(problems)
    pairs = []
    for ref, (start_us, end_us, meta) in zip(refs, (p[1] for p in problems)):
        pairs.append((ref, rasterize_candidates(start_us, end_us, meta, ratios, sample_rate)))
    db = batch_mod.pack_pairs(pairs)
    al = batch_mod.BatchAligner(db.required_fft_length(None), len(ratios), None, pairs_in_flight=min(len(pairs), 64))
    try:
        _, pres = al.solve(db)
    finally:
        al.close()
    best = pres["best_cand"].astype(np.int64)
    if (best < 0).any():
        raise RuntimeError("no framerate ratio found an offset")
    return db, best, pres


def cut_sync(problems, lag_range=None, block_samples: int = DEFAULT_BLOCK_SAMPLES,
             split_penalty: float = DEFAULT_CUT_PENALTY, radius_samples: int = split_refine.DEFAULT_RADIUS_SAMPLES,
             unmatched_margin: Optional[float] = split_refine.DEFAULT_UNMATCHED_MARGIN, sample_rate: int = SAMPLE_RATE,
             ratios: Optional[Sequence[float]] = None) -> List[CutSyncResult]:
    """Sync of subtitles made for another cut of the video.  ``problems``: list of (reference, track) as
    ``split_align.split_sync`` takes them.  Per problem: the framerate ratio from the windowless seven-ratio solve, the
    split over ``lag_range`` (one (lag_lo, lag_hi) for every problem; None = each pair's full overlap range), the
    refined breaks, and every cue's output time, or piece -2 for a cue the video does not have."""
    validate_args(block_samples, split_penalty)
    split_refine.validate_args(block_samples, radius_samples, unmatched_margin)
    if lag_range is not None:
        lag_range = validate_range(lag_range)
    split = lambda chosen: split_align_range_batch(chosen, lag_range, block_samples, split_penalty)
    return _cut_sync(problems, lag_range, block_samples, radius_samples, unmatched_margin, sample_rate, ratios, split)


def _cut_sync(problems, lag_range, block_samples, radius_samples, unmatched_margin, sample_rate, ratios, split):
    """``cut_sync``'s work (arguments checked) with ``split(chosen batch)`` -> one SplitResult per problem."""
    ratios = list(candidate_ratios() if ratios is None else ratios)
    db, best, pres = solve_ratios_windowless(problems, ratios, sample_rate)
    chosen = db.select_candidates(best)
    results = split(chosen)
    breaks = split_refine.refine_breaks_batch(chosen, results, block_samples, radius_samples, unmatched_margin)
    out = []
    for p, ((_, (start_us, end_us, _meta)), res, brk) in enumerate(zip(problems, results, breaks)):
        ratio = ratios[int(best[p])]
        cs, ce, which, um = split_refine.map_cues_refined(start_us, end_us, ratio, res.pieces, brk, sample_rate)
        rng = lag_range if lag_range is not None else full_range(chosen.lens[p, 0], chosen.lens[p, 1])
        out.append(CutSyncResult(ratio, int(best[p]), int(pres[p]["offset"]), rng, res.pieces, res.total, brk, cs, ce,
                                 which, um))
    return out
