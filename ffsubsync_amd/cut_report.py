"""Checked cut sync: a quality report for every piece of a full-range split (``cut_align``), and a decision per file.

``cut_sync`` returns pieces over each pair's full overlap range -- about 1.44 M lags for a 2 h pair, twelve times the
+-10 min window of ``split_report`` -- and nothing that says whether a piece or a break is real; a subtitle of another
film still gets a tidy set of pieces.  ``split_range_report_batch`` adds, per piece, the correlation curve of the piece's
OWN subtitle samples over the split's whole lag range, counted exactly on the device from the bits
(``csrc/ffs_cut_report.h``), with ``split_report``'s records and host derivation (psr, margin, gain_prev / gain_next).
``checked_cut_sync`` then decides per file:

    verified piece   not flat and psr >= min_piece_psr
    supported break  between two consecutive verified pieces: gain_next of the first and gain_prev of the second both
                     >= min_gain
    coverage         sum of (end_sample - start_sample) over the verified pieces, divided by S

    "cut"        at least 2 pieces, at least one verified, coverage >= min_coverage, and every break between
                 consecutive verified pieces supported: ``cut_sync``'s cue times, bit for bit
    "single"     exactly one piece, and it is verified: ``cut_sync``'s cue times
    "untrusted"  anything else: the input cue times, unmodified (upstream's ``--skip-sync-on-low-quality``)

Unverified pieces are flagged, never merged or re-solved.  ``cut_sync``, ``split_align_range_batch`` and every other
existing entry point are unchanged.
"""
import math
import numbers
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native, cut_align, quality, split_refine
from .constants import SAMPLE_RATE
from .side_call import BlockCall, pairs_for_budget, record_lists
from .split_align import DEFAULT_BLOCK_SAMPLES, Piece, _check_batch, split_outputs, split_results
from .split_report import DEFAULT_EXCLUSION_SAMPLES, DEFAULT_TOP_K, PieceQuality, SplitReport, from_record

# Chosen on the device over the full range (profiles/cut_report_calibration.py; synthetic data only)
DEFAULT_MIN_PIECE_PSR = 9.0
DEFAULT_MIN_GAIN = 6.0
DEFAULT_MIN_COVERAGE = 0.5
ROUND_PIECES = 8  # piece rows per pair and round of the device report (CUT_ROUND_PIECES)
DECISIONS = ("cut", "single", "untrusted")


@dataclass
class CheckedCutResult:
    decision: str  # "cut", "single" or "untrusted"
    reasons: List[str]  # every unverified piece, unsupported break and a coverage below the bar
    ratio: float  # framerate ratio picked by the windowless seven-ratio solve
    ratio_index: int
    global_offset: int  # that solve's single offset (samples)
    lag_range: Tuple[int, int]  # the split's lag range
    pieces: List[Piece]  # the range split's pieces (what cut_sync returns)
    total: float
    breaks: List[split_refine.RefinedBreak]  # cut_sync's refined breaks
    piece_quality: List[PieceQuality]
    verified: List[bool]  # per piece
    supported: List[bool]  # per break (between pieces i and i+1)
    coverage: float
    cue_start_us: np.ndarray  # output cue times (int64 microseconds) of the decision
    cue_end_us: np.ndarray
    cue_piece: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))  # -2 unmatched; -1 for "untrusted"
    cue_unmatched: np.ndarray = field(default_factory=lambda: np.zeros(0, bool))
    cue_verified: np.ndarray = field(default_factory=lambda: np.zeros(0, bool))  # the cue's piece is verified


def _real(v) -> bool:
    return isinstance(v, numbers.Real) and not isinstance(v, (bool, np.bool_)) and not math.isnan(float(v))


def validate_thresholds(min_piece_psr, min_gain, min_coverage) -> None:
    """Host-side checks of the decision thresholds (ValueError)."""
    for name, v in (("min_piece_psr", min_piece_psr), ("min_gain", min_gain)):
        if not _real(v):
            raise ValueError("%s=%r: need a number (not NaN)" % (name, v))
    if not _real(min_coverage) or not 0.0 <= float(min_coverage) <= 1.0:
        raise ValueError("min_coverage=%r: need a number in [0, 1]" % (min_coverage,))


def validate_args(block_samples, split_penalty, top_k, exclusion_samples) -> None:
    """Host-side checks of the call parameters (ValueError before any native call)."""
    cut_align.validate_args(block_samples, split_penalty)
    quality.validate_args(None, top_k, exclusion_samples)


def assess_cut(pieces: Sequence[PieceQuality], min_piece_psr: float = DEFAULT_MIN_PIECE_PSR,
               min_gain: float = DEFAULT_MIN_GAIN,
               min_coverage: float = DEFAULT_MIN_COVERAGE) -> Tuple[List[str], List[bool], List[bool], float]:
    """(reasons, verified per piece, supported per break, coverage) of one full-range split's piece reports.  Reasons are
    worded like ``split_report.assess_split``; a break next to an unverified piece is not supported and gives no reason
    of its own (its piece does)."""
    validate_thresholds(min_piece_psr, min_gain, min_coverage)
    reasons: List[str] = []
    verified = []
    for i, q in enumerate(pieces):
        ok = not q.flat and q.psr >= min_piece_psr
        verified.append(bool(ok))
        if q.flat:
            reasons.append("piece %d: flat correlation (std 0)" % i)
        elif not ok:
            reasons.append("piece %d: psr %.1f < %.1f" % (i, q.psr, min_piece_psr))
    supported = []
    for i, (a, b) in enumerate(zip(pieces[:-1], pieces[1:])):
        both = verified[i] and verified[i + 1]
        ok = both and a.gain_next >= min_gain and b.gain_prev >= min_gain
        supported.append(bool(ok))
        if both and not ok:
            reasons.append("break %d (block %d): gain %.1f / %.1f < %.1f" % (i, b.first_block, a.gain_next, b.gain_prev,
                                                                              min_gain))
    total = pieces[-1].end_sample if pieces else 0
    covered = sum(q.end_sample - q.start_sample for q, v in zip(pieces, verified) if v)
    coverage = covered / total if total > 0 else 0.0
    if coverage < min_coverage:
        reasons.append("coverage %.3f < %.3f" % (coverage, min_coverage))
    return reasons, verified, supported, coverage


def decide(verified: Sequence[bool], supported: Sequence[bool], coverage: float,
           min_coverage: float = DEFAULT_MIN_COVERAGE) -> str:
    """The decision of ``assess_cut``'s results (see the module docstring)."""
    n = len(verified)
    if n >= 2 and any(verified) and coverage >= min_coverage and all(
            supported[i] for i in range(n - 1) if verified[i] and verified[i + 1]):
        return "cut"
    if n == 1 and verified[0]:
        return "single"
    return "untrusted"


_plans = _native.SidePlanCache(_native.SplitRangePlan)


def _get_plan(n_pairs: int, max_blocks: int, max_lags: int, max_samples: int, pairs_in_flight: Optional[int]):
    """The report's own plan, sized for the piece rows its first report call adds (8 uint32 rows of max_lags per pair)."""
    if pairs_in_flight is None:  # the range split's workspace plus the rows: ~186 MB per 2 h full-range pair, ~12 GiB
        per_pair = (cut_align.workspace_per_pair(max_blocks, max_lags, max_samples)
                    + ROUND_PIECES * (max_lags + 64) * 4.0 + (max_samples / 16384.0 + max_blocks) * 16.0)
        pairs_in_flight = pairs_for_budget(n_pairs, per_pair)
    return _plans.get(pairs_in_flight, max_blocks, max_lags, max_samples, role="report")


def clear_plan_cache() -> None:
    _plans.clear()


def _records(call, plan, record_dtype, lo, hi, path, top_k, exclusion_samples):
    """The device report of a range plan over ``path``, the CUDA tensors [n_pairs * max_b] it reports on (block offsets;
    for a drift path jump flags too): (``record_dtype`` records [n_pairs, max_b], counts)."""
    rep_out, n_out = call.records(record_dtype), call.per_pair(np.int32)
    plan.report(*call.pair_arrays(), call.k, lo, hi, *path, int(top_k), int(exclusion_samples), rep_out, n_out)
    return call.read_records(rep_out, record_dtype), n_out.cpu().numpy()


def report_batch(batch, block_offsets, lag_ranges=None, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                 top_k: int = DEFAULT_TOP_K, exclusion_samples: int = DEFAULT_EXCLUSION_SAMPLES,
                 pairs_in_flight: Optional[int] = None):
    """The piece reports of given block offsets (int array [n_pairs, >= max_b] or a list of one array of B_p offsets
    per pair; every offset inside its pair's range) over ``lag_ranges`` (as ``cut_align.split_align_range_batch`` takes
    them).  Returns (``_native.PIECE_REPORT_DTYPE`` records [n_pairs, max_b], piece counts)."""
    validate_args(block_samples, 0.0, top_k, exclusion_samples)
    _check_batch(batch)
    lo, hi = cut_align.lag_arrays(batch, lag_ranges)
    call = BlockCall(batch, block_samples)
    what = lambda p, size, blocks: "pair %d: %d block offsets for %d blocks" % (p, size, blocks)
    path = call.place(what, ([np.asarray(block_offsets[p], dtype=np.int64) for p in range(call.n)], np.int32), clip=True)
    plan = _get_plan(call.n, call.max_b, *call.lag_dims(lo, hi), pairs_in_flight)
    return _records(call, plan, _native.PIECE_REPORT_DTYPE, lo, hi, path, top_k, exclusion_samples)


def split_range_report_batch(batch, lag_ranges=None, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                             split_penalty: float = cut_align.DEFAULT_CUT_PENALTY, top_k: int = DEFAULT_TOP_K,
                             exclusion_samples: int = DEFAULT_EXCLUSION_SAMPLES, pairs_in_flight: Optional[int] = None,
                             raw: bool = False):
    """``cut_align.split_align_range_batch`` (same inputs, same checks, bit-identical result) plus the quality report of
    every piece over the pair's lag range, on the device block offsets.  Returns one ``split_report.SplitReport`` per
    pair, or with ``raw`` (SplitResults, ``_native.PIECE_REPORT_DTYPE`` records [n_pairs, max_b], piece counts)."""
    validate_args(block_samples, split_penalty, top_k, exclusion_samples)
    _check_batch(batch)
    lo, hi = cut_align.lag_arrays(batch, lag_ranges)
    call = BlockCall(batch, block_samples)
    plan = _get_plan(call.n, call.max_b, *call.lag_dims(lo, hi), pairs_in_flight)
    outs = split_outputs(call.n, call.max_b, call.dev)
    plan.align(*call.pair_arrays(), call.k, lo, hi, float(split_penalty), *outs)
    recs, counts = _records(call, plan, _native.PIECE_REPORT_DTYPE, lo, hi, outs[:1], top_k, exclusion_samples)
    res = split_results(outs, call.n_blocks, call.k, call.sub_len)
    if raw:
        return res, recs, counts
    return [SplitReport(r, q) for r, q in zip(res, record_lists(recs, counts, from_record))]


def checked_cut_sync(problems, lag_range=None, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                     split_penalty: float = cut_align.DEFAULT_CUT_PENALTY,
                     radius_samples: int = split_refine.DEFAULT_RADIUS_SAMPLES,
                     unmatched_margin: Optional[float] = split_refine.DEFAULT_UNMATCHED_MARGIN,
                     sample_rate: int = SAMPLE_RATE, ratios: Optional[Sequence[float]] = None,
                     top_k: int = DEFAULT_TOP_K, exclusion_samples: int = DEFAULT_EXCLUSION_SAMPLES,
                     min_piece_psr: float = DEFAULT_MIN_PIECE_PSR, min_gain: float = DEFAULT_MIN_GAIN,
                     min_coverage: float = DEFAULT_MIN_COVERAGE) -> List[CheckedCutResult]:
    """``cut_align.cut_sync`` (``problems`` and its arguments as it takes them) with the piece reports and one decision
    per problem (see the module docstring)."""
    validate_args(block_samples, split_penalty, top_k, exclusion_samples)
    split_refine.validate_args(block_samples, radius_samples, unmatched_margin)
    validate_thresholds(min_piece_psr, min_gain, min_coverage)
    if lag_range is not None:
        lag_range = cut_align.validate_range(lag_range)
    reports: List[SplitReport] = []

    def split(chosen):
        reports.extend(split_range_report_batch(chosen, lag_range, block_samples, split_penalty, top_k,
                                                exclusion_samples))
        return [r.split for r in reports]

    synced = cut_align._cut_sync(problems, lag_range, block_samples, radius_samples, unmatched_margin, sample_rate,
                                 ratios, split)
    out = []
    for (_, (start_us, end_us, _meta)), c, rep in zip(problems, synced, reports):
        reasons, verified, supported, coverage = assess_cut(rep.pieces, min_piece_psr, min_gain, min_coverage)
        decision = decide(verified, supported, coverage, min_coverage)
        if decision == "untrusted":
            cs = np.asarray(start_us, dtype=np.int64).copy()
            ce = np.asarray(end_us, dtype=np.int64).copy()
            which = np.full(len(cs), -1, np.int64)
            um = np.zeros(len(cs), bool)
            cv = np.zeros(len(cs), bool)
        else:
            cs, ce, which, um = c.cue_start_us, c.cue_end_us, c.cue_piece, c.cue_unmatched
            ver = np.asarray(verified, bool)
            cv = ~um & (which >= 0) & ver[np.clip(which, 0, len(ver) - 1)]
        out.append(CheckedCutResult(decision, reasons, c.ratio, c.ratio_index, c.global_offset, c.lag_range, c.pieces,
                                    c.total, c.breaks, rep.pieces, verified, supported, coverage, cs, ce, which, um, cv))
    return out
