"""Ratio sweep: find an unknown speed factor by an exhaustive search.

Every aligner here models the speed error as one of seven framerate ratios plus whatever a drift path absorbs.  A
subtitle whose speed factor is none of the seven -- an odd re-encode, a PAL speed-up on top of another conversion -- is
handled by none of them, and golden-section search (``batch_gss.fit_gss_batch``, upstream's ``--gss``) optimises an
objective that is not unimodal: the true peak is ~1e-3 wide in ratio, and 17 evaluations land on it by luck.  This module
evaluates the reference's own objective -- ``FFTAligner(W).fit(reference, rasterise(track, r))`` -- at EVERY ratio of a
grid fine enough not to miss the peak, which the run-boundary solve makes cheap:

    sweep_grid            the grid: step = 4 * tolerance / duration, so that at the grid point nearest the true ratio no
                          cue is misplaced by more than ``tolerance`` samples (ratio error times half the duration)
    ratio_profile_batch   one ffs_cand_result per (file, grid point), the records staying in HBM as a [file][g] table
    sweep_peaks           ``ffs_sweep_peaks``: the table reduced on the device to one record of peaks and moments a file
    sweep_sync            coarse sweep, peaks, a fine stage around each peak plus the seven ratios exactly, an answer and
                          the reasons not to trust it; ``ratio`` feeds any ``*_sync(problems, ratios=[r.ratio])``

Parity is against the in-repo numpy model ``tests/sweep_model.py``.  Nothing here changes an existing entry point;
nothing is reachable from the reference CLI.
"""
import math
from dataclasses import dataclass
from datetime import timedelta
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native, quality
from .aligners import MAX_FRAMERATE_RATIO, MIN_FRAMERATE_RATIO
from .constants import SAMPLE_RATE, candidate_ratios
from .side_call import empty_error, pairs_for_budget

# Chosen on the CPU model by the rules of DESIGN 3.21 (profiles/ratio_sweep_calibration.json; synthetic data, 10 min and
# 1 h): the largest tolerance whose grid maximum keeps >= 0.9 of the exact-ratio score, and the midpoints between the
# matched classes and wrong files
DEFAULT_TOLERANCE = 40.0  # worst kept fraction 0.901 (0.824 at 60)
DEFAULT_MIN_PSR = 4.46  # matched >= 4.59, wrong <= 4.34
DEFAULT_MIN_MARGIN = 2.85  # matched >= 3.56, wrong <= 2.13
DEFAULT_TOP_K = 3
MAX_TOP_K = _native.SWEEP_MAX_PEAKS
MAX_GRID = 1 << 20
FINE_HALF = 16  # fine points on either side of a coarse peak ...
FINE_DIV = 16  # ... at 1/16 of the coarse step
CHUNK_BUDGET = 2 << 30  # bytes of rasterised vectors one rasteriser + solve call may hold
CHUNK_CAP = 1 << 16  # vectors per call at most
EDGE_REASON = "best ratio at the edge of [lo, hi]"


@dataclass
class RatioProfile:
    """Ratio profiles of n files: file f owns the points [first[f], first[f+1]) of ``table``."""

    grids: List[np.ndarray]  # float64 ratios of every file
    steps: List[float]
    first: np.ndarray  # int64 [n + 1]
    table: "object"  # uint8 CUDA tensor: first[n] ffs_cand_result records
    first_dev: "object"  # int64 CUDA tensor of ``first``
    stats: dict

    def records(self) -> List[np.ndarray]:
        """The records on the host: one ``_native.CAND_RESULT_DTYPE`` array per file (reads the whole table back)."""
        recs = self.table.cpu().numpy().view(_native.CAND_RESULT_DTYPE)
        return [recs[int(a):int(b)] for a, b in zip(self.first[:-1], self.first[1:])]


@dataclass
class SweepProfile:
    peaks: List[Tuple[float, int, float]]  # (score, offset in samples, ratio) of the coarse peaks, the maximum first
    mean: float  # of the scores over the grid points not skipped
    std: float
    n_points: int
    n_skipped: int
    psr: float  # (peak1 - mean) / std; 0 when std == 0
    margin: float  # (peak1 - peak2) / std; +inf with one peak; 0 when std == 0
    flags: int  # _native.SWEEP_FLAT / SWEEP_EMPTY / SWEEP_AMBIGUOUS


@dataclass
class SweepSyncResult:
    ratio: float  # the speed factor found: feed it to any ``*_sync(problems, ratios=[ratio])``
    offset: int  # samples, at that ratio
    score: float
    coarse_ratio: float  # the coarse peak the answer belongs to
    profile: SweepProfile
    reasons: List[str]  # empty = trust the result


def _check_range(lo, hi, tolerance_samples) -> Tuple[float, float, float]:
    try:
        lo, hi, tol = float(lo), float(hi), float(tolerance_samples)
    except (TypeError, ValueError):
        raise ValueError("lo=%r, hi=%r, tolerance_samples=%r: need numbers" % (lo, hi, tolerance_samples))
    if not (math.isfinite(lo) and math.isfinite(hi)) or not 0 < lo <= hi:
        raise ValueError("lo=%r, hi=%r: need finite ratios with 0 < lo <= hi" % (lo, hi))
    if not math.isfinite(tol) or tol < 1:
        raise ValueError("tolerance_samples=%r: need a finite number >= 1" % (tolerance_samples,))
    return lo, hi, tol


def sweep_grid(duration_samples, lo: float = MIN_FRAMERATE_RATIO, hi: float = MAX_FRAMERATE_RATIO,
               tolerance_samples: float = DEFAULT_TOLERANCE) -> np.ndarray:
    """The ratios ``lo + step * arange(G)`` (float64; one multiply and one add a point, each rounded on its own) with
    step = 4 * tolerance / duration_samples and the last point <= hi.  ``duration_samples``: the track's raster length
    at ratio 1.  At the grid point nearest the true ratio, with the offset free, no cue is misplaced by more than
    ``tolerance_samples``: the misplacement is the ratio error (at most step / 2) times half the duration."""
    lo, hi, tol = _check_range(lo, hi, tolerance_samples)
    d = int(duration_samples)
    if d != duration_samples or d < 1:
        raise ValueError("duration_samples=%r: need an integer >= 1" % (duration_samples,))
    step = 4.0 * tol / float(d)
    g = int(math.floor((hi - lo) / step)) + 1
    if g > MAX_GRID:
        raise ValueError("%d grid points in [%r, %r] at tolerance %r: more than 2^20" % (g, lo, hi, tol))
    while g > 1 and lo + step * (g - 1) > hi:
        g -= 1
    while lo + step * g <= hi:
        g += 1
    return lo + step * np.arange(g, dtype=np.float64)


def track_duration_samples(track, sample_rate: int = SAMPLE_RATE) -> int:
    """The raster length of a (start_us, end_us, is_metadata) track at ratio 1 (speech_transformers.py:962)."""
    return int(timedelta(microseconds=int(np.max(track[1]))).total_seconds() * sample_rate) + 2


def default_exclusion_steps(tolerance_samples: float = DEFAULT_TOLERANCE) -> int:
    """Two ratios whose end-of-file misplacement differs by less than ``quality.DEFAULT_EXCLUSION_SAMPLES`` (3 s) are the
    same ridge: a grid step moves the end of the file by 2 * tolerance samples against its middle."""
    return max(1, int(math.ceil(quality.DEFAULT_EXCLUSION_SAMPLES / (2.0 * float(tolerance_samples)))))


def _check_peak_args(top_k, exclusion_steps) -> None:
    k = int(top_k)
    if k != top_k or not 1 <= k <= MAX_TOP_K:
        raise ValueError("top_k=%r: need an integer in [1, %d]" % (top_k, MAX_TOP_K))
    if exclusion_steps is not None:
        e = int(exclusion_steps)
        if e != exclusion_steps or e < 1:
            raise ValueError("exclusion_steps=%r: need an integer >= 1" % (exclusion_steps,))


def _check_problems(problems, max_offset_seconds, sample_rate, budget_bytes):
    """Host checks of a problem list (ValueError before any native call); returns the lag window in samples."""
    if int(sample_rate) != sample_rate or sample_rate < 1:
        raise ValueError("sample_rate=%r: need an integer >= 1" % (sample_rate,))
    if int(budget_bytes) < 1:
        raise ValueError("budget_bytes=%r: need a positive number of bytes" % (budget_bytes,))
    w = int(round(max_offset_seconds * sample_rate))
    if not math.isfinite(max_offset_seconds) or w < 1:
        raise ValueError("max_offset_seconds=%r: need a window of at least one sample" % (max_offset_seconds,))
    for p in problems:
        if len(p) != 2 or len(p[1]) != 3:
            raise ValueError("a problem is (reference, (start_us, end_us, is_metadata))")
        ref, track = p
        if len(track[0]) != len(track[1]):
            raise ValueError("start and end times of different lengths")
        if len(track[0]) == 0:
            raise empty_error(len(ref), 0)
        if len(ref) == 0:
            raise empty_error(0, 1)
    return w


def _solver(problems, w, sample_rate, longest_ratio, max_vectors):
    """The prepared solve of the problems' files (``batch_gss.PreparedRatioSolve``); multi-level references refused."""
    from .aligners import _Vec
    from .batch_gss import PreparedRatioSolve

    ref_vecs = [_Vec(ref) for ref, _ in problems]
    for v in ref_vecs:
        if not v.two_level:
            raise ValueError("ratio_profile_batch needs a two-level reference: a multi-level float reference "
                             "(FFS_DTYPE_F64) is not supported")
    tracks = [(np.asarray(s), np.asarray(e), None if m is None else np.asarray(m)) for _, (s, e, m) in problems]
    return ref_vecs, PreparedRatioSolve(ref_vecs, tracks, w, sample_rate, 0, longest_ratio, max_vectors, max_cand=1)


def _evaluate(solver, ref_vecs, problems, which, ratios, first, chunk_vectors, sample_rate, stats):
    """The records of the vectors (file ``which[v]``, ``ratios[v]``), file by file in ``first``'s layout, as a uint8 CUDA
    table: chunks of ``chunk_vectors`` through ``solver.evaluate``; a file with an AMBIGUOUS record is redone on the
    careful per-file path."""
    torch = solver.torch
    total = int(which.size)
    table = torch.empty(max(total, 1) * 24, dtype=torch.uint8, device="cuda")
    for a in range(0, total, chunk_vectors):
        b = min(a + chunk_vectors, total)
        solver.evaluate(which[a:b], ratios[a:b], table[a * 24:])
        stats["chunks"] = stats.get("chunks", 0) + 1
    stats["vectors"] = stats.get("vectors", 0) + total
    if total:
        flags = table[:total * 24].view(torch.int32).reshape(total, 6)[:, 5]
        amb = (flags & _native.FLAG_AMBIGUOUS) != 0
        if bool(amb.any()):  # degenerate input (e.g. a silent reference): the careful path, file by file
            amb_h = amb.cpu().numpy()
            for f in range(len(problems)):
                a, b = int(first[f]), int(first[f + 1])
                if amb_h[a:b].any():
                    recs = _careful(ref_vecs[f], problems[f][1], ratios[a:b], solver.max_offset_samples, sample_rate)
                    table[a * 24:b * 24] = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
                    stats["careful_files"] = stats.get("careful_files", 0) + 1
    return table


def _careful(ref_vec, track, ratios, max_offset_samples, sample_rate) -> np.ndarray:
    """The same records through the drop-in's ``solve_pairs`` (ambiguity handling), one rasterisation per ratio."""
    from .aligners import _Vec, solve_pairs
    from .subtitle_raster import rasterize_candidates

    s, e, m = track
    pairs = [(ref_vec, [_Vec(rasterize_candidates(s, e, m, [float(r)], sample_rate, 0)[0])]) for r in ratios]
    cres, _ = solve_pairs(pairs, max_offset_samples)
    return np.ascontiguousarray(cres[:, 0])


def _chunk_vectors(solver, longest_ratio, total, budget_bytes) -> int:
    return pairs_for_budget(total, solver.vector_bytes(longest_ratio), cap=CHUNK_CAP, budget=int(budget_bytes))


def ratio_profile_batch(problems, max_offset_seconds: float = 60, lo: float = MIN_FRAMERATE_RATIO,
                        hi: float = MAX_FRAMERATE_RATIO, tolerance_samples: float = DEFAULT_TOLERANCE,
                        sample_rate: int = SAMPLE_RATE, budget_bytes: int = CHUNK_BUDGET, _prepared=None) -> RatioProfile:
    """The ratio profile of many files.  ``problems``: as ``split_align.split_sync`` takes them, a list of (reference,
    track) with the reference a two-level host vector or a ``subtitle_raster.DeviceRaster`` and the track a
    (start_us, end_us, is_metadata) triple.  Per problem: its grid (``sweep_grid`` of its own duration) and one
    ``ffs_cand_result`` per grid point -- exactly what ``MaxScoreAligner.fit_gss``'s objective evaluates at that ratio,
    amplitude min(1/r, 1) included -- in an HBM table ``[file][g]``.

    The correlation is the existing solve: the references become boundary lists once and the subtitle tables are
    uploaded once (``batch_gss.PreparedRatioSolve``, shared with ``fit_gss_batch``); per chunk of (file, ratio) vectors --
    as many as ``budget_bytes`` (about 2 GiB) of list blocks hold -- one rasteriser call and one ``align_batch(n, 1, ...)``.
    A reference too dense for a list sends the call through the bit rasters; a file whose records carry
    ``FFS_FLAG_AMBIGUOUS`` is redone on the careful per-file path; multi-level float references are refused."""
    lo, hi, tol = _check_range(lo, hi, tolerance_samples)
    w = _check_problems(problems, max_offset_seconds, sample_rate, budget_bytes)
    grids = [sweep_grid(track_duration_samples(track, sample_rate), lo, hi, tol) for _, track in problems]
    steps = [4.0 * tol / float(track_duration_samples(track, sample_rate)) for _, track in problems]
    first = np.zeros(len(problems) + 1, dtype=np.int64)
    np.cumsum([g.size for g in grids], out=first[1:])
    torch = _native.require_gpu()
    stats = {}
    if not problems:
        return RatioProfile([], [], first, torch.empty(24, dtype=torch.uint8, device="cuda"),
                            torch.from_numpy(first).cuda(), stats)
    longest = max(hi, max(candidate_ratios()))
    ref_vecs, solver = _prepared if _prepared is not None else _solver(problems, w, sample_rate, longest, int(first[-1]))
    which = np.repeat(np.arange(len(problems)), [g.size for g in grids])
    ratios = np.concatenate(grids)
    chunk = _chunk_vectors(solver, longest, int(first[-1]), budget_bytes)
    table = _evaluate(solver, ref_vecs, problems, which, ratios, first, chunk, sample_rate, stats)
    stats.update({"files": len(problems), "plan_length": int(solver.n_fft), "lists": bool(solver.use_lists),
                  "chunk_vectors": int(chunk), "vector_bytes": solver.vector_bytes(longest)})
    return RatioProfile(grids, steps, first, table, torch.from_numpy(first).cuda(), stats)


def sweep_peaks(table, first, top_k: int = DEFAULT_TOP_K, exclusion_steps: Optional[int] = None, raw: bool = False):
    """``ffs_sweep_peaks``: peaks and moments of every file's profile, computed on the device.  ``table``: a CUDA tensor
    of ffs_cand_result records (``RatioProfile.table``); ``first``: the n + 1 ascending first point indices of the files
    (host array or int64 CUDA tensor).  ``exclusion_steps`` defaults to ``default_exclusion_steps()``.  Returns one
    ``_native.SWEEP_PROFILE_DTYPE`` record per file (a host array); with ``raw`` the uint8 CUDA tensor that holds them."""
    _check_peak_args(top_k, exclusion_steps)
    e = default_exclusion_steps() if exclusion_steps is None else int(exclusion_steps)
    torch = _native.require_gpu()
    if not torch.is_tensor(first):
        host = np.ascontiguousarray(first, dtype=np.int64)
        if host.ndim != 1 or host.size < 1 or (np.diff(host) < 0).any() or host[0] < 0:
            raise ValueError("first: need n + 1 ascending point indices from 0 on")
        if int(host[-1]) * 24 > table.numel() * table.element_size():
            raise ValueError("first: the table holds fewer than %d records" % int(host[-1]))
        first = torch.from_numpy(host).cuda()
    n_files = first.numel() - 1
    out = _native.sweep_peaks(table, first, n_files, int(top_k), e)
    if raw:
        return out
    return out.cpu().numpy().view(_native.SWEEP_PROFILE_DTYPE)[:n_files]


def profile_from_record(rec, grid) -> SweepProfile:
    """SweepProfile of one ``_native.SWEEP_PROFILE_DTYPE`` record, psr and margin derived as ``quality.derive`` does."""
    n = int(rec["n_peaks"])
    peaks = [(float(rec["peak_score"][i]), int(rec["peak_offset"][i]), float(grid[int(rec["peak_index"][i])])) for i in range(n)]
    mean, std, flags = float(rec["mean"]), float(rec["std"]), int(rec["flags"])
    psr, margin, _, _ = quality.derive(peaks, mean, std, 0)
    if std == 0 or not peaks:
        flags |= _native.SWEEP_FLAT
    return SweepProfile(peaks, mean, std, int(rec["n_points"]), int(rec["n_skipped"]), psr, margin, flags)


def assess(profile: SweepProfile, at_edge: bool = False, min_psr: float = DEFAULT_MIN_PSR,
           min_margin: float = DEFAULT_MIN_MARGIN) -> List[str]:
    """Reasons not to trust a sweep, worded like ``quality.assess``; an empty list means trust it."""
    if profile.flags & _native.SWEEP_EMPTY:
        return ["empty ratio profile"]
    if profile.flags & _native.SWEEP_FLAT:
        return ["flat ratio profile (std 0)"]
    reasons: List[str] = []
    if profile.psr < min_psr:
        reasons.append("psr %.1f < %.1f" % (profile.psr, min_psr))
    if profile.margin < min_margin:
        reasons.append("margin %.1f < %.1f" % (profile.margin, min_margin))
    if at_edge:
        reasons.append(EDGE_REASON)
    return reasons


def fine_ratios(coarse_ratios: Sequence[float], step: float, lo: float, hi: float):
    """(ratios, coarse peak number of each) of the fine stage: per coarse peak the 33 ratios r_peak + j * (step / 16),
    j in [-16, 16], clipped to [lo, hi]; then the seven framerate ratios exactly (their peak: the nearest one)."""
    fine = step / FINE_DIV
    rs, owner = [], []
    for k, rp in enumerate(coarse_ratios):
        for j in range(-FINE_HALF, FINE_HALF + 1):
            rs.append(min(max(rp + j * fine, lo), hi))
            owner.append(k)
    for r in candidate_ratios():
        rs.append(float(r))
        owner.append(int(np.argmin([abs(r - rp) for rp in coarse_ratios])))
    return np.array(rs, dtype=np.float64), np.array(owner, dtype=np.int64)


def pick(ratios, owner, coarse_ratios, recs) -> int:
    """Index of the answer among the fine points: the largest score among the points not skipped, ties to the ratio
    nearest its coarse peak, then to the smaller ratio; -1 when every point is skipped."""
    scores = recs["score"]
    ok = np.flatnonzero(np.isfinite(scores) & ((recs["flags"] & _native.FLAG_EMPTY_WINDOW) == 0))
    if ok.size == 0:
        return -1
    dist = np.abs(ratios - np.asarray(coarse_ratios, dtype=np.float64)[owner])
    return int(min(ok, key=lambda i: (-scores[i], dist[i], ratios[i])))


def sweep_sync(problems, max_offset_seconds: float = 60, lo: float = MIN_FRAMERATE_RATIO, hi: float = MAX_FRAMERATE_RATIO,
               tolerance_samples: float = DEFAULT_TOLERANCE, top_k: int = DEFAULT_TOP_K,
               exclusion_steps: Optional[int] = None, min_psr: float = DEFAULT_MIN_PSR,
               min_margin: float = DEFAULT_MIN_MARGIN, sample_rate: int = SAMPLE_RATE,
               budget_bytes: int = CHUNK_BUDGET) -> List[SweepSyncResult]:
    """Sync many files whose speed factor is unknown, and say which results to trust.  Per problem (as
    ``ratio_profile_batch`` takes them): the coarse profile over [lo, hi], its ``top_k`` peaks (``sweep_peaks``), a fine
    stage of 33 ratios around each peak plus the seven framerate ratios exactly -- one more call of the same prepared
    solve, so the answer is never worse than the seven-ratio solve's -- and the largest score of the fine stage.
    ``reasons`` is ``assess`` of the coarse profile (empty = trust it), plus "best ratio at the edge of [lo, hi]" when the
    answer's coarse peak is the first or last grid point."""
    lo, hi, tol = _check_range(lo, hi, tolerance_samples)
    _check_peak_args(top_k, exclusion_steps)
    w = _check_problems(problems, max_offset_seconds, sample_rate, budget_bytes)
    if not problems:
        return []
    e = default_exclusion_steps(tol) if exclusion_steps is None else int(exclusion_steps)
    longest = max(hi, max(candidate_ratios()))
    n_grid = sum(sweep_grid(track_duration_samples(t, sample_rate), lo, hi, tol).size for _, t in problems)
    prepared = _solver(problems, w, sample_rate, longest, n_grid)
    prof = ratio_profile_batch(problems, max_offset_seconds, lo, hi, tol, sample_rate, budget_bytes, _prepared=prepared)
    recs = sweep_peaks(prof.table, prof.first_dev, top_k, e)
    profiles = [profile_from_record(r, g) for r, g in zip(recs, prof.grids)]
    # the fine stage: every file with a peak, one more evaluation through the same prepared solve
    live = [f for f, p in enumerate(profiles) if p.peaks]
    fine = {f: fine_ratios([pk[2] for pk in profiles[f].peaks], prof.steps[f], lo, hi) for f in live}
    first = np.zeros(len(problems) + 1, dtype=np.int64)
    np.cumsum([fine[f][0].size if f in fine else 0 for f in range(len(problems))], out=first[1:])
    fine_recs = None
    if live:
        ref_vecs, solver = prepared
        which = np.repeat(np.arange(len(problems)), np.diff(first))
        ratios = np.concatenate([fine[f][0] for f in live])
        chunk = _chunk_vectors(solver, longest, int(first[-1]), budget_bytes)
        table = _evaluate(solver, ref_vecs, problems, which, ratios, first, chunk, sample_rate, prof.stats)
        fine_recs = table.cpu().numpy().view(_native.CAND_RESULT_DTYPE)
    out = []
    for f, p in enumerate(profiles):
        ratio, offset, score, coarse, at_edge = math.nan, 0, -math.inf, math.nan, False
        if f in fine:
            fr, owner = fine[f]
            coarse_ratios = [pk[2] for pk in p.peaks]
            fr_recs = fine_recs[int(first[f]):int(first[f + 1])]
            i = pick(fr, owner, coarse_ratios, fr_recs)
            if i >= 0:
                ratio, offset, score = float(fr[i]), int(fr_recs[i]["offset"]), float(fr_recs[i]["score"])
                coarse = coarse_ratios[int(owner[i])]
                at_edge = coarse in (float(prof.grids[f][0]), float(prof.grids[f][-1])) and prof.grids[f].size > 1
        reasons = assess(p, at_edge, min_psr, min_margin)
        if math.isnan(ratio) and not reasons:
            reasons = ["no ratio found an offset inside the window"]
        out.append(SweepSyncResult(ratio, offset, score, coarse, p, reasons))
    return out
