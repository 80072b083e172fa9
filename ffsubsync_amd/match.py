"""Match subtitles to videos: the quality report of every (video, subtitle) pair, and the assignment built on it.

A folder of videos and a folder of subtitle files whose names do not line up is an N x M problem: which subtitle belongs
to which video.  The raw correlation score cannot answer it (matched and wrong pairs almost meet); the
normalised statistics of ``quality.py`` can -- psr and margin separate the classes with ``quality``'s default thresholds
(synthetic data only).  ``match_quality`` computes them for every pair:

  1. the existing seven-ratio solve (``batch.BatchAligner``, unchanged) on every requested pair.  Each reference's
     boundary list and each track's seven rasterised lists are built ONCE; a pair's row of the ``DeviceBatch`` points at
     the shared vectors, nothing is copied per pair;
  2. ``ffs_match_quality_batch`` (csrc/ffs_match.h) on each pair's winning candidate: the n11 curve over the lag window
     straight from the two boundary lists, then the report of ``ffs_align_quality_batch`` -- the records are byte-identical
     to ``quality.quality_batch``'s, so ``peaks[0]`` equals the solve's (score, offset) bit for bit.

``assign`` turns the matrix into a matching on the host; ``match_library`` is both.  Split, cut and drift decisions per
matched pair are the caller's: run ``checked_*_sync`` on the assignments.  Nothing here changes an existing entry point.
"""
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native, quality
from .constants import SAMPLE_RATE, candidate_ratios
from .side_call import empty_error, pairs_for_budget

ALGORITHMS = tuple(sorted(_native.MATCH_ALGORITHMS))
DEFAULT_BLOCK_PAIRS = 16384  # pairs solved and reported at a time (whole reference rows)


@dataclass
class MatchMatrix:
    """[N references, M subtitles] arrays.  ``ratio_index`` -1: not requested, or no framerate ratio landed inside the
    window -- such a pair is never trusted (its other entries are 0 / NaN)."""

    ratios: List[float]
    ratio_index: np.ndarray  # int64
    offset: np.ndarray  # int64, samples (the solve's offset = peaks[0])
    score: np.ndarray  # float64 (the solve's score = peaks[0])
    psr: np.ndarray  # float64; 0 when std == 0
    margin: np.ndarray  # float64; +inf with one peak, 0 when std == 0
    flags: np.ndarray  # int32, _native.QUALITY_FLAT / QUALITY_EMPTY_WINDOW
    records: Optional[np.ndarray] = None  # [N, M] _native.QUALITY_RESULT_DTYPE on request

    @property
    def shape(self) -> Tuple[int, int]:
        return self.ratio_index.shape

    def trusted(self, min_psr: float = quality.DEFAULT_MIN_PSR, min_margin: float = quality.DEFAULT_MIN_MARGIN) -> np.ndarray:
        """[N, M] bool: the pairs ``quality.assess`` has no reason against (and whose solve landed inside the window)."""
        bad = (_native.QUALITY_EMPTY_WINDOW | _native.QUALITY_FLAT)
        with np.errstate(invalid="ignore"):
            return ((self.ratio_index >= 0) & ((self.flags & bad) == 0) & ~(self.psr < min_psr) & ~(self.margin < min_margin)
                    & ~np.isnan(self.psr) & ~np.isnan(self.margin))


@dataclass
class Assignment:
    reference: List[Optional[int]]  # per subtitle: its video, or None
    psr: np.ndarray  # per subtitle: the assigned pair's psr (NaN without one)
    runner_up_psr: np.ndarray  # per subtitle: psr of the best OTHER trusted reference (NaN when there is none)
    ambiguous: np.ndarray  # per subtitle: another trusted reference exists
    subtitles: List[List[int]]  # per video: its subtitles, ascending


@dataclass
class LibraryMatch:
    matrix: MatchMatrix
    assignment: Assignment
    pairs: List[dict]  # per assigned subtitle: subtitle, reference, ratio_index, ratio, offset, score, psr, margin


def empty_matrix(n_ref: int, n_sub: int, ratios: Sequence[float], raw: bool = False) -> MatchMatrix:
    shape = (int(n_ref), int(n_sub))
    return MatchMatrix([float(r) for r in ratios], np.full(shape, -1, np.int64), np.zeros(shape, np.int64),
                       np.zeros(shape, np.float64), np.full(shape, np.nan), np.full(shape, np.nan), np.zeros(shape, np.int32),
                       np.zeros(shape, _native.QUALITY_RESULT_DTYPE) if raw else None)


def derive(recs):
    """(psr, margin, flags) arrays of ``_native.QUALITY_RESULT_DTYPE`` records: ``quality.from_record``, vectorised."""
    recs = np.asarray(recs)
    n, std = recs["n_peaks"], recs["std"]
    p1, p2 = recs["peak_score"][..., 0], recs["peak_score"][..., 1]
    dead = (std == 0) | (n == 0)
    safe = np.where(dead, 1.0, std)
    psr = np.where(dead, 0.0, (p1 - recs["mean"]) / safe)
    margin = np.where(dead, 0.0, np.where(n > 1, (p1 - p2) / safe, math.inf))
    flags = np.where(dead, recs["flags"] | _native.QUALITY_FLAT, recs["flags"]).astype(np.int32)
    return psr, margin, flags


def validate_pairs(pairs, n_ref: int, n_sub: int) -> np.ndarray:
    """The requested index pairs as an [n, 2] int64 array (None: all N x M, row-major)."""
    if pairs is None:
        i, j = np.divmod(np.arange(n_ref * n_sub, dtype=np.int64), max(n_sub, 1))
        return np.stack([i, j], axis=1)
    arr = np.asarray(list(pairs), dtype=np.int64).reshape(-1, 2)
    if arr.size and (arr.min() < 0 or arr[:, 0].max() >= n_ref or arr[:, 1].max() >= n_sub):
        raise ValueError("pair index outside the %d references x %d tracks" % (n_ref, n_sub))
    return arr


def assign(matrix: MatchMatrix, min_psr: float = quality.DEFAULT_MIN_PSR, min_margin: float = quality.DEFAULT_MIN_MARGIN,
           exclusive: bool = False) -> Assignment:
    """Which video each subtitle belongs to.  A pair is trusted when ``quality.assess`` has no reason against it.  Per
    subtitle: the trusted reference with the largest psr (ties: the smaller reference index) or None, the psr of the
    best OTHER trusted reference (NaN when there is none) and ``ambiguous`` when one exists.  Several subtitles may share
    a video (languages do); ``exclusive`` takes the trusted pairs by descending psr (ties: smaller reference, then smaller
    subtitle index) and assigns a pair only while both sides are free.  Pure host code, deterministic."""
    n_ref, n_sub = matrix.shape
    ok = matrix.trusted(min_psr, min_margin)
    psr = np.where(ok, matrix.psr, -np.inf)
    reference: List[Optional[int]] = [None] * n_sub
    if exclusive:
        ii, jj = np.nonzero(ok)
        order = np.lexsort((jj, ii, -psr[ii, jj]))
        ref_free = np.ones(n_ref, bool)
        for i, j in zip(ii[order].tolist(), jj[order].tolist()):
            if ref_free[i] and reference[j] is None:
                reference[j] = i
                ref_free[i] = False
    else:
        for j in range(n_sub):
            if n_ref and ok[:, j].any():
                reference[j] = int(np.argmax(psr[:, j]))  # the first maximum: the smaller reference index on ties
    own = np.full(n_sub, np.nan)
    runner = np.full(n_sub, np.nan)
    ambiguous = np.zeros(n_sub, bool)
    subtitles: List[List[int]] = [[] for _ in range(n_ref)]
    for j, i in enumerate(reference):
        others = ok[:, j].copy()
        if i is not None:
            own[j] = matrix.psr[i, j]
            subtitles[i].append(j)
            others[i] = False
        if others.any():
            runner[j] = float(psr[others, j].max())
            ambiguous[j] = True
    return Assignment(reference, own, runner, ambiguous, subtitles)


_plans = _native.SidePlanCache(_native.MatchPlan)


def clear_plan_cache() -> None:
    _plans.clear()


def _get_plan(n_pairs: int, max_lags: int, max_samples: int, n_vectors: int, pairs_in_flight: Optional[int]):
    if pairs_in_flight is None:  # bound the per-pair workspace (12 B per lag) to ~2 GiB
        pairs_in_flight = pairs_for_budget(n_pairs, 12 * max_lags + 1, cap=1024, budget=2 << 30)
    return _plans.get(pairs_in_flight, max_lags, max_samples, max(n_vectors, 2))


def quality_from_lists(ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, pair_ref, pair_sub,
                       max_offset_samples: Optional[int], top_k: int = quality.DEFAULT_TOP_K,
                       exclusion_samples: int = quality.DEFAULT_EXCLUSION_SAMPLES, algorithm: str = "auto",
                       pairs_in_flight: Optional[int] = None, device=None):
    """The device call alone: tables of boundary lists (device pointers of ``ffs_runs_list`` blocks, lengths, levels) and
    index pairs -> one ``_native.QUALITY_RESULT_DTYPE`` record per pair, in pair order."""
    quality.validate_args(max_offset_samples, top_k, exclusion_samples)
    code = _native.match_algorithm_code(algorithm)
    torch = _native.require_gpu()
    ref_len, sub_len = np.asarray(ref_len, dtype=np.int64), np.asarray(sub_len, dtype=np.int64)
    pair_ref, pair_sub = np.asarray(pair_ref, dtype=np.int64).ravel(), np.asarray(pair_sub, dtype=np.int64).ravel()
    n = pair_ref.size
    if n == 0:
        return np.zeros(0, _native.QUALITY_RESULT_DTYPE)
    if pair_sub.size != n or pair_ref.min() < 0 or pair_ref.max() >= ref_len.size or pair_sub.min() < 0 or pair_sub.max() >= sub_len.size:
        raise ValueError("pair index outside the %d references x %d subtitle vectors" % (ref_len.size, sub_len.size))
    if (ref_len <= 0).any() or (sub_len <= 0).any():
        raise empty_error(int(max(ref_len.min(), 0)), int(max(sub_len.min(), 0)))
    combos = np.unique(np.stack([ref_len[pair_ref], sub_len[pair_sub]], axis=1), axis=0)
    max_lags = max(quality.n_lags(int(r), int(s), max_offset_samples) for r, s in combos)
    plan = _get_plan(n, max(max_lags, 1), int(max(ref_len.max(), sub_len.max())), ref_len.size + sub_len.size, pairs_in_flight)
    out = torch.empty(n * _native.QUALITY_RESULT_BYTES, dtype=torch.uint8, device="cuda" if device is None else device)
    plan.report(ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi, pair_ref, pair_sub, max_offset_samples,
                top_k, exclusion_samples, out, code)
    return out.cpu().numpy().view(_native.QUALITY_RESULT_DTYPE)[:n]


def _check_refs(refs) -> list:
    """Host-side checks of the references (ValueError before any device work); host vectors come back as float64."""
    from .subtitle_raster import DeviceRaster

    out = []
    for i, ref in enumerate(refs):
        if isinstance(ref, DeviceRaster):
            if ref.n == 0:
                raise empty_error(0, 1)
            out.append(ref)
            continue
        host = np.asarray(ref, dtype=np.float64).ravel()
        if host.size == 0:
            raise empty_error(0, 1)
        if not np.all(np.isfinite(host)):
            raise ValueError("reference %d: the samples must be finite" % i)
        if np.unique(host).size > 2:
            raise ValueError("match_quality needs two-level references: reference %d is a multi-level float reference, "
                             "which is not supported" % i)
        out.append(host)
    return out


def _reference_lists(refs):
    """The references' boundary lists in one buffer: (uint8 CUDA tensor, byte offsets, lengths, lo, hi, list lengths)."""
    from .subtitle_raster import DeviceRaster

    torch = _native.require_gpu()
    rasters = [ref if isinstance(ref, DeviceRaster) else DeviceRaster.from_host(ref, lists=False) for ref in refs]
    lens = np.array([r.n for r in rasters], dtype=np.int64)
    caps = np.minimum(32768, lens + 2)
    block = (16 + 8 * caps + 63) // 64 * 64
    offs = np.concatenate([[0], np.cumsum(block)[:-1]]).astype(np.int64)
    data = torch.empty(int(block.sum()), dtype=torch.uint8, device="cuda")
    words = [r.packed_words() for r in rasters]  # (kept alive over the call)
    _native.runs_from_bits_batch(np.array([w.data_ptr() for w in words], dtype=np.uint64), lens,
                                 np.uint64(data.data_ptr()) + offs.astype(np.uint64), caps)
    hdr = data.view(torch.int32)[torch.from_numpy(offs // 4).to(data.device)].cpu().numpy()
    dense = np.flatnonzero(hdr >= caps)
    if dense.size:
        raise ValueError("reference %d has %d or more run boundaries: too dense for boundary lists"
                         % (int(dense[0]), int(caps[dense[0]])))
    lo = np.array([r.lo for r in rasters], dtype=np.float64)
    hi = np.array([r.hi for r in rasters], dtype=np.float64)
    return data, offs, lens, lo, hi, np.maximum(hdr, 2).astype(np.int32)


def match_quality(refs, tracks, pairs=None, max_offset_seconds: float = 60, ratios: Optional[Sequence[float]] = None,
                  top_k: int = quality.DEFAULT_TOP_K, exclusion_samples: int = quality.DEFAULT_EXCLUSION_SAMPLES,
                  algorithm: str = "auto", sample_rate: int = SAMPLE_RATE, raw: bool = False,
                  block_pairs: int = DEFAULT_BLOCK_PAIRS) -> MatchMatrix:
    """The quality matrix of N references against M subtitle tracks.  ``refs``: as ``split_align.split_sync`` takes them
    (two-level host vectors or ``subtitle_raster.DeviceRaster``); ``tracks``: (start_us, end_us, is_metadata) triples
    (``subtitle_raster.subtitle_records``); ``pairs``: the (reference, track) index pairs to evaluate (None: all N x M).
    Per pair: the seven-ratio solve's winner (``ratio_index``, ``offset``, ``score``) and the psr / margin / flags of its
    correlation curve over the same lag window; with ``raw`` the device records too.  A pair for which no ratio lands
    inside the window gets ``ratio_index`` -1 and is never trusted.  Large matrices go through the device a block of
    reference rows (about ``block_pairs`` pairs) at a time."""
    from . import batch as batch_mod

    w = int(round(max_offset_seconds * sample_rate))
    quality.validate_args(w, top_k, exclusion_samples)
    _native.match_algorithm_code(algorithm)
    ratios = [float(r) for r in (candidate_ratios() if ratios is None else ratios)]
    if not ratios:
        raise ValueError("need at least one framerate ratio")
    refs, tracks = _check_refs(refs), list(tracks)
    n_ref, n_sub, n_rat = len(refs), len(tracks), len(ratios)
    want = validate_pairs(pairs, n_ref, n_sub)
    out = empty_matrix(n_ref, n_sub, ratios, raw)
    if want.shape[0] == 0:
        return out
    for j, t in enumerate(tracks):
        if len(t[0]) == 0:
            raise empty_error(1, 0)
    torch = _native.require_gpu()
    r_data, r_offs, r_lens, r_lo, r_hi, r_bound = _reference_lists(refs)
    track_of = np.repeat(np.arange(n_sub), n_rat)
    ratio = np.tile(np.array(ratios), n_sub)
    t_data, t_offs, t_lens, t_bound = batch_mod.TrackSet(tracks).rasterize_runs(track_of, ratio, sample_rate)
    data = torch.cat([r_data, t_data])  # one buffer behind every row of the batch: vectors are copied once, never per pair
    t_offs = t_offs.reshape(n_sub, n_rat) + r_data.numel()
    t_lens, t_bound = t_lens.reshape(n_sub, n_rat), t_bound.reshape(n_sub, n_rat)
    t_hi = np.minimum(1.0 / ratio, 1.0).reshape(n_sub, n_rat)
    base = np.uint64(data.data_ptr())
    # whole reference rows per block
    order = np.argsort(want[:, 0], kind="stable")
    want = want[order]
    row_start = np.searchsorted(want[:, 0], np.arange(n_ref + 1))
    lo_row = 0
    while lo_row < n_ref:
        hi_row = lo_row + 1
        while hi_row < n_ref and row_start[hi_row + 1] - row_start[lo_row] <= block_pairs:
            hi_row += 1
        blk = want[row_start[lo_row]:row_start[hi_row]]
        lo_row = hi_row
        if blk.shape[0] == 0:
            continue
        bi, bj = blk[:, 0], blk[:, 1]
        col = lambda ref_col, track_cols: np.ascontiguousarray(np.concatenate([ref_col[bi][:, None], track_cols[bj]], axis=1))
        db = batch_mod.DeviceBatch(data, col(r_offs, t_offs), col(r_lens, t_lens), col(r_lo, np.zeros_like(t_hi)),
                                   col(r_hi, t_hi), _native.FFS_DTYPE_RUNS, None, col(r_bound, t_bound).astype(np.int32))
        combos = np.unique(np.stack([np.repeat(db.lens[:, 0], n_rat), db.lens[:, 1:].ravel()], axis=1), axis=0)
        n_fft = max(_native.plan_length(int(r), int(s), w) for r, s in combos)
        al = batch_mod.BatchAligner(n_fft, n_rat, w, pairs_in_flight=batch_mod.pairs_in_flight_for(blk.shape[0], 64))
        try:
            _, pres = al.solve(db)
        finally:
            al.close()
        best = pres["best_cand"].astype(np.int64)
        hit = best >= 0
        if not hit.any():
            continue
        bi, bj, best, pres = bi[hit], bj[hit], best[hit], pres[hit]
        # the report's tables: this block's references, and the winning (track, ratio) vectors, each once
        refs_used, pr = np.unique(bi, return_inverse=True)
        subs_used, ps = np.unique(bj * n_rat + best, return_inverse=True)
        sj, sk = subs_used // n_rat, subs_used % n_rat
        recs = quality_from_lists(base + r_offs[refs_used].astype(np.uint64), r_lens[refs_used], r_lo[refs_used], r_hi[refs_used],
                                  base + t_offs[sj, sk].astype(np.uint64), t_lens[sj, sk], np.zeros(sj.size), t_hi[sj, sk],
                                  pr, ps, w, top_k, exclusion_samples, algorithm, device=data.device)
        psr, margin, flags = derive(recs)
        out.ratio_index[bi, bj] = best
        out.offset[bi, bj] = pres["offset"]
        out.score[bi, bj] = pres["score"]
        out.psr[bi, bj], out.margin[bi, bj], out.flags[bi, bj] = psr, margin, flags
        if raw:
            out.records[bi, bj] = recs
    return out


def match_library(refs, tracks, pairs=None, max_offset_seconds: float = 60, ratios: Optional[Sequence[float]] = None,
                  top_k: int = quality.DEFAULT_TOP_K, exclusion_samples: int = quality.DEFAULT_EXCLUSION_SAMPLES,
                  algorithm: str = "auto", min_psr: float = quality.DEFAULT_MIN_PSR,
                  min_margin: float = quality.DEFAULT_MIN_MARGIN, exclusive: bool = False,
                  sample_rate: int = SAMPLE_RATE, raw: bool = False) -> LibraryMatch:
    """``match_quality`` + ``assign``, and per assigned subtitle its video, framerate ratio and offset -- the caller need
    not solve again."""
    m = match_quality(refs, tracks, pairs, max_offset_seconds, ratios, top_k, exclusion_samples, algorithm, sample_rate, raw)
    a = assign(m, min_psr, min_margin, exclusive)
    rows = []
    for j, i in enumerate(a.reference):
        if i is None:
            continue
        k = int(m.ratio_index[i, j])
        rows.append(dict(subtitle=j, reference=i, ratio_index=k, ratio=m.ratios[k], offset=int(m.offset[i, j]),
                         score=float(m.score[i, j]), psr=float(m.psr[i, j]), margin=float(m.margin[i, j])))
    return LibraryMatch(m, a, rows)
