"""Split-aware alignment: piecewise subtitle offsets for videos with breaks or cuts.

The reference (and ``FFTAligner`` here) finds ONE offset per file; its README names mid-video splits -- an ad break, a
recap, a scene cut the subtitles do not share -- as its one algorithmic limitation.  This module finds a
piecewise-constant offset instead: the subtitle vector is cut into blocks of ``block_samples`` samples, every block is
scored at every lag of the window (exact integer correlation on the device, ``csrc/ffs_split.h``), and a dynamic
programme picks one lag per block, paying ``split_penalty`` for every change of lag.  With an infinite penalty the
answer is the windowed argmax of the whole-vector correlation (``FFTAligner(max_offset_samples)``).

Upstream has no equivalent, so parity here is against the in-repo numpy model (``tests/split_model.py``), bit for bit.
The drop-in classes and every existing entry point are unchanged; nothing here is reachable from the reference CLI.
"""
import math
from dataclasses import dataclass, field
from datetime import timedelta
from typing import List, Optional, Sequence

import numpy as np

from . import _native
from .constants import SAMPLE_RATE, candidate_ratios
from .side_call import BlockCall, check_two_level_batch, empty_error, pairs_for_budget

DEFAULT_BLOCK_SAMPLES = 1024  # 10.24 s at 100 Hz
DEFAULT_SPLIT_PENALTY = 8192.0  # no spurious pieces above 4 000 in the CPU model; kept after the GPU tests
MAX_LAGS = 262144


@dataclass
class Piece:
    """A maximal run of blocks [first_block, end_block) that share one offset."""

    first_block: int
    end_block: int
    start_sample: int  # subtitle samples [start_sample, end_sample)
    end_sample: int
    offset: int  # samples: the subtitle moves by +offset / sample_rate seconds
    score: float  # sum of the blocks' scores at `offset`, in block order from 0.0


@dataclass
class SplitResult:
    pieces: List[Piece]
    total: float  # the DP's maximum: sum of the block scores minus P per split
    block_offsets: np.ndarray  # int32 [B]
    block_scores: np.ndarray  # float64 [B]


@dataclass
class SplitSyncResult:
    ratio: float  # framerate ratio picked by the seven-ratio solve
    ratio_index: int
    global_offset: int  # that solve's single offset (samples)
    pieces: List[Piece]
    total: float
    cue_start_us: np.ndarray  # output cue times (int64 microseconds): scaled, then shifted by the cue's piece
    cue_end_us: np.ndarray
    cue_piece: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))


def validate_block_samples(block_samples) -> None:
    """The block size check that every split entry point makes (ValueError)."""
    k = int(block_samples)
    if k != block_samples or k % 32 or not 256 <= k <= 32768:
        raise ValueError("block_samples=%r: need a multiple of 32 in [256, 32768]" % (block_samples,))


def validate_args(block_samples, max_offset_samples, split_penalty) -> None:
    """Host-side checks of the call parameters (ValueError before any native call)."""
    validate_block_samples(block_samples)
    w = int(max_offset_samples)
    if w != max_offset_samples or w < 1 or 2 * w > MAX_LAGS:
        raise ValueError("max_offset_samples=%r: need an integer W >= 1 with 2W <= %d" % (max_offset_samples, MAX_LAGS))
    p = float(split_penalty)
    if math.isnan(p) or p < 0:
        raise ValueError("split_penalty=%r: need a number >= 0 (inf = never split)" % (split_penalty,))


def pieces_from_blocks(block_offsets, block_scores, block_samples: int, sub_len: int) -> List[Piece]:
    """Maximal runs of equal block offsets, with their sample ranges and scores (summed in block order from 0.0)."""
    offs = np.asarray(block_offsets)
    out: List[Piece] = []
    b0 = 0
    for b in range(1, offs.size + 1):
        if b == offs.size or offs[b] != offs[b0]:
            score = 0.0
            for x in block_scores[b0:b]:
                score += float(x)
            out.append(Piece(b0, b, b0 * block_samples, min(b * block_samples, sub_len), int(offs[b0]), score))
            b0 = b
    return out


def _check_batch(batch) -> None:
    """The batch check of every block-wise entry point, in ``split_align_batch``'s words."""
    check_two_level_batch(batch, "split_align_batch")


_plans = _native.SidePlanCache(_native.SplitPlan)


def _get_plan(n_pairs: int, max_blocks: int, max_lags: int, max_samples: int, pairs_in_flight: Optional[int],
              report: bool = False):
    """The cached plan of this device; report calls (``split_report``) get their own, sized for the per-piece n11 rows
    the first report call adds (4 more bytes per block and lag)."""
    if pairs_in_flight is None:  # bound the workspace (~170 MB of counts per pair at 2 h, +-10 min, K = 1024) to ~12 GiB
        per_pair = max_blocks * (max_lags + 64) * (6.2 if report else 2.2) + 1
        pairs_in_flight = pairs_for_budget(n_pairs, per_pair)
    return _plans.get(pairs_in_flight, max_blocks, max_lags, max_samples, role="report" if report else None)


def clear_plan_cache() -> None:
    _plans.clear()


def split_align_batch(batch, max_offset_samples: int, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                      split_penalty: float = DEFAULT_SPLIT_PENALTY, pairs_in_flight: Optional[int] = None) -> List[SplitResult]:
    """Piecewise offsets of every pair of a ``batch.DeviceBatch`` with ONE candidate per pair
    (``DeviceBatch.select_candidates``): bit-packed vectors are read as they are, 0/1 bytes through ``to_bits()``; any
    other element type is rejected.  Lags d in [-W+1, W] with W = ``max_offset_samples``; ``split_penalty`` = inf never
    splits.  Returns one ``SplitResult`` per pair."""
    validate_args(block_samples, max_offset_samples, split_penalty)
    _check_batch(batch)
    return _solve(batch, max_offset_samples, block_samples, split_penalty, pairs_in_flight)[0]


def _solve(batch, max_offset_samples, block_samples, split_penalty, pairs_in_flight, report=None):
    """The device call behind ``split_align_batch`` (arguments checked); with ``report`` = (top_k, exclusion_samples)
    ``ffs_align_split_report_batch``.  Returns (SplitResults, piece report records [n, max_b] or None, piece counts or
    None)."""
    call = BlockCall(batch, block_samples)
    w = int(max_offset_samples)
    plan = _get_plan(call.n, call.max_b, 2 * w, int(call.sub_len.max()), pairs_in_flight, report is not None)
    outs = split_outputs(call.n, call.max_b, call.dev)
    args = call.pair_arrays() + (call.k, w, float(split_penalty))
    recs = counts = None
    if report is None:
        plan.align(*args, *outs)
    else:
        rep_out, n_out = call.records(_native.PIECE_REPORT_DTYPE), call.per_pair(np.int32)
        plan.align_report(*args, int(report[0]), int(report[1]), *outs, rep_out, n_out)
        recs, counts = call.read_records(rep_out, _native.PIECE_REPORT_DTYPE), n_out.cpu().numpy()
    return split_results(outs, call.n_blocks, call.k, call.sub_len), recs, counts


def split_outputs(n_pairs: int, max_b: int, device):
    """The device outputs of a split call: block offsets, block scores (n_pairs * max_b each) and totals (n_pairs)."""
    torch = _native.require_gpu()
    return (torch.empty(n_pairs * max_b, dtype=torch.int32, device=device),
            torch.empty(n_pairs * max_b, dtype=torch.float64, device=device),
            torch.empty(n_pairs, dtype=torch.float64, device=device))


def split_results(outs, n_blocks, block_samples: int, sub_len) -> List[SplitResult]:
    """One ``SplitResult`` per pair from the outputs of ``split_outputs`` after the call."""
    n, max_b = len(n_blocks), int(max(n_blocks))
    offs_h = outs[0].cpu().numpy().reshape(n, max_b)
    scores_h = outs[1].cpu().numpy().reshape(n, max_b)
    totals_h = outs[2].cpu().numpy()
    out = []
    for p in range(n):
        nb = int(n_blocks[p])
        bo, bs = offs_h[p, :nb].copy(), scores_h[p, :nb].copy()
        out.append(SplitResult(pieces_from_blocks(bo, bs, block_samples, int(sub_len[p])), float(totals_h[p]), bo, bs))
    return out


def _scaled_us(us: int, ratio: float) -> int:
    """SubtitleScaler (subtitle_transformers.py:35-47): timedelta(seconds=total_seconds * ratio), in microseconds."""
    td = timedelta(seconds=timedelta(microseconds=int(us)).total_seconds() * ratio)
    return (td.days * 86400 + td.seconds) * 10 ** 6 + td.microseconds


def map_cues(start_us, end_us, ratio: float, pieces: Sequence[Piece], sample_rate: int = SAMPLE_RATE):
    """Output times of every cue: scaled by ``ratio``, then shifted by the offset of the piece that holds its scaled
    start sample (the rasteriser's rounding, int(round(t * sample_rate)); clamped to the first and last piece) -- what
    try_sync writes (scale, then shift by offset / sample_rate s) when there is one piece.  Returns (start_us, end_us,
    piece index) int64 arrays."""
    if not pieces:
        raise ValueError("no pieces")
    starts = np.array([p.start_sample for p in pieces], dtype=np.int64)
    n = len(start_us)
    out_s, out_e, which = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        s_us, e_us = _scaled_us(start_us[i], ratio), _scaled_us(end_us[i], ratio)
        sample = int(round(timedelta(microseconds=s_us).total_seconds() * sample_rate))
        k = int(np.searchsorted(starts, sample, side="right")) - 1
        k = min(max(k, 0), len(pieces) - 1)
        shift = timedelta(seconds=pieces[k].offset / float(sample_rate))
        out_s[i] = _td_us(timedelta(microseconds=s_us) + shift)
        out_e[i] = _td_us(timedelta(microseconds=e_us) + shift)
        which[i] = k
    return out_s, out_e, which


def _td_us(td: timedelta) -> int:
    return (td.days * 86400 + td.seconds) * 10 ** 6 + td.microseconds


def split_sync(problems, max_offset_seconds: float = 600, block_samples: int = DEFAULT_BLOCK_SAMPLES,
               split_penalty: float = DEFAULT_SPLIT_PENALTY, sample_rate: int = SAMPLE_RATE,
               ratios: Optional[Sequence[float]] = None) -> List[SplitSyncResult]:
    """Split-aware sync of many files.  ``problems``: list of (reference, track), the reference a two-level host vector
    or a ``subtitle_raster.DeviceRaster``, the track the (start_us, end_us, is_metadata) triple of
    ``subtitle_raster.subtitle_records``.  Per problem: the framerate ratio from the existing seven-ratio batch solve over
    the same lag window, the winner rasterised on the device, the split DP, and every cue's output time."""
    w = int(round(max_offset_seconds * sample_rate))
    validate_args(block_samples, w, split_penalty)
    ratios = list(candidate_ratios() if ratios is None else ratios)
    db, best, pres = solve_ratios(problems, w, ratios, sample_rate)
    results = split_align_batch(db.select_candidates(best), w, block_samples, split_penalty)
    out = []
    for p, ((_, (start_us, end_us, _meta)), res) in enumerate(zip(problems, results)):
        ratio = ratios[int(best[p])]
        cs, ce, which = map_cues(start_us, end_us, ratio, res.pieces, sample_rate)
        out.append(SplitSyncResult(ratio, int(best[p]), int(pres[p]["offset"]), res.pieces, res.total, cs, ce, which))
    return out


def solve_ratios(problems, max_offset_samples: int, ratios: Sequence[float], sample_rate: int = SAMPLE_RATE):
    """The existing seven-ratio batch solve of (reference, track) problems (see ``split_sync``): every track rasterised on
    the device at each ratio, one ``BatchAligner`` solve over the lag window.  Returns (DeviceBatch, winning candidate
    index per problem, the solve's ffs_pair_result records)."""
    from . import batch as batch_mod
    from .subtitle_raster import DeviceRaster, rasterize_candidates

    w = int(max_offset_samples)
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
    pairs = []
    for ref, (start_us, end_us, meta) in zip(refs, (p[1] for p in problems)):
        pairs.append((ref, rasterize_candidates(start_us, end_us, meta, ratios, sample_rate)))
    db = batch_mod.pack_pairs(pairs)
    al = batch_mod.BatchAligner(db.required_fft_length(w), len(ratios), w, pairs_in_flight=min(len(pairs), 64))
    try:
        _, pres = al.solve(db)
    finally:
        al.close()
    best = pres["best_cand"].astype(np.int64)
    if (best < 0).any():
        raise RuntimeError("no framerate ratio found an offset inside the window")
    return db, best, pres
