"""Half-sample stability: an offset interval for every sync.

``surrogate.py`` answers "is this subtitle related to this audio at all"; a subtitle 3 s off inside the window is as
significant to it as one in place.  This module asks how precisely the offset is known, and whether the peak that won
would still win on a different half of the cues -- again with no tuned score threshold.  K HALF-SAMPLES of the subtitle,
each keeping a hashed half of its cue blocks with every position untouched, are solved beside the real one.  If the sync
is real every half peaks at the same lag and the spread of the K offsets is an interval for the offset; if the peak is a
chance maximum the halves peak all over the window.  K + 1 single-ratio solves a file are nothing on the run-boundary
path.

    subsample_lists       ``ffs_subsample_lists``: K thinned boundary lists per device-resident list, no host round trip
    offset_stats          ``ffs_offset_stats``: the K + 1 solve records of every file reduced on the device to one record
    stability_test_lists  both around ``align_batch(n * (K + 1), 1, RUNS, ...)`` for device-resident lists on both sides
    stable_sync           the seven-ratio solve of many files, the half-samples at the winning ratio, the interval

A half-sample cuts ALL runs of the list into blocks of ``block_runs`` consecutive runs and keeps block b iff bit 31 of
the surrogate hash of (seed, s >> 1, b), flipped for odd s, is set: half-samples 2j and 2j + 1 are complementary.
Seeds: file i of a call uses ``surrogate.file_seed(seed, i)`` unless the caller passes ``seeds``.

What it says and what it does not.  The interval is the central 90 % of the half-sample offsets (``off_lo``, ``off_hi``);
``max_dev`` and ``n_within`` count against the full solve's offset.  The defaults come from SYNTHETIC data only
(profiles/stability_calibration.json); nobody has measured real files.  By the rule of DESIGN 3.25 the calibration ships
NO default verdict: one half-sample in 64 of a matched ten-minute file with 8 to 10 blocks keeps next to nothing and peaks
anywhere, so the largest matched ``max_dev`` is 8182 samples, ``DEFAULT_TOL`` = twice that covers the whole window and
the classes do not separate at it (``DEFAULT_MIN_SHARE`` is None: ``stable`` is None unless the caller passes ``tol`` and
``min_share``).  The interval separates the classes in every cell (matched at most 5 samples wide, wrong at least 5203).
Parity is against the in-repo numpy model ``tests/stability_model.py``.  Nothing here changes an existing entry point;
nothing is reachable from the reference CLI.
"""
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from .constants import SAMPLE_RATE, candidate_ratios
from .side_call import pairs_for_budget
from .surrogate import CHUNK_BUDGET, CHUNK_CAP, _check_lists, _check_seed, _list_vector, _winning_lists, file_seed, fmix32  # noqa: F401

# By the rules of DESIGN 3.25 on the CPU model (profiles/stability_calibration.json; synthetic data, 10 min and 1 h, 32 + 32
# files each, block_runs 1 and 8): twice the largest matched max_dev (8182: block_runs 8 at 10 min, a half-sample that kept
# next to nothing), and no share threshold, because matched (1.0) and wrong (1.0) do not separate at that tol
DEFAULT_TOL = 16364
DEFAULT_MIN_SHARE = None
DEFAULT_SUBSAMPLES = 64
MAX_SUBSAMPLES = _native.STAB_MAX_K
MAX_BLOCK_RUNS = _native.STAB_MAX_BLOCK_RUNS
MAX_BOUND = (1 << 28) - 2  # boundaries of a list whose block of n + 1 entries the ABI takes
MIN_BLOCKS = 8  # fewer blocks: a half-sample keeps none or one of them too often


@dataclass
class StabilityTest:
    records: np.ndarray  # one _native.STABILITY_RESULT_DTYPE record per file (host; with ``raw`` the uint8 CUDA tensor)
    table: "object"  # uint8 CUDA tensor: n * (K + 1) ffs_cand_result records, per file the real solve first
    status: np.ndarray  # int32 per file: _native.SUB_BAD_* bits of its subtitle list (0 = fine; with ``raw`` a CUDA tensor)
    seeds: np.ndarray  # uint32 per file
    stats: dict

    def solves(self) -> np.ndarray:
        """The solve records on the host: a [n, K + 1] ``_native.CAND_RESULT_DTYPE`` array (reads the table back)."""
        n = self.seeds.size
        return self.table.cpu().numpy().view(_native.CAND_RESULT_DTYPE)[:n * (self.stats["n_subsamples"] + 1)].reshape(n, -1)


@dataclass
class StabilityRecord:
    real_score: float
    real_offset: int
    off_min: int
    off_max: int
    off_median: int
    off_lo: int  # the central 90 % of the usable half-sample offsets
    off_hi: int
    max_dev: int  # max |offset - real_offset|
    max_pair_gap: int  # max |offset(2j) - offset(2j + 1)|
    pair_score_min: float
    n_sub: int  # usable half-sample records
    n_within: int  # of them with |offset - real_offset| <= tol
    n_pairs: int
    n_pairs_within: int
    tol: int
    flags: int  # _native.STAB_EMPTY / STAB_AMBIGUOUS / STAB_NO_PAIRS


@dataclass
class StableSyncResult:
    ratio: float
    ratio_index: int
    offset: int  # samples, at that ratio
    score: float
    record: StabilityRecord
    interval_samples: Tuple[int, int]  # (off_lo, off_hi)
    interval_seconds: Tuple[float, float]
    share_within: float  # n_within / n_sub
    blocks: int  # blocks the half-samples drew from
    stable: Optional[bool]  # not EMPTY and share_within >= min_share; None without a min_share
    reasons: List[str]


def n_blocks(n_boundaries: int, block_runs: int) -> int:
    """Blocks of a list with ``n_boundaries`` entries: ceil((n / 2) / block_runs)."""
    return (int(n_boundaries) // 2 + int(block_runs) - 1) // int(block_runs)


def _check_resample(n_subsamples, block_runs) -> None:
    k, b = int(n_subsamples), int(block_runs)
    if k != n_subsamples or not 1 <= k <= MAX_SUBSAMPLES:
        raise ValueError("n_subsamples=%r: need an integer in [1, %d]" % (n_subsamples, MAX_SUBSAMPLES))
    if b != block_runs or not 1 <= b <= MAX_BLOCK_RUNS:
        raise ValueError("block_runs=%r: need an integer in [1, %d]" % (block_runs, MAX_BLOCK_RUNS))


def _check_tol(tol) -> int:
    if int(tol) != tol or tol < 0:
        raise ValueError("tol=%r: need an integer >= 0" % (tol,))
    return int(tol)


def subsample_lists(list_ptr, n_bound, lens, seeds, n_subsamples: int = DEFAULT_SUBSAMPLES, block_runs: int = 1, raw: bool = False):
    """``ffs_subsample_lists`` on the current stream.  Per vector: the device pointer of its ``ffs_runs_list``, a
    host-known bound of its length (``vec_max_boundaries``' convention), its length in samples and its uint32 seed.
    Returns (uint8 CUDA buffer, int64 [n, K] byte offsets of every half-sample's list block, status: ``_native.SUB_BAD_*``
    bits per vector -- all half-samples of a list whose header breaks the contract are empty lists).  Every block holds
    ``n_bound + 1`` entries.  With ``raw`` the status is the int32 CUDA tensor and nothing is waited for or read back;
    otherwise it is read back to a host array."""
    _check_resample(n_subsamples, block_runs)
    ptr, n_bound, lens = _check_lists("subsample_lists", list_ptr, n_bound, lens)
    seeds = np.ascontiguousarray(seeds, dtype=np.int64).ravel()
    if seeds.size != ptr.size or (seeds < 0).any() or (seeds > 0xFFFFFFFF).any():
        raise ValueError("subsample_lists: need one seed in [0, 2^32) per vector")
    if (n_bound > MAX_BOUND).any():
        raise ValueError("subsample_lists: a list of up to %d boundaries is above what a list block holds (%d)"
                         % (int(n_bound.max()), MAX_BOUND))
    torch = _native.require_gpu()
    k = int(n_subsamples)
    caps = n_bound + 1
    block = 16 + 8 * caps
    first = np.zeros(ptr.size, dtype=np.int64)
    if ptr.size:
        np.cumsum((block * k)[:-1], out=first[1:])
    total = int((block * k).sum())
    out = torch.empty(max(total, 8), dtype=torch.uint8, device="cuda")
    status = torch.empty(max(ptr.size, 1), dtype=torch.int32, device="cuda")
    _native.subsample_lists(ptr, n_bound, seeds, first, caps, k, int(block_runs), out, status)
    status = status[:ptr.size]
    return out, first[:, None] + block[:, None] * np.arange(k, dtype=np.int64)[None, :], status if raw else status.cpu().numpy()


def offset_stats(table, n_files: int, n_subsamples: int, tol: int = DEFAULT_TOL, raw: bool = False):
    """``ffs_offset_stats``: ``table`` a CUDA tensor of n_files * (n_subsamples + 1) ffs_cand_result records, per file the
    real list's solve first.  Returns one ``_native.STABILITY_RESULT_DTYPE`` record per file (a host array); with ``raw``
    the uint8 CUDA tensor that holds them."""
    k = int(n_subsamples)
    if k != n_subsamples or not 1 <= k <= MAX_SUBSAMPLES:
        raise ValueError("n_subsamples=%r: need an integer in [1, %d]" % (n_subsamples, MAX_SUBSAMPLES))
    if int(n_files) != n_files or n_files < 0:
        raise ValueError("n_files=%r: need an integer >= 0" % (n_files,))
    out = _native.offset_stats(table, int(n_files), k, _check_tol(tol))
    if raw:
        return out
    return out.cpu().numpy().view(_native.STABILITY_RESULT_DTYPE)[:int(n_files)]


def _levels(values, n, default):
    if values is None:
        return np.full(n, default, dtype=np.float64)
    values = np.ascontiguousarray(values, dtype=np.float64).ravel()
    if values.size != n or not np.all(np.isfinite(values)):
        raise ValueError("stability_test_lists: need one finite level per file")
    return values


def _careful(ref, sub, seed, k, block_runs, w) -> np.ndarray:
    """The K + 1 records of one file through the drop-in's ``solve_pairs`` (ambiguity handling), as ``surrogate._careful``
    redoes a file: ``ref`` / ``sub`` = (list pointer, bound, length, lo, hi)."""
    from .aligners import _Vec, solve_pairs

    buf, offs, _ = subsample_lists([sub[0]], [sub[1]], [sub[2]], [seed], k, block_runs, raw=True)
    ref_vec = _Vec(_list_vector(ref[0], ref[2], ref[3], ref[4]))
    ptrs = [int(sub[0])] + [buf.data_ptr() + int(o) for o in offs[0]]
    pairs = [(ref_vec, [_Vec(_list_vector(p, sub[2], sub[3], sub[4]))]) for p in ptrs]
    cres, _ = solve_pairs(pairs, w)
    return np.ascontiguousarray(cres[:, 0])


def stability_test_lists(ref_ptr, ref_len, ref_bound, sub_ptr, sub_len, sub_bound, max_offset_samples: int,
                         n_subsamples: int = DEFAULT_SUBSAMPLES, block_runs: int = 1, seed: int = 0, tol: int = DEFAULT_TOL,
                         ref_lo=None, ref_hi=None, sub_lo=None, sub_hi=None, seeds=None, budget_bytes: int = CHUNK_BUDGET,
                         raw: bool = False) -> StabilityTest:
    """The half-sample offsets of n files whose vectors are device-resident boundary lists on both sides.  Per file: the
    device pointer, length in samples and host-known list bound of its reference and of its subtitle list (and their
    levels: 0 / 1 by default; a track rasterised at ratio r has ``sub_hi`` = min(1 / r, 1)).

    Per chunk of files -- as many as ``budget_bytes`` of half-sample blocks hold -- one ``ffs_subsample_lists`` call and ONE
    ``align_batch(files * (K + 1), 1, RUNS, ...)``: every pair of a file points at the same reference list, pair 0 at
    the real list, pair 1 + s at half-sample s; the bounds travel as ``vec_max_boundaries``, so nothing waits.  The table
    is reduced by ``ffs_offset_stats`` and one record per file comes back (with the lists' status).  A file whose records
    carry ``FFS_FLAG_AMBIGUOUS`` is redone on the careful per-file path, as ``surrogate.null_test_lists`` redoes it.

    With ``raw`` everything is queued on the current stream and nothing is read back: ``records`` and ``status`` of the
    result are the CUDA tensors (uint8 records, int32 status) and no file is redone -- the caller looks at
    ``STAB_AMBIGUOUS`` itself."""
    _check_resample(n_subsamples, block_runs)
    seed = _check_seed(seed)
    tol = _check_tol(tol)
    w = int(max_offset_samples)
    if w != max_offset_samples or w < 1:
        raise ValueError("max_offset_samples=%r: need a window of at least one sample" % (max_offset_samples,))
    if int(budget_bytes) < 1:
        raise ValueError("budget_bytes=%r: need a positive number of bytes" % (budget_bytes,))
    ref_ptr, ref_bound, ref_len = _check_lists("stability_test_lists (references)", ref_ptr, ref_bound, ref_len)
    sub_ptr, sub_bound, sub_len = _check_lists("stability_test_lists (subtitles)", sub_ptr, sub_bound, sub_len)
    n = sub_ptr.size
    if ref_ptr.size != n:
        raise ValueError("stability_test_lists: %d references for %d subtitle lists" % (ref_ptr.size, n))
    if (sub_bound > MAX_BOUND).any():
        raise ValueError("stability_test_lists: a subtitle list of up to %d boundaries is above what a list block holds (%d)"
                         % (int(sub_bound.max()), MAX_BOUND))
    if (ref_bound >= 32768).any():
        raise ValueError("stability_test_lists: a reference of %d or more run boundaries is too dense for a list" % 32768)
    ref_lo, ref_hi = _levels(ref_lo, n, 0.0), _levels(ref_hi, n, 1.0)
    sub_lo, sub_hi = _levels(sub_lo, n, 0.0), _levels(sub_hi, n, 1.0)
    if seeds is None:
        seeds = np.array([file_seed(seed, i) for i in range(n)], dtype=np.int64)
    else:
        seeds = np.ascontiguousarray(seeds, dtype=np.int64).ravel()
        if seeds.size != n or (seeds < 0).any() or (seeds > 0xFFFFFFFF).any():
            raise ValueError("stability_test_lists: need one seed in [0, 2^32) per file")
    torch = _native.require_gpu()
    k = int(n_subsamples)
    stats = {"files": n, "n_subsamples": k, "block_runs": int(block_runs), "chunks": 0, "careful_files": 0}
    table = torch.empty(max(n * (k + 1), 1) * 24, dtype=torch.uint8, device="cuda")
    if n == 0:
        return StabilityTest(np.zeros(0, _native.STABILITY_RESULT_DTYPE), table, np.zeros(0, np.int32), seeds.astype(np.uint32),
                             stats)
    per_file = k * (16 + 8 * (int(sub_bound.max()) + 1))
    chunk = pairs_for_budget(n, per_file, cap=max(CHUNK_CAP // (k + 1), 1), budget=int(budget_bytes))
    n_fft = max(_native.plan_length(int(r), int(s), w) for r, s in zip(ref_len, sub_len))
    if n_fft > _native.MAX_FFT_LENGTH:
        raise ValueError("inputs too long for the device transform (N=%d > 2^24)" % n_fft)
    plan = _native.get_plan(n_fft, pairs_in_flight=min(chunk * (k + 1), 512), max_cand=1)
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    pair_out = torch.empty(chunk * (k + 1) * 24, dtype=torch.uint8, device="cuda")
    runs = (_native.FFS_DTYPE_RUNS, _native.FFS_DTYPE_RUNS)
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        m = (b - a) * (k + 1)
        buf, offs, st = subsample_lists(sub_ptr[a:b], sub_bound[a:b], sub_len[a:b], seeds[a:b], k, block_runs, raw=True)
        status[a:b] = st
        cand = np.empty((b - a, k + 1), dtype=np.uint64)
        cand[:, 0] = sub_ptr[a:b]
        cand[:, 1:] = np.uint64(buf.data_ptr()) + offs.astype(np.uint64)
        rep = lambda x: np.repeat(x[a:b], k + 1)
        ptrs, lens = np.empty(2 * m, np.uint64), np.empty(2 * m, np.int64)
        lo, hi, bounds = np.empty(2 * m), np.empty(2 * m), np.empty(2 * m, np.int32)
        ptrs[0::2], lens[0::2], lo[0::2], hi[0::2], bounds[0::2] = rep(ref_ptr), rep(ref_len), rep(ref_lo), rep(ref_hi), np.maximum(rep(ref_bound), 2)
        ptrs[1::2], lens[1::2], lo[1::2], hi[1::2], bounds[1::2] = cand.ravel(), rep(sub_len), rep(sub_lo), rep(sub_hi), np.maximum(rep(sub_bound), 2)
        plan.align_batch(m, 1, runs, ptrs, lens, lo, hi, w, None, table[a * (k + 1) * 24:], pair_out, vec_max_boundaries=bounds)
        stats["chunks"] += 1
        del buf  # (stream-ordered: the allocator hands the block out again only behind the solve)
    out = _native.offset_stats(table, n, k, tol)
    if raw:
        return StabilityTest(out, table, status, seeds.astype(np.uint32), stats)
    records = out.cpu().numpy().view(_native.STABILITY_RESULT_DTYPE)[:n].copy()
    status_h = status.cpu().numpy()
    amb = np.flatnonzero((records["flags"] & _native.STAB_AMBIGUOUS) != 0)
    if amb.size:  # degenerate input (e.g. a silent reference): the careful path, file by file
        for f in amb:
            recs = _careful((ref_ptr[f], ref_bound[f], ref_len[f], ref_lo[f], ref_hi[f]),
                            (sub_ptr[f], sub_bound[f], sub_len[f], sub_lo[f], sub_hi[f]), int(seeds[f]), k, block_runs, w)
            table[f * (k + 1) * 24:(f + 1) * (k + 1) * 24] = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
            stats["careful_files"] += 1
        records = _native.offset_stats(table, n, k, tol).cpu().numpy().view(_native.STABILITY_RESULT_DTYPE)[:n].copy()
    return StabilityTest(records, table, status_h, seeds.astype(np.uint32), stats)


def record_of(rec) -> StabilityRecord:
    """StabilityRecord of one ``_native.STABILITY_RESULT_DTYPE`` record."""
    return StabilityRecord(float(rec["real_score"]), *[int(rec[name]) for name in (
        "real_offset", "off_min", "off_max", "off_median", "off_lo", "off_hi", "max_dev", "max_pair_gap")],
        float(rec["pair_score_min"]), *[int(rec[name]) for name in ("n_sub", "n_within", "n_pairs", "n_pairs_within", "tol", "flags")])


def share_within(record: StabilityRecord) -> float:
    """n_within / n_sub (0 without a usable half-sample)."""
    return record.n_within / record.n_sub if record.n_sub else 0.0


def stable(record: StabilityRecord, min_share: Optional[float] = DEFAULT_MIN_SHARE) -> Optional[bool]:
    """The verdict: a usable record whose half-samples agree with the full solve, ``share_within`` >= ``min_share``.  None
    without a ``min_share``: the calibration ships no default, the interval stands alone."""
    if min_share is None:
        return None
    return not (record.flags & _native.STAB_EMPTY) and share_within(record) >= min_share


def assess(record: StabilityRecord, blocks: int, min_share: Optional[float] = DEFAULT_MIN_SHARE) -> List[str]:
    """What speaks against a result, worded like ``surrogate.assess``."""
    reasons: List[str] = []
    if record.flags & _native.STAB_EMPTY:
        reasons.append("empty record (no usable half-sample solve)")
    elif min_share is not None and share_within(record) < min_share:
        reasons.append("%d of %d half-samples within %d samples of the offset (share %.2f < %.2f; 90 %% interval [%d, %d])"
                       % (record.n_within, record.n_sub, record.tol, share_within(record), min_share, record.off_lo, record.off_hi))
    if blocks < MIN_BLOCKS:
        reasons.append("too few cues to resample (%d blocks < %d)" % (blocks, MIN_BLOCKS))
    return reasons


def _check_sync(problems, max_offset_seconds, ratios, sample_rate, start_seconds, min_share):
    """Host checks of ``stable_sync`` (ValueError before any native call); returns (window in samples, ratios)."""
    from .ratio_sweep import _check_problems

    if start_seconds > 0:
        raise ValueError("stable_sync needs start_seconds <= 0: boundary lists cannot hold the negative start samples of "
                         "start_seconds > 0")
    if min_share is not None and not (math.isfinite(min_share) and 0 <= min_share <= 1):
        raise ValueError("min_share=%r: need a number in [0, 1] (or None: no verdict)" % (min_share,))
    ratios = [float(r) for r in (candidate_ratios() if ratios is None else ratios)]
    if not ratios or not all(math.isfinite(r) and r > 0 for r in ratios):
        raise ValueError("ratios=%r: need at least one finite ratio > 0" % (ratios,))
    return _check_problems(problems, max_offset_seconds, sample_rate, CHUNK_BUDGET), ratios


def stable_sync(problems, max_offset_seconds: float = 60, ratios: Optional[Sequence[float]] = None,
                n_subsamples: int = DEFAULT_SUBSAMPLES, block_runs: int = 1, seed: int = 0, tol: int = DEFAULT_TOL,
                min_share: Optional[float] = DEFAULT_MIN_SHARE, sample_rate: int = SAMPLE_RATE,
                start_seconds: float = 0) -> List[StableSyncResult]:
    """Sync many files and say how precisely every offset is known.  ``problems``: as ``quality.quality_sync`` takes
    them, a list of (reference, track) with the reference a two-level host vector or a ``subtitle_raster.DeviceRaster``
    and the track a (start_us, end_us, is_metadata) triple.  Per problem: the ratio, offset and score of the seven-ratio
    solve (the first maximal candidate), the track rasterised to a boundary list at that ratio (amplitude min(1 / r, 1)),
    its half-samples (``stability_test_lists``; file i resampled with ``file_seed(seed, i)``), the interval
    (off_lo, off_hi) in samples and seconds, ``share_within`` = n_within / n_sub and, with a ``min_share``, the verdict:
    ``stable`` iff the record is not EMPTY and ``share_within`` >= ``min_share``.

    Refused by name before any device work: multi-level float references, ``start_seconds`` > 0, a host reference too
    dense for a boundary list (counted on the host; a reference that is already on the device is refused once its list
    has been counted there)."""
    _check_resample(n_subsamples, block_runs)
    _check_seed(seed)
    _check_tol(tol)
    w, ratios = _check_sync(problems, max_offset_seconds, ratios, sample_rate, start_seconds, min_share)
    if not problems:
        return []
    solver, recs, best, best_ratio, (data, offs, lens, bounds), n_sub = _winning_lists("stable_sync", problems, ratios, w, sample_rate)
    test = stability_test_lists(solver.ref_ptr, solver.ref_len, solver.ref_bound, np.uint64(data.data_ptr()) + offs.astype(np.uint64),
                                lens, bounds, w, n_subsamples, block_runs, seed, tol, solver.ref_lo, solver.ref_hi, None,
                                np.minimum(1.0 / best_ratio, 1.0))
    out = []
    for f in range(len(problems)):
        record = record_of(test.records[f])
        blocks = n_blocks(int(n_sub[f]), block_runs)
        out.append(StableSyncResult(float(best_ratio[f]), int(best[f]), int(recs[f][best[f]]["offset"]),
                                    float(recs[f][best[f]]["score"]), record, (record.off_lo, record.off_hi),
                                    (record.off_lo / float(sample_rate), record.off_hi / float(sample_rate)),
                                    share_within(record), blocks, stable(record, min_share), assess(record, blocks, min_share)))
    return out
