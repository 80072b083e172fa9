"""Progressive alignment: solve while the audio decodes, stop when the answer has settled.

A sync is bound by decoding the audio, not by the solve.  Score counts are additive over the reference, so after every
buffer of reference labels the exact seven-ratio answer on what has been read so far costs one small update on the
device (``csrc/ffs_progressive.h``: the new samples against the subtitle samples they can meet), not a re-solve; the
curve statistics of ``quality.py`` -- and how far the best framerate ratio stands above the others -- say when it has
stopped moving.  ``progressive_sync`` then stops pulling that file's audio.

    ratio_margin = (best ratio's peak - best other ratio's peak) / std of the best ratio's curve

The lag window is d in [-W+1, W] whatever the prefix length (the reference's masked window for a prefix depends on the
prefix through its transform length; wherever that mask is this window, the records here are byte-identical to
``quality.quality_batch``'s and the answer is ``quality.quality_sync``'s).  Parity is against the numpy model
``tests/progressive_model.py``.  Two-level references only, windowed only, appends only; split, cut, drift and sweep
solves are not progressive: run them afterwards on ``ProgressiveSolve.reference(file)``.  The default ``StopRule`` comes
from synthetic data (``profiles/progressive_calibration.json``).  Nothing here changes an existing entry point; nothing
is reachable from the reference CLI.
"""
import math
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np

from . import _native, quality
from .constants import DEFAULT_ENERGY_THRESHOLD_DB, SAMPLE_RATE, candidate_ratios
from .side_call import empty_error

MAX_CANDIDATES = _native.PROG_MAX_CAND
DEFAULT_MAX_REFERENCE_SECONDS = 3 * 3600.0
DEFAULT_OFFSET_TOLERANCE = 2  # samples: the offset_tol of workloads/splits.check_recovery
# Chosen by rule on the CPU model (profiles/progressive_calibration.json): of the (stable_updates,
# min_ratio_margin) cells without a wrong stop, the one that reads least, moved one step to the safe side on both axes.
# (None would mean that no cell was free of wrong stops: a default rule that never settles.)  Best cell: k = 4, m = 0.
DEFAULT_STABLE_UPDATES: Optional[int] = 5
DEFAULT_MIN_RATIO_MARGIN = 0.05


@dataclass
class ProgressState:
    """One file after one append (``ffs_prog_state`` plus the host derivation)."""
    ref_len: int  # reference samples consumed
    best_cand: int  # index into the solve's ratios
    offset: int
    score: float
    quality: quality.AlignmentQuality  # of the best candidate's curve over the window
    ratio_margin: float  # (score - other_best) / std; NaN with one candidate; 0 on a flat curve
    other_best: float  # the largest peak score among the other candidates (NaN with one candidate)


@dataclass
class StopRule:
    """When a file's answer counts as settled: the last ``stable_updates`` states all name the same candidate, have
    offsets within ``offset_tolerance`` samples of the newest, each pass the three thresholds, and have consumed at
    least ``min_seconds`` of reference.  ``stable_updates=None`` never settles."""
    min_psr: float = quality.DEFAULT_MIN_PSR
    min_margin: float = quality.DEFAULT_MIN_MARGIN
    min_ratio_margin: float = DEFAULT_MIN_RATIO_MARGIN
    stable_updates: Optional[int] = DEFAULT_STABLE_UPDATES
    offset_tolerance: int = DEFAULT_OFFSET_TOLERANCE
    min_seconds: float = 0.0
    sample_rate: int = SAMPLE_RATE

    def __post_init__(self) -> None:
        k = self.stable_updates
        if k is not None and (int(k) != k or k < 1):
            raise ValueError("stable_updates=%r: need an integer >= 1, or None" % (k,))
        for name in ("min_psr", "min_margin", "min_ratio_margin", "min_seconds"):
            v = getattr(self, name)
            if not isinstance(v, (int, float)) or math.isnan(v):
                raise ValueError("%s=%r: need a number" % (name, v))
        if int(self.offset_tolerance) != self.offset_tolerance or self.offset_tolerance < 0:
            raise ValueError("offset_tolerance=%r: need an integer >= 0" % (self.offset_tolerance,))
        if int(self.sample_rate) != self.sample_rate or self.sample_rate < 1:
            raise ValueError("sample_rate=%r: need an integer >= 1" % (self.sample_rate,))

    def passes(self, st: ProgressState) -> bool:
        """One state against the thresholds and ``min_seconds``."""
        q = st.quality
        if q.flat or not (q.psr >= self.min_psr and q.margin >= self.min_margin):
            return False
        if not (math.isnan(st.other_best) or st.ratio_margin >= self.min_ratio_margin):
            return False
        return st.ref_len >= self.min_seconds * self.sample_rate

    def settled(self, history: Sequence[ProgressState]) -> bool:
        """Pure host decision on a file's states so far, oldest first."""
        k = self.stable_updates
        if k is None or len(history) < k:
            return False
        last = history[-k:]
        new = last[-1]
        return all(st.best_cand == new.best_cand and abs(st.offset - new.offset) <= self.offset_tolerance
                   and self.passes(st) for st in last)


@dataclass
class ProgressiveSyncResult:
    ratio: float
    ratio_index: int
    offset: int
    score: float
    quality: quality.AlignmentQuality
    ratio_margin: float
    consumed_samples: int
    updates: int
    settled: bool
    reasons: List[str] = field(default_factory=list)  # settled: empty; else quality.assess of the final state


def _window(max_offset_seconds, sample_rate) -> int:
    if int(sample_rate) != sample_rate or sample_rate < 1:
        raise ValueError("sample_rate=%r: need an integer >= 1" % (sample_rate,))
    if not isinstance(max_offset_seconds, (int, float)) or not math.isfinite(max_offset_seconds):
        raise ValueError("max_offset_seconds=%r: need a finite lag window (progressive alignment is windowed only)"
                         % (max_offset_seconds,))
    w = int(round(max_offset_seconds * sample_rate))
    if w < 1 or 2 * w > _native.PROG_MAX_LAGS:
        raise ValueError("max_offset_seconds=%r: need a window W of 1 <= W, 2W <= %d samples"
                         % (max_offset_seconds, _native.PROG_MAX_LAGS))
    return w


def _check_tracks(tracks) -> None:
    for t in tracks:
        if len(t) != 3:
            raise ValueError("a track is (start_us, end_us, is_metadata)")
        if len(t[0]) != len(t[1]):
            raise ValueError("start and end times of different lengths")
        if len(t[0]) == 0:
            raise empty_error(1, 0)


def _float_reference_error(dtype, name="ProgressiveSolve.append") -> ValueError:
    """side_call.check_two_level_batch's words for a multi-level float reference."""
    return ValueError("%s needs a two-level reference: a multi-level float reference (FFS_DTYPE_%s) "
                      "is not supported" % (name, "F32" if np.dtype(dtype) == np.float32 else "F64"))


class _DeviceWords:
    """int32 words at a device address, for ``torch.as_tensor``."""

    def __init__(self, ptr: int, n_words: int) -> None:
        self.__cuda_array_interface__ = {"shape": (int(n_words),), "typestr": "<i4", "data": (int(ptr), False),
                                         "version": 2, "strides": None}


class ProgressiveSolve:
    """The progressive solve of many files: every track rasterised once on the device at every ratio, one slot of an
    ``ffs_prog_plan`` per file.  ``append`` feeds reference labels and returns each file's state on what it has read."""

    _append_name = "ProgressiveSolve.append"

    def __init__(self, tracks, max_offset_seconds: float = 60, ratios: Optional[Sequence[float]] = None,
                 sample_rate: int = SAMPLE_RATE, max_reference_seconds: float = DEFAULT_MAX_REFERENCE_SECONDS,
                 top_k: int = quality.DEFAULT_TOP_K, exclusion_samples: int = quality.DEFAULT_EXCLUSION_SAMPLES,
                 ref_levels=(0.0, 1.0)) -> None:
        from .subtitle_raster import rasterize_candidates

        self.w = _window(max_offset_seconds, sample_rate)
        quality.validate_args(self.w, top_k, exclusion_samples)
        self.ratios = list(candidate_ratios() if ratios is None else ratios)
        if not 1 <= len(self.ratios) <= MAX_CANDIDATES:
            raise ValueError("%d ratios: need 1 to %d candidates per file" % (len(self.ratios), MAX_CANDIDATES))
        if not all(isinstance(r, (int, float)) and math.isfinite(r) and r > 0 for r in self.ratios):
            raise ValueError("ratios must be finite and > 0")
        tracks = list(tracks)
        if not tracks:
            raise ValueError("no tracks")
        _check_tracks(tracks)
        if not (isinstance(max_reference_seconds, (int, float)) and math.isfinite(max_reference_seconds)
                and 1 <= max_reference_seconds * sample_rate < 2 ** 30):
            raise ValueError("max_reference_seconds=%r: need 1 <= samples < 2^30" % (max_reference_seconds,))
        lo, hi = float(ref_levels[0]), float(ref_levels[1])
        if not (math.isfinite(lo) and math.isfinite(hi)):
            raise ValueError("two-level vectors need finite levels")
        self.ref_levels = (lo, hi)
        self.sample_rate = int(sample_rate)
        self.top_k, self.exclusion_samples = int(top_k), int(exclusion_samples)
        self.max_ref = int(max_reference_seconds * sample_rate)
        self.n_files, self.n_cand = len(tracks), len(self.ratios)
        self.torch = torch = _native.require_gpu()
        self.rasters = [rasterize_candidates(s, e, m, self.ratios, sample_rate) for s, e, m in tracks]
        for cands in self.rasters:
            for c in cands:
                if c.n < 1:
                    raise empty_error(1, 0)
        max_sub = max(c.n for cands in self.rasters for c in cands)
        self.plan = _native.ProgPlan(self.n_files, self.n_cand, 2 * self.w, self.max_ref, max_sub)
        self.device = torch.device("cuda", self.plan.device)
        self.consumed = [0] * self.n_files
        shape = (self.n_files, self.n_cand)
        self._open(np.arange(self.n_files), np.full(self.n_files, self.n_cand),
                   np.array([[c.packed_words().data_ptr() for c in cands] for cands in self.rasters], np.uint64),
                   np.array([[c.n for c in cands] for cands in self.rasters], np.int64),
                   np.array([[c.lo for c in cands] for cands in self.rasters]).reshape(shape),
                   np.array([[c.hi for c in cands] for cands in self.rasters]).reshape(shape),
                   np.full(self.n_files, lo), np.full(self.n_files, hi), np.full(self.n_files, self.w))

    def _open(self, *tables) -> None:
        self.plan.open(*tables)

    def _chunk(self, f, chunk):
        """(words or None, first_bit, n) of one file's chunk."""
        words, first_bit, n = self._chunk_form(chunk)
        if self.consumed[f] + n > self.max_ref:
            raise ValueError("file %d: %d + %d samples exceed max_reference_seconds (%d samples)"
                             % (f, self.consumed[f], n, self.max_ref))
        return words, first_bit, n

    def _chunk_form(self, chunk):
        """(words or None, first_bit, n) of a chunk in any of its forms."""
        torch = self.torch
        if isinstance(chunk, tuple):
            if len(chunk) != 3:
                raise ValueError("a packed chunk is (int32 CUDA words, first_bit, n)")
            words, first_bit, n = chunk
            if not (hasattr(words, "is_cuda") and words.is_cuda and words.dtype == torch.int32 and words.is_contiguous()):
                raise ValueError("a packed chunk needs contiguous int32 CUDA words")
            if int(first_bit) != first_bit or not 0 <= first_bit < 32:
                raise ValueError("first_bit=%r outside [0, 32)" % (first_bit,))
            if int(n) != n or n < 0 or int(first_bit) + int(n) > 32 * words.numel():
                raise ValueError("n=%r: need 0 <= n and first_bit + n <= the bits of the words" % (n,))
            first_bit, n = int(first_bit), int(n)
        elif hasattr(chunk, "is_cuda"):
            if not chunk.is_cuda:
                raise ValueError("a tensor chunk must be a CUDA label tensor (or pass a host array)")
            if chunk.dtype not in (torch.float32, torch.uint8):
                raise ValueError("a label tensor chunk must be float32 (> 0.5 is speech) or uint8")
            n, first_bit = int(chunk.numel()), 0
            words = None
        else:
            host = np.asarray(chunk)
            if host.dtype != np.bool_:
                if host.dtype.kind == "f" and not np.all((host == 0) | (host == 1)):
                    raise _float_reference_error(host.dtype if host.dtype == np.float32 else np.float64, self._append_name)
                if not np.all((host == 0) | (host == 1)):
                    raise ValueError("a host chunk must hold 0/1 or bool samples")
            n, first_bit = int(host.size), 0
            words = None
        return words, first_bit, n

    def _device_words(self, chunk, words, n):
        """The int32 CUDA words of a checked chunk (packed here unless it came packed)."""
        torch = self.torch
        if words is None:
            if hasattr(chunk, "is_cuda"):
                words = _native.pack_bits(chunk.contiguous().reshape(-1)) if n else None
            elif n:
                packed = np.packbits(np.asarray(chunk).ravel() != 0, bitorder="little")
                host = np.zeros((n + 31) // 32 * 4, np.uint8)
                host[:packed.size] = packed
                words = torch.from_numpy(host.view(np.int32)).to(self.device)
            if words is None or words.numel() == 0:
                words = torch.zeros(1, dtype=torch.int32, device=self.device)
        return words

    def _check_open(self, name="ProgressiveSolve") -> None:
        if self.plan is None:
            raise ValueError("this %s is closed" % name)

    def _check_file(self, f) -> None:
        if not isinstance(f, (int, np.integer)) or not 0 <= f < self.n_files:
            raise ValueError("file %r: need an index in [0, %d)" % (f, self.n_files))

    def append(self, chunks: Dict[int, object]) -> Dict[int, ProgressState]:
        """Feed one chunk per named file (index into the tracks): a host 0/1 or bool array, a CUDA label tensor
        (float32: > 0.5 is speech; uint8: != 0), or (int32 CUDA words, first_bit, n).  One native call for all of them."""
        self._check_open()
        files = list(chunks)
        for f in files:
            self._check_file(f)
        if not files:
            return {}
        checked = [self._chunk(f, chunks[f]) for f in files]  # every ValueError before any native call
        return self._append(files, checked, None, [chunks[f] for f in files])

    def _append(self, files, checked, starts, chunks) -> Dict[int, ProgressState]:
        """``append`` and, with the ``starts`` of the chunks, ``SampledSolve.append_at`` behind their checks: the chunks
        of ``files`` in their ``checked`` (words or None, first_bit, n) forms onto the device, one native call, the
        host's books (only once that call has returned), the records read back."""
        torch = self.torch
        keep = [self._device_words(chunk, words, n) for chunk, (words, _, n) in zip(chunks, checked)]
        ptrs, bits, lens = [w.data_ptr() for w in keep], [c[1] for c in checked], [c[2] for c in checked]
        n = len(files)
        cand_out = torch.empty(n * self.n_cand * _native.QUALITY_RESULT_BYTES, dtype=torch.uint8, device=self.device)
        state_out = torch.empty(n * _native.PROG_STATE_BYTES, dtype=torch.uint8, device=self.device)
        if starts is None:
            self.plan.append(files, ptrs, bits, lens, self.top_k, self.exclusion_samples, cand_out, state_out)
        else:
            self.plan.append_at(files, ptrs, bits, starts, lens, self.top_k, self.exclusion_samples, cand_out, state_out)
        for i, f in enumerate(files):
            self.consumed[f] += lens[i]
            if starts is not None and lens[i]:
                self._known[f] = _merged(self._known[f] + [(starts[i], starts[i] + lens[i])])
        recs = cand_out.cpu().numpy().view(_native.QUALITY_RESULT_DTYPE).reshape(n, self.n_cand)
        states = state_out.cpu().numpy().view(_native.PROG_STATE_DTYPE)
        del keep
        self.last_records = {f: recs[i] for i, f in enumerate(files)}  # the raw candidate records of the last call
        self.last_states = {f: states[i] for i, f in enumerate(files)}
        return {f: state_from_records(states[i], recs[i]) for i, f in enumerate(files)}

    def reference(self, f: int):
        """The consumed prefix of file ``f`` as a ``DeviceRaster`` (a copy): a settled file can go straight into
        ``split_sync`` / ``drift_sync`` on what was read."""
        from .subtitle_raster import DeviceRaster

        self._check_open()
        self._check_file(f)
        torch = self.torch
        ptr, n = self.plan.reference(f)
        if n == 0:
            return DeviceRaster(torch.zeros(0, dtype=torch.int32, device=self.device), *self.ref_levels, n=0)
        with torch.cuda.device(self.device):
            words = torch.as_tensor(_DeviceWords(ptr, (n + 31) // 32), device=self.device).clone()
        return DeviceRaster(words, *self.ref_levels, n=n)

    def close(self) -> None:
        if self.plan is not None:
            self.plan.close()
            self.plan = None
            self.rasters = []

    def __enter__(self):
        return self

    def __exit__(self, *exc) -> None:
        self.close()


def state_from_records(state, cand_records) -> ProgressState:
    """``ProgressState`` of one ``PROG_STATE_DTYPE`` record and the slot's candidate records."""
    best = int(state["best_cand"])
    rec = cand_records[best]
    peaks = [(float(rec["peak_score"][i]), int(rec["peak_offset"][i])) for i in range(int(rec["n_peaks"]))]
    mean, std, score, other = float(state["mean"]), float(state["std"]), float(state["score"]), float(state["other_best"])
    psr, margin, flags, (gain,) = quality.derive(peaks, mean, std, int(state["flags"]), own=score, others=[other])
    q = quality.AlignmentQuality(peaks, mean, std, int(rec["n_lags"]), psr, margin, flags)
    return ProgressState(int(state["ref_len"]), best, int(state["offset"]), score, q, gain, other)


def pcm_label_chunks(source, sample_rate: int = SAMPLE_RATE, frame_rate: int = 48000,
                     energy_threshold_db: float = DEFAULT_ENERGY_THRESHOLD_DB):
    """The energy detector's 100 s buffers (``WINDOWS_PER_BUFFER`` frames each) of an s16le mono stream as label chunks
    for ``ProgressiveSolve.append`` / ``progressive_sync``: yields (int32 CUDA words, first_bit, n) per buffer, through
    ``ffs_vad_energy_bits``.  ``source``: what ``PCMSpeechTransformer.fit`` accepts -- a binary file object (e.g.
    ``subprocess.Popen(...).stdout``), bytes or an int16 array -- or an int16 CPU tensor, as ``detect_pinned_stream``
    takes (pinned: copied without staging).  Nothing is read ahead of the consumer; other detectors supply their own
    label chunks."""
    from .speech_transformers import BYTES_PER_SAMPLE, WINDOWS_PER_BUFFER, PCMSpeechTransformer, frames_per_window

    frame_len = frames_per_window(sample_rate, frame_rate)
    chunk_bytes = frame_len * WINDOWS_PER_BUFFER * BYTES_PER_SAMPLE
    if hasattr(source, "is_pinned"):  # an int16 CPU tensor (pinned: the copies need no staging), as detect_pinned_stream takes
        if str(source.dtype) != "torch.int16":
            raise ValueError("a PCM tensor must be int16 (s16le mono samples)")
        flat = source.reshape(-1)
        step = chunk_bytes // BYTES_PER_SAMPLE
        for o in range(0, int(flat.numel()), step):
            pcm = flat[o:o + step].to("cuda", non_blocking=True)
            words, n_frames = _native.vad_energy_bits(pcm, frame_len, energy_threshold_db)
            yield words, 0, n_frames
        return
    reader = PCMSpeechTransformer(vad="energy", sample_rate=sample_rate, frame_rate=frame_rate)
    for in_bytes in reader._chunks(source, chunk_bytes):
        n = in_bytes.size // BYTES_PER_SAMPLE * BYTES_PER_SAMPLE
        if n == 0:
            continue
        torch = _native.require_gpu()
        pcm = torch.from_numpy(np.array(in_bytes[:n], copy=True).view("<i2")).cuda()
        words, n_frames = _native.vad_energy_bits(pcm, frame_len, energy_threshold_db)
        yield words, 0, n_frames


def progressive_sync(problems, rule: Optional[StopRule] = None, max_offset_seconds: float = 60,
                     ratios: Optional[Sequence[float]] = None, sample_rate: int = SAMPLE_RATE,
                     max_reference_seconds: float = DEFAULT_MAX_REFERENCE_SECONDS, top_k: int = quality.DEFAULT_TOP_K,
                     exclusion_samples: int = quality.DEFAULT_EXCLUSION_SAMPLES,
                     ref_levels=(0.0, 1.0)) -> List[ProgressiveSyncResult]:
    """Sync many files while their audio decodes.  ``problems``: (chunk iterable, track) per file -- the iterable yields
    reference label chunks as ``ProgressiveSolve.append`` takes them (``pcm_label_chunks`` for decoded PCM), the track is
    the (start_us, end_us, is_metadata) triple of ``subtitle_raster.subtitle_records``.  Runs in rounds: one chunk from
    every live file, one append.  A file that ``rule`` calls settled is never pulled again, and its iterable's ``close()``
    is called if it has one (the hook for ending the decoder).  A file that never settles ends with the answer on its
    whole reference, ``quality.quality_sync``'s wherever the reference's lag mask is the window."""
    rule = StopRule() if rule is None else rule
    problems = list(problems)
    for p in problems:
        if len(p) != 2:
            raise ValueError("a problem is (chunk iterable, (start_us, end_us, is_metadata))")
    solve = ProgressiveSolve([p[1] for p in problems], max_offset_seconds, ratios, sample_rate, max_reference_seconds,
                             top_k, exclusion_samples, ref_levels)
    try:
        sources = [p[0] for p in problems]
        iters: List[Optional[Iterable]] = [iter(s) for s in sources]

        def rounds():
            while any(it is not None for it in iters):
                chunks = {}
                for f, it in enumerate(iters):
                    if it is None:
                        continue
                    try:
                        chunks[f] = next(it)
                    except StopIteration:
                        iters[f] = None
                yield chunks

        def settle(f):
            for obj in (sources[f], iters[f]):  # the caller's own object first: it knows its decoder
                close = getattr(obj, "close", None)
                if close is not None:
                    close()
                    break
            iters[f] = None

        return _sync_rounds(solve, rule, solve.append, rounds, settle)
    finally:
        solve.close()


def _sync_rounds(solve, rule, append, rounds, settle) -> List[ProgressiveSyncResult]:
    """The rounds of ``progressive_sync`` and ``sampled_sync`` and their results.  ``rounds()`` yields one round's chunks
    of the live files at a time, as ``append`` takes them, while any file is live; ``settle(f)`` is told when ``rule``
    calls file ``f`` settled: it is not to be read again."""
    history: List[List[ProgressState]] = [[] for _ in range(solve.n_files)]
    done = [False] * solve.n_files
    for chunks in rounds():
        for f, st in append(chunks).items():
            history[f].append(st)
            if rule.settled(history[f]):
                done[f] = True
                settle(f)
    out = []
    for f, h in enumerate(history):
        if not h:
            raise empty_error(0, solve.rasters[f][0].n)
        st = h[-1]
        reasons = [] if done[f] else quality.assess(st.quality, rule.min_psr, rule.min_margin)
        out.append(ProgressiveSyncResult(solve.ratios[st.best_cand], st.best_cand, st.offset, st.score, st.quality,
                                         st.ratio_margin, st.ref_len, len(h), done[f], reasons))
    return out


def _merged(intervals):
    """Sorted disjoint intervals with abutting neighbours joined (a ``SampledSolve``'s books of what it has fed)."""
    out: List[List[int]] = []
    for a, b in sorted(intervals):
        if out and out[-1][1] == a:
            out[-1][1] = b
        else:
            out.append([a, b])
    return [(a, b) for a, b in out]
