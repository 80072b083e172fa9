"""Sampled alignment: read a few segments spread over the audio, score only what was read, stop when settled.

Progressive alignment (``progressive.py``) reads a prefix.  The reference project's one fast mode, ``--multi-segment-sync``
(``MultiSegmentVideoSpeechTransformer``, speech_transformers.py:760-903), reads windows spread over the file instead and
places them in a vector that is zero everywhere else -- so every cue on unread audio is charged as a mismatch.  Here an
unread frame contributes nothing to the score (``csrc/ffs_sampled.h``): the counts run over the known frames only, which
is what the reference aligner computes on a vector that holds 0.5 in every unread frame.  Counts are additive over any
set of reference samples, so every segment costs one small update and the exact seven-ratio answer on what has been read
is there after each one; ``progressive.StopRule`` decides, unchanged, with ``min_seconds`` counting known seconds.

Parity is against the numpy model ``tests/sampled_model.py``.  Two-level references only, windowed only, disjoint
segments only.  The default rule comes from synthetic data (``profiles/sampled_calibration.json``); whether spread
segments settle earlier than a prefix on real films is not measured.  Nothing here changes an existing entry point.
"""
import math
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native, quality
from .constants import DEFAULT_ENERGY_THRESHOLD_DB, SAMPLE_RATE
from .progressive import ProgressiveSolve, ProgressiveSyncResult, ProgressState, StopRule, _sync_rounds

MAX_INTERVALS = _native.PROG_MAX_INTERVALS
# Chosen by profiles/progressive_calibration.py's rule on the CPU model (profiles/sampled_calibration.json):
# of the (stable_updates, min_ratio_margin) cells without a wrong stop, the one that reads least, moved one step to the
# safe side on both axes.  On the synthetic files NO cell is free of wrong stops on the spread schedule (at one hour a
# file can settle three or four samples from its full-reference offset, beyond the tolerance of two), so by the rule
# the default never settles: pass a StopRule to stop early.
DEFAULT_SAMPLED_STABLE_UPDATES: Optional[int] = None
DEFAULT_SAMPLED_MIN_RATIO_MARGIN = 0.0
DEFAULT_SAMPLED_RULE = StopRule(min_ratio_margin=DEFAULT_SAMPLED_MIN_RATIO_MARGIN,
                                stable_updates=DEFAULT_SAMPLED_STABLE_UPDATES)


def _bit_reversed(n: int) -> List[int]:
    """0 .. n-1 in bit-reversed order: m runs over the bit reversals of 0 .. N-1 (N the power of two >= n) and names
    floor(m n / N), first mention only.  For n a power of two this is the bit reversal itself; for any n the first 2^k
    entries are floor(i n / 2^k), evenly spread."""
    bits = max(n - 1, 0).bit_length()
    out, seen = [], set()
    for m in range(1 << bits):
        k = (int(format(m, "0%db" % bits)[::-1], 2) if bits else 0) * n >> bits
        if k not in seen:
            seen.add(k)
            out.append(k)
    return out


def segment_schedule(total_samples: int, segment_samples: int) -> List[Tuple[int, int]]:
    """The grid segments [k seg, min((k + 1) seg, T)) in bit-reversed order of k: any prefix of the schedule is spread
    over the file, the whole schedule tiles [0, T) exactly."""
    if int(total_samples) != total_samples or total_samples < 1:
        raise ValueError("total_samples=%r: need an integer >= 1" % (total_samples,))
    if int(segment_samples) != segment_samples or segment_samples < 1:
        raise ValueError("segment_samples=%r: need an integer >= 1" % (segment_samples,))
    total, seg = int(total_samples), int(segment_samples)
    return [(k * seg, min((k + 1) * seg, total)) for k in _bit_reversed((total + seg - 1) // seg)]


def prefix_schedule(total_samples: int, segment_samples: int) -> List[Tuple[int, int]]:
    """The same segments front to back (what ``progressive_sync`` reads)."""
    return sorted(segment_schedule(total_samples, segment_samples))


def _totals(durations, n_files: int, sample_rate: int) -> List[int]:
    durations = list(durations)
    if len(durations) != n_files:
        raise ValueError("%d durations for %d tracks: need one per file" % (len(durations), n_files))
    out = []
    for d in durations:
        if not isinstance(d, (int, float, np.integer, np.floating)) or not math.isfinite(d):
            raise ValueError("duration %r: need finite seconds" % (d,))
        t = int(d * sample_rate)
        if not 1 <= t < 2 ** 30:
            raise ValueError("duration %r: need 1 <= samples < 2^30" % (d,))
        out.append(t)
    return out


class SampledSolve(ProgressiveSolve):
    """``ProgressiveSolve`` on sampled slots: every file has a declared duration, and ``append_at`` feeds reference
    labels at any position not read yet.  The state after each call is the exact masked answer on the known frames."""

    _append_name = "SampledSolve.append_at"

    def __init__(self, tracks, durations, max_offset_seconds: float = 60, ratios: Optional[Sequence[float]] = None,
                 sample_rate: int = SAMPLE_RATE, top_k: int = quality.DEFAULT_TOP_K,
                 exclusion_samples: int = quality.DEFAULT_EXCLUSION_SAMPLES, ref_levels=(0.0, 1.0)) -> None:
        tracks = list(tracks)
        if int(sample_rate) != sample_rate or sample_rate < 1:
            raise ValueError("sample_rate=%r: need an integer >= 1" % (sample_rate,))
        self.totals = _totals(durations, len(tracks), int(sample_rate)) if tracks else []
        self._known: List[List[Tuple[int, int]]] = [[] for _ in tracks]
        super().__init__(tracks, max_offset_seconds, ratios, sample_rate,
                         (max(self.totals, default=1) + 0.5) / sample_rate, top_k, exclusion_samples, ref_levels)

    def _open(self, *tables) -> None:
        self.plan.open_sampled(*tables, np.array(self.totals, np.int64))

    def append(self, chunks):
        raise ValueError("a SampledSolve takes positions: use append_at({file: (start_sample, chunk)})")

    def _check_interval(self, f: int, a, n: int) -> int:
        if not isinstance(a, (int, np.integer)) or a < 0 or a + n > self.totals[f]:
            raise ValueError("file %d: [%r, %r + %d) outside the reference [0, %d)" % (f, a, a, n, self.totals[f]))
        a = int(a)
        if n == 0:
            return a
        joins = 0
        for lo, hi in self._known[f]:
            if a < hi and lo < a + n:
                raise ValueError("file %d: [%d, %d) overlaps the known interval [%d, %d)" % (f, a, a + n, lo, hi))
            joins += (hi == a) + (lo == a + n)
        if len(self._known[f]) + 1 - joins > MAX_INTERVALS:
            raise ValueError("file %d: more than %d known intervals" % (f, MAX_INTERVALS))
        return a

    def append_at(self, chunks: Dict[int, tuple]) -> Dict[int, ProgressState]:
        """Feed one (start_sample, chunk) per named file; ``chunk`` in any form ``ProgressiveSolve.append`` takes.  The
        samples must lie inside [0, duration) and must not have been fed before.  One native call for all of them."""
        self._check_open("SampledSolve")
        files = list(chunks)
        for f in files:
            self._check_file(f)
            if not isinstance(chunks[f], tuple) or len(chunks[f]) != 2:
                raise ValueError("file %d: need (start_sample, chunk)" % f)
        if not files:
            return {}
        checked, starts = [], []  # every ValueError before any native call
        for f in files:
            start, chunk = chunks[f]
            form = self._chunk_form(chunk)
            starts.append(self._check_interval(f, start, form[2]))
            checked.append(form)
        return self._append(files, checked, starts, [chunks[f][1] for f in files])

    def known(self, f: int) -> List[Tuple[int, int]]:
        """The merged known intervals of file ``f``, ascending (``ffs_prog_known``)."""
        self._check_open("SampledSolve")
        self._check_file(f)
        return [(int(a), int(b)) for a, b in self.plan.known(f)]


def _segment_chunk(data, n_want: int, sample_rate: int, frame_rate: int, energy_threshold_db: float):
    """What ``read_segment`` returned as a chunk of at most ``n_want`` labels: int16 samples (array, bytes or tensor) are
    PCM and go through ``ffs_vad_energy_bits`` as in ``pcm_label_chunks``; anything else is labels already."""
    from .speech_transformers import frames_per_window

    if isinstance(data, (bytes, bytearray, memoryview)):
        raw = np.frombuffer(data, np.uint8)
        data = np.array(raw[:raw.size // 2 * 2], copy=True).view("<i2")
    is_tensor = hasattr(data, "is_cuda")
    if (is_tensor and str(data.dtype) == "torch.int16") or (not is_tensor and not isinstance(data, tuple)
                                                           and np.asarray(data).dtype == np.int16):
        torch = _native.require_gpu()
        frame_len = frames_per_window(sample_rate, frame_rate)
        pcm = data if is_tensor else torch.from_numpy(np.ascontiguousarray(data))
        pcm = pcm.reshape(-1)[:n_want * frame_len].to("cuda", non_blocking=True)
        if int(pcm.numel()) < frame_len:
            return np.zeros(0, bool)
        words, n_frames = _native.vad_energy_bits(pcm, frame_len, energy_threshold_db)
        return words, 0, min(int(n_frames), n_want)
    if isinstance(data, tuple):
        if len(data) != 3:
            raise ValueError("a packed chunk is (int32 CUDA words, first_bit, n)")
        return data[0], data[1], min(int(data[2]), n_want)
    return data[:n_want]


def _chunk_len(chunk) -> int:
    """The samples of a chunk in any of its forms."""
    if isinstance(chunk, tuple):
        return int(chunk[2])
    return int(chunk.numel()) if hasattr(chunk, "is_cuda") else int(np.asarray(chunk).size)


def sampled_sync(problems, rule: Optional[StopRule] = None, segment_seconds: float = 60,
                 order: Optional[Callable[[int, int], Sequence[Tuple[int, int]]]] = None, max_offset_seconds: float = 60,
                 ratios: Optional[Sequence[float]] = None, sample_rate: int = SAMPLE_RATE,
                 top_k: int = quality.DEFAULT_TOP_K, exclusion_samples: int = quality.DEFAULT_EXCLUSION_SAMPLES,
                 ref_levels=(0.0, 1.0), frame_rate: int = 48000,
                 energy_threshold_db: float = DEFAULT_ENERGY_THRESHOLD_DB) -> List[ProgressiveSyncResult]:
    """Sync many files from segments of their audio.  ``problems``: (read_segment, track, duration_seconds) per file --
    ``read_segment(start_seconds, seconds)`` returns that stretch as reference labels in any form
    ``ProgressiveSolve.append`` takes, or as int16 PCM at ``frame_rate`` (the hook for ``ffmpeg -ss ... -t ...``); the
    track is the (start_us, end_us, is_metadata) triple of ``subtitle_raster.subtitle_records``.  ``order(total_samples,
    segment_samples)`` gives each file's disjoint segments in reading order (default ``segment_schedule``; pass
    ``prefix_schedule`` to read front to back).  ``read_segment`` must return the whole segment: more is cut off, less
    is a ValueError before that round's native call (a hole would break the interval count checked up front, and a file
    that never settles would not have read everything).  Runs in rounds: one segment from every live file, one native
    call.  A file that ``rule`` calls settled is never read again, and ``read_segment.close()`` is called if it has one.
    A file that never settles has read everything and ends on the full-reference answer: ``quality.quality_sync``'s
    wherever the reference's lag mask is the window."""
    rule = DEFAULT_SAMPLED_RULE if rule is None else rule
    if not isinstance(rule, StopRule):
        raise ValueError("rule=%r: need a StopRule" % (rule,))
    problems = list(problems)
    for p in problems:
        if len(p) != 3 or not callable(p[0]):
            raise ValueError("a problem is (read_segment, (start_us, end_us, is_metadata), duration_seconds)")
    if int(sample_rate) != sample_rate or sample_rate < 1:
        raise ValueError("sample_rate=%r: need an integer >= 1" % (sample_rate,))
    if not isinstance(segment_seconds, (int, float)) or not math.isfinite(segment_seconds) \
            or int(segment_seconds * sample_rate) < 1:
        raise ValueError("segment_seconds=%r: need at least one sample" % (segment_seconds,))
    seg = int(segment_seconds * sample_rate)
    order = segment_schedule if order is None else order
    if not callable(order):
        raise ValueError("order=%r: need a function (total_samples, segment_samples) -> [(a, b)]" % (order,))
    totals = _totals([p[2] for p in problems], len(problems), int(sample_rate))
    schedules = []
    for t in totals:
        sched = [(int(a), int(b)) for a, b in order(t, seg)]
        flat = sorted(sched)
        if any(not 0 <= a < b <= t for a, b in sched) or any(x[1] > y[0] for x, y in zip(flat, flat[1:])):
            raise ValueError("order: need disjoint segments inside [0, %d)" % t)
        count, starts, ends = 0, set(), set()
        for a, b in sched:  # the merged intervals after every append: one more, less one per neighbour it abuts
            count += 1 - (a in ends) - (b in starts)
            starts.add(a)
            ends.add(b)
            if count > MAX_INTERVALS:
                raise ValueError("order: more than %d known intervals at a time" % MAX_INTERVALS)
        schedules.append(sched)
    solve = SampledSolve([p[1] for p in problems], [p[2] for p in problems], max_offset_seconds, ratios, sample_rate, top_k,
                         exclusion_samples, ref_levels)
    try:
        readers = [p[0] for p in problems]
        at = [0] * len(problems)
        live = [bool(s) for s in schedules]

        def rounds():
            while any(live):
                chunks = {}
                for f, sched in enumerate(schedules):
                    if not live[f]:
                        continue
                    a, b = sched[at[f]]
                    at[f] += 1
                    live[f] = at[f] < len(sched)
                    data = readers[f](a / sample_rate, (b - a) / sample_rate)
                    chunk = _segment_chunk(data, b - a, solve.sample_rate, frame_rate, energy_threshold_db)
                    if _chunk_len(chunk) != b - a:
                        raise ValueError("file %d: read_segment(%r, %r) returned %d samples, the segment has %d"
                                         % (f, a / sample_rate, (b - a) / sample_rate, _chunk_len(chunk), b - a))
                    chunks[f] = (a, chunk)
                yield chunks

        def settle(f):
            live[f] = False
            close = getattr(readers[f], "close", None)
            if close is not None:
                close()

        return _sync_rounds(solve, rule, solve.append_at, rounds, settle)
    finally:
        solve.close()
