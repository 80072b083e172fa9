"""Per-cue evidence report: which lines are still wrong after a sync?

Every sync of this library ends by writing cue times, and its reports stop one level above the cue (whole file, piece,
segment, break).  This module looks at each cue by itself (``csrc/ffs_cue_report.h``): in the cue's own
neighbourhood (``context_samples`` on each side) it scores the lag the sync applied and every lag within
``radius_samples`` of it with the split's exact two-level score, and it counts the reference speech under the cue
itself.  From the record one can tell a cue whose neighbourhood fits better at another lag ("shifted"), a cue the video
has no speech for at any lag nearby ("silent": an SDH line, a lyric, a sign, a credit), and a cue that is mostly
uncovered at the lag it got.

``cue_table`` turns cue times into the device table, ``cue_report_batch`` is the device call, ``cue_report_sync`` runs it
behind any sync result, ``assess_cues`` gives a verdict per cue and ``snap_cues`` moves the "shifted" ones.

Parity is against the in-repo numpy model ``tests/cue_model.py``, bit for bit.  No existing entry point changes.
"""
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _native
from .constants import SAMPLE_RATE
from .side_call import bits_batch, check_two_level_batch, no_workspace_split_plan
from .split_align import _scaled_us, empty_error

# Chosen on the CPU model (profiles/cue_report_calibration.py -> profiles/cue_report_calibration.json;
# synthetic data only, nobody has measured real files)
DEFAULT_RADIUS = 300
DEFAULT_CONTEXT = 100
DEFAULT_MIN_GAIN = 0.2
DEFAULT_MIN_COVER = 0.85


@dataclass
class CueReport:
    start: int  # the cue as given: subtitle samples [start, end) and the lag the sync applied
    end: int
    lag: int
    lo: int  # the window [lo, hi): the cue and its context, inside the subtitle vector
    hi: int
    own: tuple  # (ov, n11, n1x, nx1) of the window at the applied lag
    best: tuple  # the same at lag + best_delta
    own_score: float
    best_score: float
    best_delta: int
    n_best: int  # lags within the radius that reach best_score
    cue_own_n11: int  # reference speech under the cue at the applied lag, of cue_own_ov samples with a partner
    cue_own_ov: int
    cue_max_n11: int  # the most reference speech under the cue at any lag within the radius, at lag + cue_max_delta
    cue_max_delta: int
    flags: int  # _native.CUE_*

    @property
    def empty(self) -> bool:
        return bool(self.flags & (_native.CUE_EMPTY | _native.CUE_INVALID))

    @property
    def silent(self) -> bool:
        return bool(self.flags & _native.CUE_SILENT)

    @property
    def at_edge(self) -> bool:
        return bool(self.flags & _native.CUE_BEST_AT_EDGE)

    @property
    def gain(self) -> float:
        return self.best_score - self.own_score

    @property
    def cover(self) -> float:
        """The share of the cue's samples (those with a partner) that meet reference speech at the applied lag."""
        return self.cue_own_n11 / self.cue_own_ov if self.cue_own_ov > 0 else 0.0


def from_record(rec) -> CueReport:
    """CueReport of one ``_native.CUE_REPORT_DTYPE`` record (or of a model record with the same fields)."""
    return CueReport(int(rec["start"]), int(rec["end"]), int(rec["lag"]), int(rec["lo"]), int(rec["hi"]),
                     tuple(int(x) for x in rec["own"]), tuple(int(x) for x in rec["best"]), float(rec["own_score"]),
                     float(rec["best_score"]), int(rec["best_delta"]), int(rec["n_best"]), int(rec["cue_own_n11"]),
                     int(rec["cue_own_ov"]), int(rec["cue_max_n11"]), int(rec["cue_max_delta"]), int(rec["flags"]))


def validate_args(radius_samples, context_samples) -> None:
    """Host-side checks of the call parameters (ValueError before any native call)."""
    r = int(radius_samples)
    if r != radius_samples or not 0 <= r <= _native.CUE_MAX_RADIUS:
        raise ValueError("radius_samples=%r: need an integer in [0, %d]" % (radius_samples, _native.CUE_MAX_RADIUS))
    m = int(context_samples)
    if m != context_samples or not 0 <= m <= _native.CUE_MAX_CONTEXT:
        raise ValueError("context_samples=%r: need an integer in [0, %d]" % (context_samples, _native.CUE_MAX_CONTEXT))


def flat_cue_table(cues, n_pairs: int):
    """The flat ``_native.CUE_DTYPE`` table of per-pair (start, end, lag) triples, and each pair's first entry and
    count (ValueError for a wrong number of pairs or mismatched lengths)."""
    if len(cues) != n_pairs:
        raise ValueError("%d cue tables for %d pairs" % (len(cues), n_pairs))
    cols = []
    for p, triple in enumerate(cues):
        if len(triple) != 3:
            raise ValueError("pair %d: cues are a (start, end, lag) triple of arrays" % p)
        start, end, lag = (np.asarray(x, dtype=np.int64).ravel() for x in triple)
        if not start.size == end.size == lag.size:
            raise ValueError("pair %d: %d starts, %d ends and %d lags: the three cue arrays need one length"
                             % (p, start.size, end.size, lag.size))
        cols.append((start, end, lag))
    count = np.array([c[0].size for c in cols], dtype=np.int64)
    first = np.zeros(n_pairs, np.int64)
    if n_pairs:
        np.cumsum(count[:-1], out=first[1:])
    table = np.zeros(int(count.sum()), _native.CUE_DTYPE)
    for (start, end, lag), f, c in zip(cols, first, count):
        table["start"][f:f + c], table["end"][f:f + c], table["lag"][f:f + c] = start, end, lag
    return table, first, count


_plans = _native.SidePlanCache(_native.SplitPlan)


def _get_plan(n_pairs: int):
    """A split plan of this device that holds no split workspace: cue report calls use its sub-batching only."""
    return no_workspace_split_plan(_plans, n_pairs)


def clear_plan_cache() -> None:
    _plans.clear()


def cue_report_batch(batch, cues, radius_samples: int = DEFAULT_RADIUS, context_samples: int = DEFAULT_CONTEXT,
                     raw: bool = False, plan=None):
    """Per-cue reports of every pair of a ``batch.DeviceBatch`` with ONE candidate per pair.  ``cues``: one (start, end,
    lag) triple of int64 arrays per pair -- subtitle samples [start, end) and the lag the sync applied (``cue_table``).
    Returns one list of ``CueReport`` per pair, or with ``raw`` (the ``_native.CUE_REPORT_DTYPE`` records of the flat
    table, the per-pair slices into it)."""
    validate_args(radius_samples, context_samples)
    check_two_level_batch(batch, "cue_report_batch", float_ref_message=True)
    n = batch.n_pairs
    table, first, count = flat_cue_table(cues, n)
    slices = [slice(int(f), int(f + c)) for f, c in zip(first, count)]
    torch = _native.require_gpu()
    batch = bits_batch(batch)
    dev = batch.data.device
    if table.size:
        cue_dev = torch.from_numpy(table.view(np.uint8).reshape(-1)).to(dev)
        rec_out = torch.empty(table.size * _native.CUE_REPORT_BYTES, dtype=torch.uint8, device=dev)
        plan = _get_plan(n) if plan is None else plan
        plan.cue_report(*batch.pair_arrays(), cue_dev, first, count, int(radius_samples), int(context_samples), rec_out)
        recs = rec_out.cpu().numpy().view(_native.CUE_REPORT_DTYPE)
    else:
        recs = np.zeros(0, _native.CUE_REPORT_DTYPE)
    if raw:
        return recs, slices
    return [[from_record(x) for x in recs[sl]] for sl in slices]


def cue_table(start_us, end_us, ratio: float, out_start_us, sample_rate: int = SAMPLE_RATE, is_metadata=None,
              sub_len: Optional[int] = None):
    """The (start, end, lag) sample table of a track's cues behind a sync that scaled them by ``ratio`` and wrote the
    start times ``out_start_us``.  [start, end) is the rasteriser's own interval (``ffs_raster_intervals``: the scaling
    of ``split_align._scaled_us``, its start and length rounding, its clamp to the raster of ``sub_len`` samples -- by
    default the track's own raster length): exactly the run the cue contributed to the subtitle vector at that ratio; a
    cue that contributed nothing (metadata, no sample) is [0, 0).  lag = rint((out_start_us - scaled start) * rate /
    10^6): the integer piece or block offset of a piecewise sync exactly, a polyline shift rounded."""
    start_us = np.asarray(start_us, dtype=np.int64).ravel()
    end_us = np.asarray(end_us, dtype=np.int64).ravel()
    out_start_us = np.asarray(out_start_us, dtype=np.int64).ravel()
    if not start_us.size == end_us.size == out_start_us.size:
        raise ValueError("%d starts, %d ends and %d output starts: the cue arrays need one length"
                         % (start_us.size, end_us.size, out_start_us.size))
    n = start_us.size
    if sub_len is None:
        sub_len = _native.raster_length(end_us, ratio, sample_rate) if n else 0
    meta = None if is_metadata is None else np.asarray(is_metadata).ravel()
    iv = _native.raster_intervals(start_us, end_us, meta, ratio, sample_rate, 0.0, sub_len)
    if iv.shape[0] != n:  # some cues contribute nothing and are left out of the list: one by one
        iv = np.zeros((n, 2), np.int32)
        for i in range(n):
            if meta is not None and meta[i]:
                continue
            one = _native.raster_intervals(start_us[i:i + 1], end_us[i:i + 1], None, ratio, sample_rate, 0.0, sub_len)
            if one.shape[0]:
                iv[i] = one[0]
    scaled = np.array([_scaled_us(u, ratio) for u in start_us], dtype=np.int64)
    lag = np.rint((out_start_us - scaled).astype(np.float64) * float(sample_rate) / 1e6).astype(np.int64)
    return iv[:, 0].astype(np.int64), iv[:, 1].astype(np.int64), lag


def cue_report_sync(problems, results, radius_samples: int = DEFAULT_RADIUS, context_samples: int = DEFAULT_CONTEXT,
                    sample_rate: int = SAMPLE_RATE, raw: bool = False):
    """Per-cue reports behind any sync: ``problems`` as the sync took them ((reference, (start_us, end_us,
    is_metadata)) pairs), ``results`` its outputs (anything with ``ratio``, ``cue_start_us`` and ``cue_end_us``).  Each
    track is rasterised once at its result's ratio, the tables come from ``cue_table``, and one device call reports on
    every cue.  Returns one ``CueReport`` list per problem (``raw``: as ``cue_report_batch``)."""
    from . import batch as batch_mod
    from .subtitle_raster import DeviceRaster, rasterize_candidates

    validate_args(radius_samples, context_samples)
    if len(problems) != len(results):
        raise ValueError("%d results for %d problems" % (len(results), len(problems)))
    pairs, tables = [], []
    for p, ((ref, (start_us, end_us, meta)), res) in enumerate(zip(problems, results)):
        if len(start_us) == 0:
            raise empty_error(len(ref), 0)
        if len(res.cue_start_us) != len(start_us):
            raise ValueError("problem %d: %d cues, %d output times" % (p, len(start_us), len(res.cue_start_us)))
        if not isinstance(ref, DeviceRaster):
            host = np.asarray(ref, dtype=np.float64).ravel()
            if host.size == 0:
                raise empty_error(0, 1)
            if not np.all(np.isfinite(host)):
                raise ValueError("problem %d: the reference has non-finite levels" % p)
            if np.unique(host).size > 2:
                raise ValueError("cue_report_sync needs two-level references: reference %d is a multi-level float "
                                 "reference, which is not supported" % p)
            _native.require_gpu()
            ref = DeviceRaster.from_host(host, lists=False)
        elif ref.n == 0:
            raise empty_error(0, 1)
        sub = rasterize_candidates(start_us, end_us, meta, [res.ratio], sample_rate)[0]
        pairs.append((ref, [sub]))
        tables.append(cue_table(start_us, end_us, res.ratio, res.cue_start_us, sample_rate, meta, sub.n))
    return cue_report_batch(batch_mod.pack_pairs(pairs), tables, radius_samples, context_samples, raw)


def assess_cues(reports: Sequence[CueReport], min_gain: float = DEFAULT_MIN_GAIN,
                min_cover: float = DEFAULT_MIN_COVER) -> List[str]:
    """One verdict per cue, the first that applies: "empty" (no sample, or an invalid lag); "silent" (no reference
    speech under the cue at any lag within the radius); "shifted" (another lag inside the radius, not at its edge, fits
    the neighbourhood better by at least ``min_gain`` per window sample); "uncovered" (less than ``min_cover`` of the cue
    meets reference speech at the applied lag); "ok"."""
    out = []
    for r in reports:
        if r.empty:
            out.append("empty")
        elif r.silent:
            out.append("silent")
        elif r.best_delta != 0 and r.gain >= min_gain * (r.hi - r.lo) and not r.at_edge:
            out.append("shifted")
        elif r.cover < min_cover:
            out.append("uncovered")
        else:
            out.append("ok")
    return out


def snap_cues(cue_start_us, cue_end_us, reports: Sequence[CueReport], verdicts: Sequence[str],
              sample_rate: int = SAMPLE_RATE):
    """Copies of the cue times with every "shifted" cue moved by best_delta / sample_rate seconds (each on its own: no
    joint choice, no order constraint); nothing else moves."""
    out_s = np.array(cue_start_us, dtype=np.int64, copy=True)
    out_e = np.array(cue_end_us, dtype=np.int64, copy=True)
    if not out_s.size == out_e.size == len(reports) == len(verdicts):
        raise ValueError("one report and one verdict per cue")
    for i, (r, v) in enumerate(zip(reports, verdicts)):
        if v == "shifted":
            move = int(round(r.best_delta * 10 ** 6 / float(sample_rate)))
            out_s[i] += move
            out_e[i] += move
    return out_s, out_e
