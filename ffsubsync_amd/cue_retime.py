"""Joint cue retiming: one order-preserving residual shift per cue, chosen together.

The per-cue report (``cue_report.py``) decides each cue alone: a stretch of lines a re-edit moved together
is a handful of ambiguous decisions, a cue whose best lag sits at a neighbour's speech is snapped to the neighbour's
line, and two snapped cues can swap order.  This module makes the joint choice (``csrc/ffs_cue_retime.h``):
a Viterbi pass over (cue x residual shift) whose node score is the integer agreement of the cue's neighbourhood at that
shift and whose links charge ``penalty_q`` per sample of change of shift between consecutive cues (at most ``jump_q``
per link), with the cues kept in order.  The pair's levels do not enter: everything is exact integer arithmetic.

``retime_batch`` is the device call, ``retime_sync`` runs it behind any sync result, ``apply_retime`` moves the cues.
The table order is the chain order: pass cues in file order.

Parity is against the in-repo numpy model ``tests/retime_model.py``, bit for bit.  No existing entry point changes.
"""
from dataclasses import dataclass
from typing import Sequence

import numpy as np

from . import _native
from .constants import SAMPLE_RATE
from .cue_report import _get_plan, cue_table, flat_cue_table, validate_args as _validate_report_args
from .side_call import bits_batch, check_two_level_batch
from .split_align import empty_error

# Chosen on the CPU model (profiles/cue_retime_calibration.py -> profiles/cue_retime_calibration.json;
# synthetic data only, nobody has measured real files)
DEFAULT_RADIUS = 300
DEFAULT_CONTEXT = 0
DEFAULT_PENALTY_Q = 256
DEFAULT_JUMP_Q = 64 * 150


@dataclass
class RetimedCue:
    start: int  # the cue as given: subtitle samples [start, end) and the lag the sync applied
    end: int
    lag: int
    delta: int  # the residual shift chosen for the cue (samples); 0 for a skipped cue
    flags: int  # _native.RETIME_*
    own: int  # agreement of the cue's neighbourhood at the applied lag
    at: int  # ... at lag + delta
    best: int  # ... at the cue's own best shift, lag + best_delta
    best_delta: int
    link: int  # what the link into this cue cost, in 64ths of a sample of agreement

    @property
    def skipped(self) -> bool:
        return bool(self.flags & (_native.RETIME_EMPTY | _native.RETIME_INVALID))

    @property
    def moved(self) -> bool:
        return bool(self.flags & _native.RETIME_MOVED)

    @property
    def jump(self) -> bool:
        return bool(self.flags & _native.RETIME_JUMP)

    @property
    def at_edge(self) -> bool:
        return bool(self.flags & _native.RETIME_AT_EDGE)


@dataclass
class RetimeSummary:
    total: int  # the chain's score in 64ths: 64 * sum(at) - sum(link)
    own_total: int  # 64 * sum(own): the score of moving nothing
    best_total: int  # 64 * sum(best): the bound of every cue at its own best shift for free
    n_live: int
    n_moved: int
    n_jumps: int


def from_record(rec) -> RetimedCue:
    """RetimedCue of one ``_native.CUE_RETIME_DTYPE`` record (or of a model record with the same fields)."""
    return RetimedCue(int(rec["start"]), int(rec["end"]), int(rec["lag"]), int(rec["delta"]), int(rec["flags"]),
                      int(rec["own"]), int(rec["at"]), int(rec["best"]), int(rec["best_delta"]), int(rec["link"]))


def summary_from_record(rec) -> RetimeSummary:
    return RetimeSummary(int(rec["total"]), int(rec["own_total"]), int(rec["best_total"]), int(rec["n_live"]),
                         int(rec["n_moved"]), int(rec["n_jumps"]))


def validate_args(radius, context, penalty_q, jump_q) -> None:
    """Host-side checks of the call parameters (ValueError before any native call)."""
    r = int(radius)
    if r != radius or not 0 <= r <= _native.RETIME_MAX_RADIUS:
        raise ValueError("radius=%r: need an integer in [0, %d]" % (radius, _native.RETIME_MAX_RADIUS))
    _validate_report_args(0, context)
    q = int(penalty_q)
    if q != penalty_q or not 0 <= q <= _native.RETIME_MAX_PENALTY_Q:
        raise ValueError("penalty_q=%r: need an integer in [0, 2^20] (64ths of a sample of agreement per sample of shift)"
                         % (penalty_q,))
    j = int(jump_q)
    if j != jump_q or not (j == _native.RETIME_NO_JUMP or 0 <= j <= _native.RETIME_MAX_JUMP_Q):
        raise ValueError("jump_q=%r: need -1 (no cap) or an integer in [0, 2^40]" % (jump_q,))


def workspace_bytes(cue_counts, radius: int, pairs_in_flight: int) -> int:
    """Bytes of retime workspace ``ffs_cue_retime_batch`` needs for pairs with these cue counts: 6 bytes per (cue,
    shift) of the largest sub-batch (the header's cutting rule), rounded up to 256."""
    n_delta, need, p, counts = 2 * int(radius) + 1, 0, 0, [int(c) for c in cue_counts]
    while p < len(counts):
        rows, n = 0, 0
        while p + n < len(counts) and n < pairs_in_flight:
            if n and (rows + counts[p + n]) * n_delta * _native.RETIME_CELL_BYTES > _native.RETIME_WORK_CAP:
                break
            rows += counts[p + n]
            n += 1
        need = max(need, -(-rows * n_delta * _native.RETIME_CELL_BYTES // 256) * 256)
        p += n
    return need


def retime_batch(batch, cues, radius: int = DEFAULT_RADIUS, context: int = DEFAULT_CONTEXT,
                 penalty_q: int = DEFAULT_PENALTY_Q, jump_q: int = DEFAULT_JUMP_Q, keep_order: bool = True,
                 raw: bool = False, plan=None):
    """Joint retiming of every pair of a ``batch.DeviceBatch`` with ONE candidate per pair.  ``cues``: one (start, end,
    lag) triple of int64 arrays per pair, in file order (``cue_report.cue_table``).  Returns (one list of ``RetimedCue``
    per pair, one ``RetimeSummary`` per pair), or with ``raw`` (the ``_native.CUE_RETIME_DTYPE`` records of the flat
    table, the per-pair slices into it, the ``_native.RETIME_SUMMARY_DTYPE`` records)."""
    validate_args(radius, context, penalty_q, jump_q)
    check_two_level_batch(batch, "retime_batch", float_ref_message=True)
    n = batch.n_pairs
    table, first, count = flat_cue_table(cues, n)
    for p, c in enumerate(count):
        if int(c) * (2 * int(radius) + 1) * _native.RETIME_CELL_BYTES > _native.RETIME_WORK_CAP:
            raise ValueError("pair %d: %d cues x %d shifts x 6 bytes exceed the retime workspace cap of %d bytes"
                             % (p, int(c), 2 * int(radius) + 1, _native.RETIME_WORK_CAP))
    slices = [slice(int(f), int(f + c)) for f, c in zip(first, count)]
    torch = _native.require_gpu()
    batch = bits_batch(batch)
    dev = batch.data.device
    cue_dev = torch.from_numpy(table.view(np.uint8).reshape(-1)).to(dev)
    rec_out = torch.empty(table.size * _native.CUE_RETIME_BYTES, dtype=torch.uint8, device=dev)
    sum_out = torch.empty(n * _native.RETIME_SUMMARY_BYTES, dtype=torch.uint8, device=dev)
    plan = _get_plan(n) if plan is None else plan
    plan.cue_retime(*batch.pair_arrays(), cue_dev, first, count, int(radius), int(context), int(penalty_q), int(jump_q),
                    _native.RETIME_KEEP_ORDER if keep_order else 0, rec_out, sum_out)
    recs = rec_out.cpu().numpy().view(_native.CUE_RETIME_DTYPE)
    sums = sum_out.cpu().numpy().view(_native.RETIME_SUMMARY_DTYPE)
    if raw:
        return recs, slices, sums
    return [[from_record(x) for x in recs[sl]] for sl in slices], [summary_from_record(x) for x in sums]


def retime_sync(problems, results, radius: int = DEFAULT_RADIUS, context: int = DEFAULT_CONTEXT,
                penalty_q: int = DEFAULT_PENALTY_Q, jump_q: int = DEFAULT_JUMP_Q, keep_order: bool = True,
                sample_rate: int = SAMPLE_RATE, raw: bool = False):
    """Joint retiming behind any sync: ``problems`` as the sync took them ((reference, (start_us, end_us, is_metadata))
    pairs, the cues in file order), ``results`` its outputs (anything with ``ratio``, ``cue_start_us`` and
    ``cue_end_us``).  Each track is rasterised once at its result's ratio, the tables come from
    ``cue_report.cue_table``, and one device call retimes every file.  Returns as ``retime_batch``."""
    from . import batch as batch_mod
    from .subtitle_raster import DeviceRaster, rasterize_candidates

    validate_args(radius, context, penalty_q, jump_q)
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
                raise ValueError("retime_sync needs two-level references: reference %d is a multi-level float "
                                 "reference, which is not supported" % p)
            _native.require_gpu()
            ref = DeviceRaster.from_host(host, lists=False)
        elif ref.n == 0:
            raise empty_error(0, 1)
        sub = rasterize_candidates(start_us, end_us, meta, [res.ratio], sample_rate)[0]
        pairs.append((ref, [sub]))
        tables.append(cue_table(start_us, end_us, res.ratio, res.cue_start_us, sample_rate, meta, sub.n))
    return retime_batch(batch_mod.pack_pairs(pairs), tables, radius, context, penalty_q, jump_q, keep_order, raw)


def apply_retime(cue_start_us, cue_end_us, records: Sequence, sample_rate: int = SAMPLE_RATE):
    """Copies of the cue times with EVERY live cue moved by delta / sample_rate seconds (``records``: ``RetimedCue``s or
    raw records; a skipped cue has delta 0 and stays)."""
    out_s = np.array(cue_start_us, dtype=np.int64, copy=True)
    out_e = np.array(cue_end_us, dtype=np.int64, copy=True)
    if not out_s.size == out_e.size == len(records):
        raise ValueError("one record per cue")
    for i, r in enumerate(records):
        delta = int(r.delta) if isinstance(r, RetimedCue) else int(r["delta"])
        move = int(round(delta * 10 ** 6 / float(sample_rate)))
        out_s[i] += move
        out_e[i] += move
    return out_s, out_e
