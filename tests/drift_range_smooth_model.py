"""TEST INFRASTRUCTURE ONLY -- numpy model of the smooth drift fit over a lag range (csrc/ffs_drift_range_smooth.h,
ffsubsync_amd.drift_range_smooth): the contract the device is held to, bit for bit.

It is ``drift_range_model.solve`` followed by ``drift_smooth_model.fit`` with ONE change: a knot candidate
c_i = o_{k_i} + u is valid where lag_lo <= c_i <= lag_hi instead of -W + 1 <= c_i <= W.  ``fit`` reads three members of
its counts object -- ``valid``, ``block_terms``, ``coeffs`` -- and ``RangeCounts`` supplies them for a range: ``valid`` is
the range test, ``block_terms`` are the range path's (``cut_model._Pair``: absent samples, lags without overlap
contribute nothing) with n11 counted directly at the few lags asked for, no [B, L] table anywhere.

``band_row`` / ``band_of`` restate the bound the device's band rows rest on: every lag a line of interval i visits lies
in [min(o_k, o_{k+n}) - R, max(o_k, o_{k+n}) + R], at most max_step * ceil(3M / 2) + 2R + 1 lags inside a segment.
"""
import numpy as np

import drift_range_model as drg
import drift_report_model as drm
import drift_smooth_model as dsm
from cut_model import _Pair


class RangeCounts:
    """What ``drift_smooth_model.fit`` reads, over the lag range [lag_lo, lag_hi]."""

    def __init__(self, rb, sb, ref_levels, sub_levels, block_samples, lag_lo, lag_hi):
        self.pair = _Pair(rb, sb, ref_levels, sub_levels, block_samples, lag_lo, lag_hi)
        self.lo, self.hi = int(lag_lo), int(lag_hi)
        self.k, self.R, self.S = self.pair.k, self.pair.R, self.pair.S
        self.coeffs = drm._coeffs(ref_levels, sub_levels)
        self.n_blocks = self.pair.n_blocks
        self.visited = None  # a list: block_terms appends (block, lags) of every call (the band test)

    def valid(self, lag):
        return (lag >= self.lo) & (lag <= self.hi)

    def n11_at(self, b, lag):
        """n11 of block b at the lags ``lag`` (any shape), counted from the block's runs of ones against the reference's
        prefix popcounts: samples outside the reference are absent."""
        p = self.pair
        blk = p.s[b * p.k:(b + 1) * p.k]
        edges = np.flatnonzero(np.diff(np.concatenate([[0], blk, [0]]))) + b * p.k
        out = np.zeros(np.shape(lag), dtype=np.int64)
        for u, v in zip(edges[0::2], edges[1::2]):
            out += p._pr_at(v + lag) - p._pr_at(u + lag)
        return out

    def block_terms(self, b, lag):
        """(ov, n11, n1x, nx1) of block b at the lags ``lag`` (int64 array), as ``cut_model._Pair.scores`` forms them."""
        p = self.pair
        lag = np.asarray(lag, dtype=np.int64)
        if self.visited is not None:
            self.visited.append((b, lag.copy()))
        blo, bhi = b * p.k, min((b + 1) * p.k, p.S)
        a = np.maximum(blo, -lag)
        e = np.minimum(bhi, p.R - lag)
        ok = e > a
        a = np.where(ok, a, 0)
        e = np.where(ok, e, 0)
        n11 = np.where(ok, self.n11_at(b, lag), 0)
        nx1 = np.where(ok, p._pr_at(e + lag) - p._pr_at(a + lag), 0)
        return e - a, n11, p.ps[e] - p.ps[a], nx1


def band_row(max_step, knot_blocks, radius):
    """Cells of one block's band row (``range_band_row`` of csrc/ffs_drift_range_smooth.h)."""
    return int(max_step) * ((3 * int(knot_blocks) + 1) // 2) + 2 * int(radius) + 1


def band_of(offsets, k0, n, radius):
    """(first lag, width) of the band of the interval with knots at blocks k0 and k0 + n."""
    o0, o1 = int(offsets[k0]), int(offsets[k0 + n])
    return min(o0, o1) - int(radius), abs(o1 - o0) + 2 * int(radius) + 1


def intervals_of(jump, knot_blocks):
    """[(k0, n, last)] of every interval of every segment, in block order."""
    out = []
    for f, e in drm.segments_of(jump):
        ks = dsm.knots_of(f, e, knot_blocks)
        out += [(ks[i], ks[i + 1] - ks[i], i == len(ks) - 2) for i in range(len(ks) - 1)]
    return out


def fit(cnt, offsets, jump, knot_blocks, radius, bend_cost, table_cache=None):
    """``drift_smooth_model.fit`` over a ``RangeCounts``."""
    return dsm.fit(cnt, offsets, jump, knot_blocks, radius, bend_cost, table_cache)


def solve(rb, sb, ref_levels, sub_levels, block_samples, lag_lo, lag_hi, split_penalty, max_step, step_cost, knot_blocks,
          radius, bend_cost, drift=None):
    """((block offsets, block scores, jump flags, total) of drift_range_model.solve, smooth offsets, knot flags, records).
    ``drift``: that solve's result where the caller has it already."""
    if drift is None:
        drift = drg.solve(rb, sb, ref_levels, sub_levels, block_samples, lag_lo, lag_hi, split_penalty, max_step, step_cost)
    cnt = RangeCounts(rb, sb, ref_levels, sub_levels, block_samples, lag_lo, lag_hi)
    smooth, knot, recs = fit(cnt, drift[0], drift[2], knot_blocks, radius, bend_cost)
    return drift, smooth, knot, recs
