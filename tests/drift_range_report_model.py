"""TEST INFRASTRUCTURE ONLY -- numpy model of the per-segment path report of a drift solve over any lag range
[lag_lo, lag_hi] (csrc/ffs_drift_range_report.h, ffsubsync_amd.drift_range_report): the contract the device is held to,
bit for bit.  It is tests/drift_report_model.py's contract with the lag set d = lag_lo + j, j in [0, L):

Per segment i (a maximal run [f, e) of blocks with no jump inside, block offsets o_b, o_min / o_max over them):
  - shift set delta in [lag_lo - o_min, lag_hi - o_max] (n_lags = L - (o_max - o_min) shifts, shift index t puts block b
    at the lag lag_lo + t + (o_b - o_min))
  - path curve: OV, N11, N1X, NX1 summed over the segment's blocks as exact integers -- block b at lag d contributes the
    samples [max(bK, -d), min((b+1)K, S, R-d)) -- then ONE split_mix expression, exactly 0.0 where OV = 0
  - moments in the device's summation order and greedy peaks (split_report_model's helpers), own / prev / next, and the
    flat maximum over d in [o_min, o_max] of the constant-lag piece curve, the largest d on ties.

The model streams and holds no B x L table: n11 of a RUN of consecutive blocks that share one offset is taken at all
shifts at once from the runs [u, v) of the stretch's set subtitle bits on the reference's prefix popcounts, as
tests/cut_report_model.py does for a piece.  A run is exact as one unit because the per-block sample ranges of
consecutive blocks at one lag concatenate; ``by_block=True`` sums block by block instead (the statement of the contract),
and tests/test_drift_range_report_host.py holds the two equal.
"""
import numpy as np

import cut_report_model as crm
import drift_range_model as drgm
import drift_report_model as drm
import split_report_model as srm
from ffsubsync_amd import _native

FLAT = srm.FLAT
OWN_NOT_PEAK = drm.OWN_NOT_PEAK


class Bits:
    """The two bit vectors with their prefix popcounts."""

    def __init__(self, rb, sb):
        self.r = (np.asarray(rb) != 0).astype(np.int64)
        self.s = (np.asarray(sb) != 0).astype(np.int64)
        self.R, self.S = self.r.size, self.s.size
        self.pr = np.concatenate([[0], np.cumsum(self.r)])
        self.ps = np.concatenate([[0], np.cumsum(self.s)])


def runs_of(offsets, first_block, end_block, by_block=False):
    """[(first block, end block, offset)] of the maximal stretches of equal offsets inside [first_block, end_block)."""
    o = np.asarray(offsets, dtype=np.int64)
    out, b0 = [], first_block
    for b in range(first_block + 1, end_block + 1):
        if b == end_block or by_block or o[b] != o[b0]:
            out.append((b0, b, int(o[b0])))
            b0 = b
    return out


def stretch_n11(bits, lo, hi, lag):
    """n11 of subtitle samples [lo, hi) at the lags ``lag`` (int64 array), exact."""
    blk = bits.s[lo:hi]
    edges = np.flatnonzero(np.diff(np.concatenate([[0], blk, [0]])))
    out = np.zeros(lag.size, dtype=np.int64)
    for u, v in zip(edges[0::2] + lo, edges[1::2] + lo):
        out += bits.pr[np.clip(v + lag, 0, bits.R)] - bits.pr[np.clip(u + lag, 0, bits.R)]
    return out


def path_sums(bits, block_samples, lag_lo, lag_hi, first_block, end_block, offsets, by_block=False):
    """(ov, n11, n1x, nx1) int64 over the shift set of the blocks [first_block, end_block)."""
    k = int(block_samples)
    o = np.asarray(offsets, dtype=np.int64)[first_block:end_block]
    o_min, o_max = int(o.min()), int(o.max())
    n = (int(lag_hi) - int(lag_lo) + 1) - (o_max - o_min)
    t = np.arange(n, dtype=np.int64)
    ov, n11, n1x, nx1 = (np.zeros(n, np.int64) for _ in range(4))
    for f, e, ob in runs_of(offsets, first_block, end_block, by_block):
        lag = t + (int(lag_lo) + ob - o_min)
        rlo, rhi = f * k, min(e * k, bits.S)
        a = np.maximum(rlo, -lag)
        z = np.minimum(rhi, bits.R - lag)
        ok = z > a
        a = np.where(ok, a, 0)
        z = np.where(ok, z, 0)
        ov += z - a
        n11 += stretch_n11(bits, rlo, rhi, lag)  # 0 where nothing overlaps: the partners are clipped to the reference
        n1x += bits.ps[z] - bits.ps[a]
        nx1 += np.where(ok, bits.pr[np.clip(z + lag, 0, bits.R)] - bits.pr[np.clip(a + lag, 0, bits.R)], 0)
    return ov, n11, n1x, nx1


def path_curve(bits, ref_levels, sub_levels, block_samples, lag_lo, lag_hi, first_block, end_block, offsets,
               by_block=False):
    """p(delta) over the shift set of the blocks [first_block, end_block)."""
    ov, n11, n1x, nx1 = path_sums(bits, block_samples, lag_lo, lag_hi, first_block, end_block, offsets, by_block)
    return drm._mix(ov, n11, n1x, nx1, drm._coeffs(ref_levels, sub_levels))


def report(rb, sb, ref_levels, sub_levels, block_samples, lag_lo, lag_hi, offsets, jump, top_k=3, exclusion_samples=300):
    """(SEGMENT_REPORT_DTYPE records of the segments of the path (``offsets``, ``jump``), their path curves)."""
    bits = Bits(rb, sb)
    k, lo_l, hi_l = int(block_samples), int(lag_lo), int(lag_hi)
    offsets = np.asarray(offsets, dtype=np.int64)
    if offsets.size != (bits.S + k - 1) // k or np.asarray(jump).size != offsets.size:
        raise ValueError("one offset and one jump flag per block")
    if offsets.min() < lo_l or offsets.max() > hi_l:
        raise ValueError("a block offset lies outside the lag range")
    segs = drm.segments_of(jump)
    recs = np.zeros(len(segs), dtype=_native.SEGMENT_REPORT_DTYPE)
    curves = []
    for i, (f, e) in enumerate(segs):
        o = offsets[f:e]
        o_min, o_max = int(o.min()), int(o.max())
        d_lo, d_hi = lo_l - o_min, hi_l - o_max
        c = path_curve(bits, ref_levels, sub_levels, k, lo_l, hi_l, f, e, offsets)
        curves.append(c)
        lo, hi = f * k, min(e * k, bits.S)
        mean, std, flags = srm.moments(c)
        pk = drm.shift_peaks(c, d_lo, top_k, exclusion_samples)
        qs = crm.piece_curve(rb, sb, ref_levels, sub_levels, lo, hi, o_min, o_max)
        flat_j = qs.size - 1 - int(np.argmax(qs[::-1]))

        def at(delta):
            return c[delta - d_lo] if d_lo <= delta <= d_hi else np.nan

        rec = recs[i]
        rec["first_block"], rec["end_block"], rec["start_sample"], rec["end_sample"] = f, e, lo, hi
        rec["first_offset"], rec["last_offset"], rec["min_offset"], rec["max_offset"] = int(o[0]), int(o[-1]), o_min, o_max
        rec["own_score"] = at(0)
        rec["prev_score"] = at(int(offsets[f - 1]) - int(o[0])) if i > 0 else np.nan
        rec["next_score"] = at(int(offsets[e]) - int(o[-1])) if i + 1 < len(segs) else np.nan
        rec["flat_score"], rec["flat_offset"] = qs[flat_j], o_min + flat_j
        rec["mean"], rec["std"], rec["n_lags"] = mean, std, c.size
        for z, (ps_, sh) in enumerate(pk):
            rec["peak_score"][z], rec["peak_shift"][z] = ps_, sh
        rec["n_peaks"] = len(pk)
        rec["flags"] = flags | (OWN_NOT_PEAK if not pk or pk[0][1] != 0 else 0)
    return recs, curves


def solve_report(rb, sb, ref_levels, sub_levels, block_samples, lag_lo, lag_hi, split_penalty, max_step, step_cost,
                 top_k=3, exclusion_samples=300):
    """((block offsets, block scores, jump flags, total) of drift_range_model.solve, records, curves)."""
    sol = drgm.solve(rb, sb, ref_levels, sub_levels, block_samples, lag_lo, lag_hi, split_penalty, max_step, step_cost)
    recs, curves = report(rb, sb, ref_levels, sub_levels, block_samples, lag_lo, lag_hi, sol[0], sol[2], top_k,
                          exclusion_samples)
    return sol, recs, curves
