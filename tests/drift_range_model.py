"""TEST INFRASTRUCTURE ONLY -- numpy model of the lag-range drift aligner (ffsubsync_amd/drift_range.py,
csrc/ffs_drift_range.h).

``cut_model._Pair``'s streamed block score rows (lag set d in [lag_lo, lag_hi], lag index j = d - lag_lo, absent
samples, the fp64 score operation by operation, lags without overlap 0) under ``drift_model``'s option loop: STAY, then
+1, -1, ..., +s, -s (block b-1 at lag index j - e, cost Q * a, one product), then JUMP to T = J_{b-1} - P; an option
replaces the best so far only when strictly greater; the largest lag index wins every maximum.  This model IS the
contract the device is held to, bit for bit.

The model streams: one score row and one value row at a time, the codes (0 STAY, 2a-1 = +a, 2a = -a, 2s+1 JUMP) packed
two per byte, so the full overlap range of a long pair fits in memory.  ``RowDP`` is the DP alone, fed row by row;
several of them can share one stream of rows (profiles/drift_range_calibration.py does).
"""
import numpy as np

from cut_model import _Pair, _last_argmax
from drift_model import validate


class RowDP:
    """The drift DP over score rows pushed in block order; ``finish`` backtracks."""

    def __init__(self, split_penalty, max_step, step_cost):
        self.s, q = validate(max_step, step_cost)
        self.pen = np.float64(split_penalty)
        self.cost = [q * np.float64(a) for a in range(self.s + 1)]  # c_a: one product each
        self.v = None
        self.codes = []  # codes[b - 1]: block b's row, two codes per byte (even lag index in the low nibble)
        self.arg = []  # arg[b]: the largest argmax of row b

    def push(self, m_row):
        m_row = np.asarray(m_row, dtype=np.float64)
        if self.v is None:
            self.v = m_row.copy()
            return
        v, n = self.v, self.v.size
        j = _last_argmax(v)
        self.arg.append(j)
        t = v[j] - self.pen
        best = v.copy()
        cd = np.zeros(n + (n & 1), dtype=np.uint8)
        for a in range(1, min(self.s, n - 1) + 1):  # smaller moves first, +a before -a
            cand = v[:n - a] - self.cost[a]  # e = +a: block b at j, block b-1 at j - a
            take = cand > best[a:]  # strict: ties keep the earlier option
            best[a:] = np.where(take, cand, best[a:])
            cd[a:n][take] = 2 * a - 1
            cand = v[a:] - self.cost[a]  # e = -a
            take = cand > best[:n - a]
            best[:n - a] = np.where(take, cand, best[:n - a])
            cd[:n - a][take] = 2 * a
        take = t > best  # strict: ties do not jump
        best = np.where(take, t, best)
        cd[:n][take] = 2 * self.s + 1
        self.codes.append(cd[0::2] | (cd[1::2] << 4))
        self.v = best + m_row

    def finish(self):
        """(block lag indices o[b] int64, jump flags [B] uint8, total)."""
        n_blocks = len(self.codes) + 1
        end = _last_argmax(self.v)
        total = self.v[end]
        o = np.zeros(n_blocks, dtype=np.int64)
        jump = np.zeros(n_blocks, dtype=np.uint8)
        o[-1] = end
        for b in range(n_blocks - 1, 0, -1):
            jb = int(o[b])
            c = (int(self.codes[b - 1][jb >> 1]) >> (4 * (jb & 1))) & 15
            if c == 2 * self.s + 1:
                jump[b] = 1
                o[b - 1] = self.arg[b - 1]
            elif c:
                a = (c + 1) >> 1
                o[b - 1] = jb - (a if c & 1 else -a)
            else:
                o[b - 1] = jb
        return o, jump, total


def dp_rows(m, split_penalty, max_step, step_cost):
    """(block lag indices, jump flags, total) of the drift DP over a [B, L] score table (or any iterable of rows)."""
    dp = RowDP(split_penalty, max_step, step_cost)
    for row in m:
        dp.push(row)
    return dp.finish()


def solve(ref01, sub01, ref_levels, sub_levels, block_samples, lag_lo, lag_hi, split_penalty, max_step, step_cost):
    """(block offsets in samples [B] int64, block scores m_b(o_b) [B], jump flags [B] uint8, total) of one problem over
    [lag_lo, lag_hi]."""
    p = _Pair(ref01, sub01, ref_levels, sub_levels, block_samples, lag_lo, lag_hi)
    o, jump, total = dp_rows((p.scores(b) for b in range(p.n_blocks)), split_penalty, max_step, step_cost)
    offsets = o + p.lo
    scores = np.array([p.scores(b, lag=[int(offsets[b])])[0] for b in range(p.n_blocks)], dtype=np.float64)
    return offsets, scores, jump, float(total)
