"""TEST INFRASTRUCTURE ONLY -- an independent reference for the optimum the split aligners promise
(ffsubsync_amd/split_align.py, ffsubsync_amd/cut_align.py).

The models next to the kernels (split_model, cut_model, ...) copy the kernels' lag-state DP step for step, so a mistake
they share goes unseen.  This module shares nothing with them: no block counts, no prefix popcounts, no score
expression, no lag-state recurrence.  It computes

    objective(o) = sum_b m_b(o_b) - P * #{b : o_b != o_(b-1)}

from its definition and finds its maximum over piece structures instead of over lag states:

  - slice correlation: I(a, e)[d] = sum over i in [a, e) with 0 <= i + d < R of s'(i) * r'(i + d), s' = 2 * level - 1
    of each vector's two levels (samples outside the reference are absent: a lag with no overlap scores 0), by direct
    sums, or for large problems with integer mapped levels by a float64 FFT rounded to integers;
  - segment DP: M(a, c) = max_d I(aK, min(cK, S))[d] over blocks [a, c); best[0] = 0 and
    best[c] = max over a < c of best[a] + M(a, c) - (P if a > 0 else 0); the optimum is best[B].  Exact because in an
    optimal path every maximal run of equal offsets sits at an argmax of its own slice (two adjacent runs at one lag
    lose to their merge);
  - a small enumerator of all L^B lag paths, the check of the segment DP itself.

With integer mapped levels every I is an integer, so totals compare exactly for dyadic P; otherwise use ``tolerance``.
"""
import itertools
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
DIRECT_CELLS = 1 << 21  # slice length x lags up to which I is summed directly


def mapped(bits, levels):
    """s'(i) = 2 * level - 1 of the sample's level: levels[1] where the bit is set, levels[0] elsewhere."""
    lo, hi = 2.0 * float(levels[0]) - 1.0, 2.0 * float(levels[1]) - 1.0
    return np.where(np.asarray(bits) != 0, hi, lo)


def integer_levels(*level_sets):
    """True when every level maps to an integer (then every correlation is an integer)."""
    return all(float(2.0 * float(x) - 1.0).is_integer() for lv in level_sets for x in lv)


def slice_corr(s_map, r_map, a, e, lag_lo, lag_hi, integer=None):
    """I(a, e)[d] for d in [lag_lo, lag_hi] (float64 array of lag_hi - lag_lo + 1 values)."""
    s_map = np.asarray(s_map, dtype=np.float64)
    r_map = np.asarray(r_map, dtype=np.float64)
    a, e, lag_lo, lag_hi = int(a), int(e), int(lag_lo), int(lag_hi)
    n, L, R = e - a, lag_hi - lag_lo + 1, r_map.size
    out = np.zeros(L, dtype=np.float64)
    if n <= 0 or L <= 0:
        return out
    # reference samples a + lag_lo + t, t in [0, n + L - 1): every (i, d) of the slice and the lag set
    p0 = a + lag_lo
    lo, hi = max(p0, 0), min(p0 + n + L - 1, R)
    if hi <= lo:
        return out  # no overlap at any lag
    win = np.zeros(n + L - 1, dtype=np.float64)
    win[lo - p0:hi - p0] = r_map[lo:hi]
    x = s_map[a:e]
    if integer is None:
        integer = bool(np.all(x == np.rint(x)) and np.all(win == np.rint(win)))
    if n * L <= DIRECT_CELLS or not integer:
        view = np.lib.stride_tricks.sliding_window_view(win, n)  # view[j] = win[j:j + n]
        step = max(1, DIRECT_CELLS // n)
        for j0 in range(0, L, step):
            out[j0:j0 + step] = view[j0:j0 + step] @ x
        return out
    size = 1 << int(math.ceil(math.log2(n + L - 1)))
    c = np.fft.irfft(np.fft.rfft(win, size) * np.conj(np.fft.rfft(x, size)), size)[:L]
    rounded = np.rint(c)
    err = float(np.max(np.abs(c - rounded)))
    assert err <= 1e-3, "FFT correlation %.3g away from an integer" % err
    return rounded


class Reference:
    """One problem over the lag set [lag_lo, lag_hi]: block rows I_b = I(bK, min((b+1)K, S)), interval rows I(a, c)
    (blocks [a, c)) and M(a, c) of every interval.

    The sum is grouped by the subtitle's level: I = s'_1 * C_1 + s'_0 * C_0, C_x = sum of r'(i + d) over the samples at
    level x, an integer correlation (the reference's mapped levels must be integers).  Interval rows come from prefix
    sums of the integer block rows of C_1 and C_0, so every I is exact for integer levels and within three roundings
    of the real sum otherwise."""

    def __init__(self, ref01, sub01, ref_levels, sub_levels, block_samples, lag_lo, lag_hi):
        self.r = mapped(ref01, ref_levels)
        self.s = mapped(sub01, sub_levels)
        assert integer_levels(ref_levels), "the reference's mapped levels must be integers"
        self.K, self.lo, self.hi = int(block_samples), int(lag_lo), int(lag_hi)
        self.S, self.R = self.s.size, self.r.size
        self.B = (self.S + self.K - 1) // self.K
        self.L = self.hi - self.lo + 1
        self.exact = integer_levels(ref_levels, sub_levels)
        self.levels = (2.0 * float(sub_levels[0]) - 1.0, 2.0 * float(sub_levels[1]) - 1.0)
        hi_bits = (np.asarray(sub01) != 0).astype(np.float64)
        self.prefix = []
        for ind in (1.0 - hi_bits, hi_bits):  # C_0, C_1
            rows = np.stack([slice_corr(ind, self.r, b * self.K, min((b + 1) * self.K, self.S), self.lo, self.hi, True)
                             for b in range(self.B)])
            pre = np.zeros((self.B + 1, self.L), dtype=np.float64)
            np.cumsum(rows, axis=0, out=pre[1:])  # integers below 2^53: exact
            self.prefix.append(pre)
        self.rows = np.stack([self.interval(b, b + 1) for b in range(self.B)])
        self._M = None
        # bound of |sum of the products| of any slice at any lag: the scale of fp64 rounding on the tolerance path
        self.abs_terms = float(np.sum(np.abs(self.s))) * float(np.max(np.abs(self.r)))

    @property
    def M(self):
        """M(a, c) of every interval, built on first use (the report reference needs the rows alone)."""
        if self._M is None:
            self._M = np.full((self.B + 1, self.B + 1), -np.inf)
            for a in range(self.B):
                for c in range(a + 1, self.B + 1):
                    self._M[a, c] = float(np.max(self.interval(a, c)))
        return self._M

    def lag_index(self, d):
        return int(d) - self.lo

    def interval(self, a, c):
        """I(aK, min(cK, S)) over the lag set."""
        (p0, p1), (l0, l1) = self.prefix, self.levels
        return l1 * (p1[c] - p1[a]) + l0 * (p0[c] - p0[a])

    def at(self, a, c, d):
        """I(aK, min(cK, S))[d]; 0 for a lag outside the lag set is an error, not a value."""
        j = self.lag_index(d)
        assert 0 <= j < self.L, (d, self.lo, self.hi)
        return float(self.interval(a, c)[j])

    def best(self, penalty):
        return segment_dp(self.M, self.B, penalty)

    def tolerance(self, penalty):
        """8 eps B sum|terms|, sum|terms| including the penalties a path can pay (only splits that gain can be taken,
        so at most 2 sum|products| of penalty per split); 0 on the exact path."""
        if self.exact:
            return 0.0
        p = float(penalty)
        pen = min(p, 2.0 * self.abs_terms) if math.isfinite(p) else 0.0
        return 8.0 * EPS * self.B * (self.abs_terms + pen * max(self.B - 1, 0))


def segment_dp(M, n_blocks, penalty):
    """(best[0..B], pieces of one optimal structure as (a, c) block intervals) of the piece-structure DP over M."""
    p = float(penalty)
    best = np.full(n_blocks + 1, -np.inf)
    back = np.zeros(n_blocks + 1, dtype=np.int64)
    best[0] = 0.0
    for c in range(1, n_blocks + 1):
        for a in range(c):
            v = best[a] + M[a, c]
            if a > 0:
                v = v - p  # a conditional: P = inf must not meet 0 * inf
            if v > best[c]:
                best[c], back[c] = v, a
    pieces, c = [], n_blocks
    while c > 0:
        pieces.append((int(back[c]), c))
        c = int(back[c])
    return best, pieces[::-1]


def path_objective(rows, path, penalty):
    """objective of one lag-index path over block rows [B, L]: sum of the blocks' values, minus P per change."""
    total = 0.0
    for b, j in enumerate(path):
        total += float(rows[b, j])
    switches = sum(1 for b in range(1, len(path)) if path[b] != path[b - 1])
    return total - float(penalty) * switches if switches else total


def enumerate_optimum(rows, penalty, limit=50000):
    """(max objective, every optimal path as a tuple of lag indices) over all L^B paths of block rows [B, L]."""
    B, L = rows.shape
    assert L ** B <= limit, (L, B)
    paths = np.array(list(itertools.product(range(L), repeat=B)), dtype=np.int64).reshape(-1, B)
    vals = rows[np.arange(B), paths].sum(axis=1)
    switches = (paths[:, 1:] != paths[:, :-1]).sum(axis=1) if B > 1 else np.zeros(len(paths), np.int64)
    p = float(penalty)
    obj = vals - p * switches if math.isfinite(p) else np.where(switches > 0, -np.inf, vals)
    top = float(obj.max())
    return top, [tuple(int(x) for x in row) for row in paths[obj == top]]


def pieces_of(block_offsets):
    """[(first_block, end_block, offset)] of the maximal runs of equal block offsets."""
    o = [int(x) for x in block_offsets]
    out, b0 = [], 0
    for b in range(1, len(o) + 1):
        if b == len(o) or o[b] != o[b0]:
            out.append((b0, b, o[b0]))
            b0 = b
    return out


def check_solution(ref, penalty, block_offsets, total, block_scores=None, pieces=None):
    """Problems with a solver's answer against the reference (empty list = none):
      1. total == best[B] (within ``ref.tolerance``);
      2. every piece [a, c) has its offset in the lag set and I(a, c)[o] == M(a, c);
      3. pieces cover every block, adjacent pieces differ, sum I(piece)[o] - P (n_pieces - 1) == total;
      4. block_scores[b] == I_b at block_offsets[b] (when given);
    ``pieces`` (when given): [(first_block, end_block, offset, score)] as the solver reports them, each score
    == I(a, c)[o]."""
    bad = []
    tol = ref.tolerance(penalty)
    best, _ = ref.best(penalty)
    want = float(best[ref.B])
    if not abs(float(total) - want) <= tol:
        bad.append(("total", float(total), want, tol))
    offs = [int(x) for x in block_offsets]
    if len(offs) != ref.B:
        return bad + [("blocks", len(offs), ref.B)]
    runs = pieces_of(offs)
    acc = 0.0
    for a, c, o in runs:
        if not ref.lo <= o <= ref.hi:
            bad.append(("offset outside the lag set", a, c, o))
            continue
        v = ref.at(a, c, o)
        acc += v
        if not abs(v - ref.M[a, c]) <= tol:
            bad.append(("piece not at its slice's maximum", a, c, o, v, float(ref.M[a, c])))
    if not bad:
        split_cost = float(penalty) * (len(runs) - 1) if len(runs) > 1 else 0.0
        if not abs(acc - split_cost - float(total)) <= tol:
            bad.append(("path objective != total", acc - split_cost, float(total)))
    if block_scores is not None:
        for b, o in enumerate(offs):
            if ref.lo <= o <= ref.hi and not abs(float(block_scores[b]) - float(ref.rows[b, ref.lag_index(o)])) <= tol:
                bad.append(("block score", b, o, float(block_scores[b]), float(ref.rows[b, ref.lag_index(o)])))
    if pieces is not None:
        if [(p[0], p[1], p[2]) for p in pieces] != runs:
            bad.append(("pieces", [(p[0], p[1], p[2]) for p in pieces], runs))
        else:
            for a, c, o, score in pieces:
                if ref.lo <= o <= ref.hi and not abs(float(score) - ref.at(a, c, o)) <= tol:
                    bad.append(("piece score", a, c, o, float(score), ref.at(a, c, o)))
    return bad


def tie_penalty(ref):
    """The exact gain of the best two-piece split over one piece, max_c M(0, c) + M(c, B) - M(0, B), when at that
    penalty no other structure beats the tie (one piece and that split both reach best[B]); None otherwise."""
    if ref.B < 2:
        return None
    one = float(ref.M[0, ref.B])
    two = max(float(ref.M[0, c] + ref.M[c, ref.B]) for c in range(1, ref.B))
    p = two - one
    if not p > 0:
        return None
    best, _ = ref.best(p)
    return p if float(best[ref.B]) == one == two - p else None


def two_offset_bits(rng, R, S, shifts, flip=0.08, run=40.0, cut=None):
    """Problems for the tests (not part of the reference): two-level bits, a reference of random runs and a subtitle
    that follows it at shifts[0] before a cut (random unless given) and at shifts[1] after it, a fraction ``flip`` of
    its samples inverted; both levels present in both."""
    seg = np.maximum(1, rng.geometric(1.0 / run, size=R // 4 + 16))
    rb = np.repeat(rng.rand(seg.size) < 0.45, seg)[:R]
    rb = np.concatenate([rb, np.zeros(R - rb.size, bool)])
    cut = int(rng.randint(0, S + 1)) if cut is None else int(cut)
    idx = np.arange(S) + np.where(np.arange(S) < cut, shifts[0], shifts[1])
    sb = np.zeros(S, bool)
    ok = (idx >= 0) & (idx < R)
    sb[ok] = rb[idx[ok]]
    sb ^= rng.rand(S) < flip
    if S >= 2:
        sb[0], sb[1] = True, False
    rb[0], rb[1] = True, False
    return rb, sb
