"""TEST INFRASTRUCTURE ONLY -- numpy model of the sample-exact jumps of a drift solve (csrc/ffs_drift_refine.h,
ffsubsync_amd.drift_refine): the contract the device is held to, bit for bit.

``split_refine_model`` with two changes.  The refined positions are the blocks f >= 1 with ``block_jump[f] != 0``
(whether or not the offset changes there), and the lags follow the path: for a subtitle sample x, b(x) = x // K,
  lag_a(x) = o[min(b(x), f - 1)],  lag_b(x) = o[max(b(x), f)]
A(t) = the score of the counts of [L, t) at lag_a(x), B(t) of [t, U) at lag_b(x); a sample whose partner x + lag(x) lies
outside the reference is absent.  Windows, N, F, G, the cut search, the flags and the records are split_refine_model's.
"""
import numpy as np

from ffsubsync_amd import _native
from split_refine_model import AT_EDGE, CLIPPED, UNMATCHED, _mix, constants, cut, windows  # noqa: F401


def jumps_of(block_jump):
    """Blocks f >= 1 with block_jump[f] != 0."""
    j = np.asarray(block_jump)
    return [int(b) for b in np.flatnonzero(j[1:] != 0) + 1]


def sample_lags(block_offsets, block_samples, f, lo, hi):
    """(lag_a, lag_b) int64 arrays over the samples lo .. hi - 1 of the jump at block f."""
    o = np.asarray(block_offsets, dtype=np.int64)
    b = np.arange(lo, hi, dtype=np.int64) // int(block_samples)
    return o[np.minimum(b, f - 1)], o[np.maximum(b, f)]


def _prefix_counts(r, s, lo, hi, lag):
    """(ov, n11, n1x, nx1) over [lo, t) for t = lo .. hi at the per-sample lags ``lag``."""
    R = r.size
    i = np.arange(lo, hi, dtype=np.int64)
    pres = (i + lag >= 0) & (i + lag < R)
    rv = np.zeros(i.size, bool)
    rv[pres] = r[(i + lag)[pres]]
    sv = s[lo:hi]
    cs = lambda x: np.concatenate([[0], np.cumsum(x.astype(np.int64))])
    return cs(pres), cs(sv & rv), cs(sv & pres), cs(rv)


def curves(rb, sb, ref_levels, sub_levels, lo, hi, block_offsets, block_samples, f, beta):
    """(A, B, N) over t = lo .. hi for the jump at block f."""
    r, s = np.asarray(rb) != 0, np.asarray(sb) != 0
    c, z0, z1 = constants(r, ref_levels, sub_levels, beta)
    la, lb = sample_lags(block_offsets, block_samples, f, lo, hi)
    pa = _prefix_counts(r, s, lo, hi, la)
    pb = _prefix_counts(r, s, lo, hi, lb)
    A = _mix(c, *pa)
    B = _mix(c, *[x[-1] - x for x in pb])
    n1 = np.concatenate([[0], np.cumsum(s[lo:hi].astype(np.int64))])
    n0 = np.arange(hi - lo + 1, dtype=np.int64) - n1
    N = n0.astype(np.float64) * z0 + n1.astype(np.float64) * z1
    return A, B, N


def refine(rb, sb, ref_levels, sub_levels, block_offsets, block_jump, block_samples, radius, beta):
    """BREAK_REFINE_DTYPE records of one pair's jumps (beta None = a single cut)."""
    S = np.asarray(sb).size
    k = int(block_samples)
    o = np.asarray(block_offsets, dtype=np.int64)
    fb = jumps_of(block_jump)
    cuts = [b * k for b in fb]
    recs = np.zeros(len(fb), dtype=_native.BREAK_REFINE_DTYPE)
    for j, (b, c, (lo, hi, clipped)) in enumerate(zip(fb, cuts, windows(cuts, S, int(radius)))):
        A, B, N = curves(rb, sb, ref_levels, sub_levels, lo, hi, o, k, b, beta)
        i1, i2, obj = cut(A, B, N, beta is None)
        t1, t2 = lo + i1, lo + i2
        flags = (CLIPPED if clipped else 0) | (AT_EDGE if (t1 == lo and lo > 0) or (t2 == hi and hi < S) else 0) \
            | (UNMATCHED if t1 < t2 else 0)
        rec = recs[j]
        rec["block"], rec["cut"], rec["lo"], rec["hi"], rec["t1"], rec["t2"] = b, c, lo, hi, t1, t2
        rec["offset_prev"], rec["offset_next"] = int(o[b - 1]), int(o[b])
        rec["coarse_score"] = A[c - lo] + B[c - lo]
        rec["refined_score"] = obj
        rec["flags"] = flags
    return recs


def brute(rb, sb, ref_levels, sub_levels, lo, hi, block_offsets, block_samples, f, beta):
    """(t1, t2, objective) by direct counting at every t, each sample at its own block's lag, and an O(n^2) search over
    every t1 <= t2: the largest objective, the smallest t2 that reaches it, then the smallest maximiser of F on [L, t2]."""
    r, s = np.asarray(rb) != 0, np.asarray(sb) != 0
    c, z0, z1 = constants(r, ref_levels, sub_levels, beta)
    R = r.size
    o = [int(x) for x in block_offsets]
    k = int(block_samples)

    def score(x0, x1, second):
        ov = n11 = n1x = nx1 = 0
        for i in range(x0, x1):
            b = i // k
            lag = o[max(b, f)] if second else o[min(b, f - 1)]
            if 0 <= i + lag < R:
                ov += 1
                n1x += int(s[i])
                nx1 += int(r[i + lag])
                n11 += int(s[i] and r[i + lag])
        return _mix(c, ov, n11, n1x, nx1)[()]

    n = hi - lo + 1
    A = [score(lo, lo + i, False) for i in range(n)]
    B = [score(lo + i, hi, True) for i in range(n)]
    if beta is None:
        best = None
        for i in range(n):
            v = A[i] + B[i]
            if best is None or v > best[2]:
                best = (lo + i, lo + i, v)
        return best
    N = []
    for i in range(n):
        n1 = int(s[lo:lo + i].sum())
        N.append(np.float64(i - n1) * z0 + np.float64(n1) * z1)
    vals = {}
    for i2 in range(n):
        g = N[i2] + B[i2]
        for i1 in range(i2 + 1):
            vals[(i1, i2)] = g + (A[i1] - N[i1])
    top = max(vals.values())
    i2 = min(j for (_, j), v in vals.items() if v == top)
    F = [A[i] - N[i] for i in range(i2 + 1)]
    i1 = F.index(max(F))
    return lo + i1, lo + i2, vals[(i1, i2)]
