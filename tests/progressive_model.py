"""Numpy statement of the progressive alignment (csrc/ffs_progressive.h, ffsubsync_amd.progressive): the
contract the device is pinned against.  Builds on tests/quality_model.py.

A slot: a two-level reference prefix r[0:L) that grows by appends, n_cand two-level candidate vectors, the lag window
d in [-W+1, W] whatever L is.  Subtitle sample i meets reference sample i + d.
  - n11_c(d) is kept as integers and grows per append by sum_{j in [L, L+n)} r[j] s_c[j - d]
  - score of candidate c at lag d: quality_model's arithmetic on (n11, n1x, nx1, ov) over the overlap
    i in [max(0, -d), min(S_c, L - d)); exactly 0.0 where it is empty.  Peaks are taken in the device's arithmetic
    (exact_reference.fma), so they hold bit for bit at any levels; the moments are numpy's
  - per candidate one report (quality_model.peaks / moments over the 2W scores), per slot one state
  - StopRule / run: the host decision of ffsubsync_amd.progressive, restated
"""
import math

import numpy as np

import exact_reference as er
import quality_model as qm
from oracle import runs_model as rm


def window_lags(W):
    return np.arange(-int(W) + 1, int(W) + 1, dtype=np.int64)


def n11_increment(new01, L, sub01, W):
    """sum_{j in [L, L+n)} r[j] s[j - d] for every d of the window (int64), by an fp64 FFT rounded to integers; r[L:L+n]
    = ``new01``.  Reads the subtitle samples [L - W, L + n + W - 1) only."""
    new = np.asarray(new01).astype(np.float64)
    n, W = new.size, int(W)
    if n == 0:
        return np.zeros(2 * W, np.int64)
    s = np.asarray(sub01)
    lo, hi = L - W, L + n + W - 1  # window of subtitle positions j - d
    win = np.zeros(hi - lo)
    a, b = max(lo, 0), min(hi, s.size)
    if b > a:
        win[a - lo:b - lo] = s[a:b] != 0
    # c[e] = sum_t new[t] win[t + e], e = W - d in [0, 2W)
    nfft = 1 << int(np.ceil(np.log2(win.size + n)))
    full = np.fft.irfft(np.fft.rfft(win, nfft) * np.conj(np.fft.rfft(new, nfft)), nfft)[:2 * W]
    c = np.rint(full).astype(np.int64)
    assert np.all(np.abs(full - c) < 0.25)
    return c[::-1].copy()  # ascending d


def n11_brute(ref01, sub01, W):
    """n11 of every lag of the window on the whole reference, by definition (tiny sizes)."""
    r, s = np.asarray(ref01) != 0, np.asarray(sub01) != 0
    out = np.zeros(2 * int(W), np.int64)
    for k, d in enumerate(window_lags(W)):
        for i in range(s.size):
            if 0 <= i + d < r.size:
                out[k] += int(s[i] and r[i + d])
    return out


def scores_from_counts(n11, ref01, sub01, ref_levels, sub_levels, W):
    """The 2W scores of the window from the integer n11 row and the vectors' prefix sums."""
    r, s = np.asarray(ref01) != 0, np.asarray(sub01) != 0
    L, S = r.size, s.size
    lags = window_lags(W)
    i0 = np.maximum(0, -lags)
    i1 = np.minimum(S, L - lags)
    ov = np.maximum(0, i1 - i0)
    has = ov > 0
    cs = np.concatenate([[0], np.cumsum(s.astype(np.int64))])
    cr = np.concatenate([[0], np.cumsum(r.astype(np.int64))])
    a, b = np.clip(i0, 0, S), np.clip(i1, 0, S)
    n1x = np.where(has, cs[b] - cs[a], 0)
    nx1 = np.where(has, cr[np.clip(b + lags, 0, L)] - cr[np.clip(a + lags, 0, L)], 0)
    f = lambda x: x.astype(np.float64)
    n11 = np.where(has, n11, 0)
    sc = rm.two_level_scores(f(n11), f(n1x), f(nx1), f(ov), qm._pm1(sub_levels[0]), qm._pm1(sub_levels[1]),
                             qm._pm1(ref_levels[0]), qm._pm1(ref_levels[1]))
    c00, c01, c10, c11 = er.two_level_coefficients(ref_levels, sub_levels)

    def exact_at(i):
        """The device's expression bit for bit (two_level_score: n00 c00, then three fused multiply-adds)."""
        if not has[i]:
            return 0.0
        a, b, c = int(n11[i]), int(n1x[i]) - int(n11[i]), int(nx1[i]) - int(n11[i])
        r = float(int(ov[i]) - a - b - c) * c00
        r = er.fma(float(c), c01, r)
        r = er.fma(float(b), c10, r)
        return er.fma(float(a), c11, r)

    # numpy's unfused sum and the fused chain differ by less than this (exact_reference._BOUND of the terms' magnitudes)
    slack = 2.0 ** -46 * float(ov.max()) * max(abs(c00), abs(c01), abs(c10), abs(c11))
    return lags, np.where(has, sc, 0.0), exact_at, slack


def exact_peaks(lags, sc, exact_at, slack, top_k, exclusion_samples):
    """quality_model.peaks with the device's arithmetic: each round's maximum is taken over the exact scores of the lags
    whose numpy score lies within ``slack`` of the round's numpy maximum; ties to the largest lag."""
    out = []
    ok = np.ones(lags.size, bool)
    for _ in range(top_k):
        if not ok.any():
            break
        near = np.flatnonzero(ok & (sc >= sc[ok].max() - slack - 1e-300))
        ex = np.array([exact_at(i) for i in near])
        i = int(near[ex == ex.max()][-1])
        out.append((float(ex.max()), int(lags[i])))
        ok &= np.abs(lags - lags[i]) >= exclusion_samples
    return out


def report_from_scores(lags, sc, exact_at, slack, top_k, exclusion_samples):
    mean, std, flags = qm.moments(sc)
    # sum_bound: what the rounding of either summation order can move the mean by (n terms, each sum within 2^-53 of
    # the magnitudes added so far): the mean of scores that cancel is known no better than this
    return dict(peaks=exact_peaks(lags, sc, exact_at, slack, top_k, exclusion_samples), mean=mean, std=std,
                n_lags=int(lags.size), flags=flags, sum_bound=float(lags.size * 2.0 ** -53 * np.abs(sc).mean()))


def state_from_reports(reps, L):
    """The slot state: best candidate = largest peak-1 score, smallest index on ties."""
    p1 = [rep["peaks"][0][0] for rep in reps]
    best = int(np.argmax(p1))  # (the first maximum)
    rep = reps[best]
    others = [p for c, p in enumerate(p1) if c != best]
    return dict(ref_len=int(L), best_cand=best, offset=rep["peaks"][0][1], score=rep["peaks"][0][0], mean=rep["mean"],
                std=rep["std"], runner_up=rep["peaks"][1][0] if len(rep["peaks"]) > 1 else math.nan,
                other_best=max(others) if others else math.nan, flags=rep["flags"])


class Slot:
    """One file: candidates [(0/1 vector, (lo, hi))], reference levels, W."""

    def __init__(self, cands, ref_levels, W):
        self.cands = [(np.asarray(v) != 0, tuple(lv)) for v, lv in cands]
        self.ref_levels = tuple(ref_levels)
        self.W = int(W)
        self.ref = np.zeros(0, bool)
        self.n11 = [np.zeros(2 * self.W, np.int64) for _ in self.cands]

    def append(self, new01, top_k=3, exclusion_samples=300):
        """Append samples; returns (reports per candidate, state)."""
        new = np.asarray(new01) != 0
        L = self.ref.size
        for c, (s, _) in enumerate(self.cands):
            self.n11[c] += n11_increment(new, L, s, self.W)
        self.ref = np.concatenate([self.ref, new])
        return self.records(top_k, exclusion_samples)

    def records(self, top_k=3, exclusion_samples=300):
        reps = []
        for c, (s, lv) in enumerate(self.cands):
            reps.append(report_from_scores(*scores_from_counts(self.n11[c], self.ref, s, self.ref_levels, lv, self.W), top_k,
                                           exclusion_samples))
        return reps, state_from_reports(reps, self.ref.size)


def report(ref01, sub01, ref_levels, sub_levels, W, top_k=3, exclusion_samples=300):
    """The report of one candidate on a whole prefix, from scratch (n11 through quality_model.counts)."""
    lags = window_lags(W)
    r, s = np.asarray(ref01) != 0, np.asarray(sub01) != 0
    if r.size == 0:
        n11 = np.zeros(lags.size, np.int64)
    else:
        n11 = qm.counts(r, s, lags)[0]
    return report_from_scores(*scores_from_counts(n11, r, s, ref_levels, sub_levels, W), top_k, exclusion_samples)


def window_is_reference_mask(L, S, W):
    """E2's condition, by the reference's own mask: its lag set for (L, S, W) is exactly [-W+1, W]."""
    if L < 1:
        return False
    got = qm.lag_set(L, S, W)
    return got.size == 2 * W and int(got[0]) == -W + 1 and int(got[-1]) == W


# ---- the host decision ------------------------------------------------------------------------------------------

def derived(state):
    """(psr, margin, ratio_margin) of a state: quality.derive restated (flat: 0, 0, and 0 or NaN)."""
    std = state["std"]
    if std == 0:
        return 0.0, 0.0, math.nan if math.isnan(state["other_best"]) else 0.0
    psr = (state["score"] - state["mean"]) / std
    margin = math.inf if math.isnan(state["runner_up"]) else (state["score"] - state["runner_up"]) / std
    return psr, margin, (state["score"] - state["other_best"]) / std


def settled(history, min_psr, min_margin, min_ratio_margin, stable_updates, offset_tolerance, min_samples):
    """StopRule.settled restated on model states: the last ``stable_updates`` states all name the same candidate, have
    offsets within ``offset_tolerance`` of the newest, pass the three thresholds and have L >= ``min_samples``."""
    if stable_updates is None or len(history) < stable_updates:
        return False
    last = history[-stable_updates:]
    new = last[-1]
    for st in last:
        psr, margin, rm_ = derived(st)
        if st["best_cand"] != new["best_cand"] or abs(st["offset"] - new["offset"]) > offset_tolerance:
            return False
        if st["flags"] & qm.FLAT or not (psr >= min_psr and margin >= min_margin):
            return False
        if not (math.isnan(st["other_best"]) or rm_ >= min_ratio_margin):
            return False
        if st["ref_len"] < min_samples:
            return False
    return True


def run(ref01, cands, ref_levels, W, chunk, rule, top_k=3, exclusion_samples=300):
    """One file through progressive_sync: chunks of ``chunk`` samples until ``rule`` (the keyword arguments of
    ``settled``) says stop or the reference ends.  Returns dict(updates, settled, state, history)."""
    slot = Slot(cands, ref_levels, W)
    ref = np.asarray(ref01) != 0
    history = []
    done = False
    for o in range(0, ref.size, chunk):
        _, st = slot.append(ref[o:o + chunk], top_k, exclusion_samples)
        history.append(st)
        if settled(history, **rule):
            done = True
            break
    return dict(updates=len(history), settled=done, state=history[-1], history=history)


def decision_distance(history, rule):
    """The smallest relative distance of a decision statistic (psr, margin, ratio_margin) of any state from its threshold
    (inf when a threshold is 0 and the statistic too)."""
    out = math.inf
    for st in history:
        for v, t in zip(derived(st), (rule["min_psr"], rule["min_margin"], rule["min_ratio_margin"])):
            if math.isfinite(v):
                out = min(out, abs(v - t) / max(abs(t), 1e-300) if t != 0 else (math.inf if v == 0 else abs(v)))
    return out
