"""Numpy statement of the sampled alignment (csrc/ffs_sampled.h, ffsubsync_amd.sampled): the contract the
device is pinned against.  Builds on tests/progressive_model.py and tests/quality_model.py.

A slot: a two-level reference of declared length T of which disjoint intervals [a, b) arrive in any order; K is their
union (abutting intervals merge).  n_cand two-level candidates, the lag window d in [-W+1, W].  Subtitle sample i meets
reference sample i + d.  Counts of candidate c at lag d over I(d) = { i : 0 <= i < S_c, i + d in K }:
    ov = |I|,  n11 = sum_I s[i] r[i+d],  n1x = sum_I s[i],  nx1 = sum_I r[i+d]
  - score: exactly 0.0 where ov = 0, else progressive_model's arithmetic on (n11, n1x, nx1) with this ov in place of the
    overlap length -- the unmodified reference aligner's score on a reference that holds 0.5 in every unread frame
  - per candidate one report (greedy peaks, moments, FLAT over the 2W scores), per slot one state with ref_len = |K|
  - segment_schedule / run: the host side of ffsubsync_amd.sampled, restated
"""
import numpy as np

import exact_reference as er
import progressive_model as pm
import quality_model as qm
from oracle import runs_model as rm

MAX_INTERVALS = 256


def merge(intervals):
    """Sorted union of disjoint [a, b) intervals with abutting ones merged."""
    out = []
    for a, b in sorted((int(a), int(b)) for a, b in intervals if b > a):
        if out and out[-1][1] == a:
            out[-1][1] = b
        else:
            assert not out or out[-1][1] < a, "intervals overlap"
            out.append([a, b])
    return [tuple(x) for x in out]


def side_increment(a, b, ref01, sub01, W):
    """(ov, n1x, nx1) that the interval [a, b) of the reference ``ref01`` (whole length; only [a, b) is read) adds at
    every lag of the window: subtitle samples [i0, i1) = [max(a - d, 0), min(b - d, S)) meet it."""
    s = np.asarray(sub01) != 0
    r = np.asarray(ref01) != 0
    lags = pm.window_lags(W)
    i0 = np.maximum(a - lags, 0)
    i1 = np.minimum(b - lags, s.size)
    has = i1 > i0
    i0, i1 = np.where(has, i0, 0), np.where(has, i1, 0)
    cs = np.concatenate([[0], np.cumsum(s.astype(np.int64))])
    seg = np.zeros(r.size, np.int64)
    seg[a:b] = r[a:b]
    cr = np.concatenate([[0], np.cumsum(seg)])
    return i1 - i0, cs[i1] - cs[i0], np.where(has, cr[np.clip(i1 + lags, 0, r.size)] - cr[np.clip(i0 + lags, 0, r.size)], 0)


def counts_brute(ref01, known, sub01, W):
    """(n11, n1x, nx1, ov) of every lag of the window by the definition: a triple loop (tiny sizes)."""
    r, s, k = np.asarray(ref01) != 0, np.asarray(sub01) != 0, np.asarray(known) != 0
    out = np.zeros((4, 2 * int(W)), np.int64)
    for j, d in enumerate(pm.window_lags(W)):
        for i in range(s.size):
            if 0 <= i + d < r.size and k[i + d]:
                out[0, j] += int(s[i] and r[i + d])
                out[1, j] += int(s[i])
                out[2, j] += int(r[i + d])
                out[3, j] += 1
    return out


def counts_direct(ref01, known, sub01, W):
    """(n11, n1x, nx1, ov) of every lag of the window from scratch over the whole known set, in int64, with nothing
    incremental: no append order, no interval as it was fed, no word.  With k the known mask and kr = k & r,
        ov(d) = sum_p k[p] [0 <= p - d < S]    n1x(d) = sum_p k[p] s[p - d]
        nx1(d) = sum_p kr[p] [0 <= p - d < S]  n11(d) = sum_p kr[p] s[p - d]
    and each sum over p runs over the maximal runs [a, b) of its mask, where it is a difference of two entries of a prefix
    sum (of ones, or of s) at b - d and a - d cut to [0, S]."""
    r, s, k = np.asarray(ref01) != 0, np.asarray(sub01) != 0, np.asarray(known) != 0
    lags = pm.window_lags(W)
    ones = np.arange(s.size + 1, dtype=np.int64)
    cs = np.concatenate([[0], np.cumsum(s.astype(np.int64))])

    def over(mask, prefix):
        edges = np.flatnonzero(np.diff(np.concatenate([[0], mask.astype(np.int8), [0]])))
        total = np.zeros(lags.size, np.int64)
        for a, b in zip(edges[::2], edges[1::2]):
            total += prefix[np.clip(b - lags, 0, s.size)] - prefix[np.clip(a - lags, 0, s.size)]
        return total

    return np.stack([over(k & r, cs), over(k, cs), over(k & r, ones), over(k, ones)])


def scores_from_counts(n11, n1x, nx1, ov, ref_levels, sub_levels, W):
    """progressive_model.scores_from_counts with the overlap given: (lags, numpy scores, exact_at, slack)."""
    lags = pm.window_lags(W)
    has = ov > 0
    f = lambda x: np.where(has, x, 0).astype(np.float64)
    sc = rm.two_level_scores(f(n11), f(n1x), f(nx1), f(ov), qm._pm1(sub_levels[0]), qm._pm1(sub_levels[1]),
                             qm._pm1(ref_levels[0]), qm._pm1(ref_levels[1]))
    c00, c01, c10, c11 = er.two_level_coefficients(ref_levels, sub_levels)

    def exact_at(i):
        """The device's expression bit for bit (samp_score: n00 c00, then three fused multiply-adds)."""
        if not has[i]:
            return 0.0
        a, b, c = int(n11[i]), int(n1x[i]) - int(n11[i]), int(nx1[i]) - int(n11[i])
        r = float(int(ov[i]) - a - b - c) * c00
        r = er.fma(float(c), c01, r)
        r = er.fma(float(b), c10, r)
        return er.fma(float(a), c11, r)

    slack = 2.0 ** -46 * float(max(int(ov.max()), 1)) * max(abs(c00), abs(c01), abs(c10), abs(c11))
    return lags, np.where(has, sc, 0.0), exact_at, slack


class Slot:
    """One file: candidates [(0/1 vector, (lo, hi))], reference levels, W, the declared reference length T."""

    def __init__(self, cands, ref_levels, W, T):
        self.cands = [(np.asarray(v) != 0, tuple(lv)) for v, lv in cands]
        self.ref_levels = tuple(ref_levels)
        self.W, self.T = int(W), int(T)
        self.ref = np.zeros(self.T, bool)
        self.known = np.zeros(self.T, bool)
        self.intervals = []
        self.counts = [np.zeros((4, 2 * self.W), np.int64) for _ in self.cands]  # n11, n1x, nx1, ov

    def check(self, a, n):
        """What ffs_prog_append_at refuses: a string, or None."""
        a, n = int(a), int(n)
        if n < 0 or a < 0 or a + n > self.T:
            return "outside the reference"
        if n and self.known[a:a + n].any():
            return "overlaps"
        if n and len(merge(self.intervals + [(a, a + n)])) > MAX_INTERVALS:
            return "intervals"
        return None

    def append_at(self, a, new01, top_k=3, exclusion_samples=300):
        """Samples [a, a + len(new01)) become known; returns (reports per candidate, state)."""
        new = np.asarray(new01) != 0
        a, b = int(a), int(a) + new.size
        assert self.check(a, new.size) is None
        if new.size:
            self.ref[a:b] = new
            self.known[a:b] = True
            self.intervals = merge(self.intervals + [(a, b)])
            for c, (s, _) in enumerate(self.cands):
                self.counts[c][0] += pm.n11_increment(new, a, s, self.W)
                ov, n1x, nx1 = side_increment(a, b, self.ref, s, self.W)
                self.counts[c][1] += n1x
                self.counts[c][2] += nx1
                self.counts[c][3] += ov
        return self.records(top_k, exclusion_samples)

    def records(self, top_k=3, exclusion_samples=300):
        reps = []
        for c, (_, lv) in enumerate(self.cands):
            n11, n1x, nx1, ov = self.counts[c]
            reps.append(pm.report_from_scores(*scores_from_counts(n11, n1x, nx1, ov, self.ref_levels, lv, self.W), top_k,
                                              exclusion_samples))
        return reps, pm.state_from_reports(reps, int(self.known.sum()))

    def slack(self, c):
        """scores_from_counts' slack for candidate c on what is known now: what a score by another summation order (numpy's
        unfused sum, a transform's entry) may differ by from the device's fused chain."""
        n11, n1x, nx1, ov = self.counts[c]
        return scores_from_counts(n11, n1x, nx1, ov, self.ref_levels, self.cands[c][1], self.W)[3]

    def filled(self, unknown=0.5):
        """The float reference the one-shot aligner takes: the reference levels where known, ``unknown`` elsewhere."""
        lo, hi = self.ref_levels
        return np.where(self.known, np.where(self.ref, hi, lo), unknown).astype(np.float64)


def report(ref01, known, sub01, ref_levels, sub_levels, W, top_k=3, exclusion_samples=300):
    """The report of one candidate on a known set, from scratch: one append per maximal run of ``known``."""
    k = np.asarray(known) != 0
    slot = Slot([(sub01, sub_levels)], ref_levels, W, k.size)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], k.astype(np.int8), [0]])))
    for a, b in zip(edges[::2], edges[1::2]):
        slot.append_at(a, np.asarray(ref01)[a:b] != 0, top_k, exclusion_samples)
    return slot.records(top_k, exclusion_samples)[0][0]


def decision_gap(slot):
    """(exact top-2 gap of the slot's decision, (best_cand, offset)): the largest exact score over every (candidate, lag)
    minus the next one.  Above 0.5, no rounding of a transform can change the winner."""
    rest = []
    for c in range(len(slot.cands)):
        n11, n1x, nx1, ov = slot.counts[c]
        lags, _, exact_at, _ = scores_from_counts(n11, n1x, nx1, ov, slot.ref_levels, slot.cands[c][1], slot.W)
        rest += [(exact_at(i), c, int(lags[i])) for i in range(lags.size)]
    rest.sort(reverse=True)
    return rest[0][0] - rest[1][0], (rest[0][1], rest[0][2])


# ---- the host side ----------------------------------------------------------------------------------------------

def bit_reversed(n):
    """0 .. n-1 in bit-reversed order: m runs over the bit reversals of 0 .. N-1 (N the power of two >= n) and names
    index floor(m n / N), first mention only.  For n a power of two this is the bit reversal itself; for any n the first
    2^k entries are floor(i n / 2^k), evenly spread."""
    n = int(n)
    bits = max(n - 1, 0).bit_length()
    out, seen = [], set()
    for m in range(1 << bits):
        k = (int(format(m, "0%db" % bits)[::-1], 2) if bits else 0) * n >> bits
        if k not in seen:
            seen.add(k)
            out.append(k)
    return out


def segment_schedule(total, seg):
    """The grid segments [k seg, min((k + 1) seg, T)) in bit-reversed order of k."""
    total, seg = int(total), int(seg)
    n = (total + seg - 1) // seg
    return [(k * seg, min((k + 1) * seg, total)) for k in bit_reversed(n)]


def run(ref01, cands, ref_levels, W, schedule, rule, top_k=3, exclusion_samples=300):
    """One file through sampled_sync: the segments of ``schedule`` in order until ``rule`` (the keyword arguments of
    progressive_model.settled; ref_len counts known samples) says stop or the schedule ends."""
    ref = np.asarray(ref01) != 0
    slot = Slot(cands, ref_levels, W, ref.size)
    history = []
    done = False
    for a, b in schedule:
        _, st = slot.append_at(a, ref[a:b], top_k, exclusion_samples)
        history.append(st)
        if pm.settled(history, **rule):
            done = True
            break
    return dict(updates=len(history), settled=done, state=history[-1], history=history, slot=slot)
