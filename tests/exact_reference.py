"""Exact CPU reference of every solve record, ties included (numpy and ``fractions`` only).

What the library promises for one candidate:
  - lag set: exactly the entries of the reference's masked ``convolve`` array (quality_model.lag_set, Python slice
    semantics included); convolve index k is lag N-1-S-k
  - counts at every lag: n11 = sum_i s[i] r[i+d] by an fp64 FFT rounded to integers (rounding slack asserted < 0.25),
    ov / n1x / nx1 from cumulative sums -- nothing from the run-boundary formula or a window walk
  - score: the device's fp64 expression bit for bit (``two_level_score`` in csrc/ffs_kernels.h: n00 c00, then three
    fused multiply-adds, c.. = products of the mapped levels 2x - 1); lags whose overlap is empty score exactly 0.0
  - winner: the maximum over every lag, ties to the LARGEST lag (np.argmax's first k); an empty window gives -inf at
    offset N-1-S with flag 1
  - pair: the first maximal candidate among those whose |offset| passes the filter (aligners.py:154-167), the filtered
    ones flagged 4
Multi-level references (the run path's threshold lists, csrc/ffs_runs.h LevelInfo): the same structure with the weighted
counts M11 / Mx1 of M = sum_k m_k [r >= lam_k] and the coefficients k0, k1x, kx1, k11 (ov k0, then three fmas).

Python has no math.fma before 3.13: ``fma`` evaluates a*b + c exactly with Fractions and rounds once.  Only lags whose
plain numpy score lies within a safe bound of the maximum are evaluated that way; numpy settles every other lag.
"""
from fractions import Fraction

import numpy as np

import quality_model as qm
from oracle import aligners_oracle as orc

FLAG_EMPTY = 1
FLAG_FILTERED = 4
# numpy's unfused sum and the device's fused chain each round at most 7 times; both differ from the exact value by less
# than 2^-50 of the sum of the terms' magnitudes, so a lag more than 2^-46 of it below the numpy maximum cannot tie
_BOUND = 2.0 ** -46


def fma(a, b, c):
    """a*b + c rounded once to the nearest double (IEEE fusedMultiplyAdd, zero signs included)."""
    a, b, c = float(a), float(b), float(c)
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact != 0:
        return float(exact)
    prod_neg = (a == 0.0 or b == 0.0) and (np.copysign(1.0, a) * np.copysign(1.0, b) < 0)
    if (a == 0.0 or b == 0.0) and c == 0.0 and prod_neg and np.signbit(c):
        return -0.0
    return 0.0


def pm1(level):
    return 2.0 * float(level) - 1.0


def two_level_coefficients(ref_levels, sub_levels):
    """(c00, c01, c10, c11) as the device forms them: products of the mapped levels in fp64."""
    s0, s1 = pm1(sub_levels[0]), pm1(sub_levels[1])
    r0, r1 = pm1(ref_levels[0]), pm1(ref_levels[1])
    return s0 * r0, s0 * r1, s1 * r0, s1 * r1


def _nfft(R, S):
    return 1 << int(np.ceil(np.log2(R + S)))


class RefSpectrum:
    """The reference vector (0/1, or the integer M of a multi-level reference) with its fp64 spectrum, reused by every
    candidate of a pair whose transform length matches."""

    def __init__(self, r):
        self.r = np.asarray(r)
        self.cum = np.concatenate([[0], np.cumsum(self.r.astype(np.int64))])
        self._spec = {}

    def spectrum(self, nfft):
        if nfft not in self._spec:
            self._spec[nfft] = np.fft.rfft(self.r.astype(np.float64), nfft)
        return self._spec[nfft]


def counts(ref, sub01, lags):
    """(n11, n1x, nx1, ov) at every lag (int64): n11 by an fp64 FFT rounded to integers, the rest by cumulative sums.
    ``ref`` is a 0/1 vector or a RefSpectrum (then n11 / nx1 are weighted by its integer values)."""
    ref = ref if isinstance(ref, RefSpectrum) else RefSpectrum(ref)
    s = np.asarray(sub01).astype(np.int64)
    R, S = ref.r.size, s.size
    lags = np.asarray(lags, dtype=np.int64)
    i0 = np.maximum(0, -lags)
    i1 = np.minimum(S, R - lags)
    ov = np.maximum(0, i1 - i0)
    has = ov > 0
    n11 = np.zeros(lags.size, np.int64)
    if has.any():
        nfft = _nfft(R, S)
        conv = np.fft.irfft(ref.spectrum(nfft) * np.fft.rfft(s[::-1].astype(np.float64), nfft), nfft)
        raw = conv[lags[has] + S - 1]  # conv[d + S - 1] = sum_i s[i] r[i + d]
        n11[has] = np.rint(raw).astype(np.int64)
        slack = float(np.abs(raw - n11[has]).max())
        assert slack < 0.25, slack
    cs = np.concatenate([[0], np.cumsum(s)])
    a, b = np.clip(i0, 0, S), np.clip(i1, 0, S)
    n1x = np.where(has, cs[b] - cs[a], 0)
    nx1 = np.where(has, ref.cum[np.clip(b + lags, 0, R)] - ref.cum[np.clip(a + lags, 0, R)], 0)
    return n11, n1x, nx1, ov


def _chain(first, terms):
    """first = (count, coefficient) multiplied in fp64, then one fma per (count, coefficient) of ``terms``."""
    r = float(first[0]) * first[1]
    for n, c in terms:
        r = fma(float(n), c, r)
    return r


def _pick(lags, ov, approx, abssum, exact_at):
    """Exact maximum over the lags (zero-overlap lags = 0.0), ties to the largest lag: (score, offset, n_at_max)."""
    sc = np.where(ov > 0, approx, 0.0)
    top = float(sc.max())
    near = np.flatnonzero(sc >= top - _BOUND * float(abssum.max()) - 1e-300)
    ex = np.array([exact_at(i) if ov[i] > 0 else 0.0 for i in near])
    best = float(ex.max())
    at = near[ex == best]
    return best, int(lags[at].max()), int(at.size)


def _empty(R, S):
    return dict(score=float("-inf"), offset=orc.fft_length(R, S) - 1 - S, flags=FLAG_EMPTY, n_at_max=0)


def candidate(ref01, sub01, ref_levels, sub_levels, max_offset_samples):
    """Exact record of one candidate against a two-level reference: dict(score, offset, flags, n_at_max)."""
    ref = ref01 if isinstance(ref01, RefSpectrum) else RefSpectrum(np.asarray(ref01) != 0)
    sub01 = np.asarray(sub01) != 0
    R, S = ref.r.size, sub01.size
    lags = qm.lag_set(R, S, max_offset_samples)
    if lags.size == 0:
        return _empty(R, S)
    n11, n1x, nx1, ov = counts(ref, sub01, lags)
    c00, c01, c10, c11 = two_level_coefficients(ref_levels, sub_levels)
    n10, n01 = n1x - n11, nx1 - n11
    n00 = ov - n11 - n10 - n01
    f = lambda x: x.astype(np.float64)
    approx = f(n00) * c00 + f(n01) * c01 + f(n10) * c10 + f(n11) * c11
    abssum = np.abs(f(n00) * c00) + np.abs(f(n01) * c01) + np.abs(f(n10) * c10) + np.abs(f(n11) * c11)
    exact_at = lambda i: _chain((n00[i], c00), [(n01[i], c01), (n10[i], c10), (n11[i], c11)])
    score, offset, n_at = _pick(lags, ov, approx, abssum, exact_at)
    return dict(score=score, offset=offset, flags=0, n_at_max=n_at)


def score_at(ref01, sub01, ref_levels, sub_levels, d):
    """The exact score of one lag (0.0 without overlap)."""
    ref01, sub01 = np.asarray(ref01) != 0, np.asarray(sub01) != 0
    i0, i1 = max(0, -d), min(sub01.size, ref01.size - d)
    if i1 <= i0:
        return 0.0
    s, r = sub01[i0:i1].astype(np.int64), ref01[i0 + d:i1 + d].astype(np.int64)
    n11, n1x, nx1, ov = int(np.dot(s, r)), int(s.sum()), int(r.sum()), i1 - i0
    c00, c01, c10, c11 = two_level_coefficients(ref_levels, sub_levels)
    n10, n01 = n1x - n11, nx1 - n11
    return _chain((ov - n11 - n10 - n01, c00), [(n01, c01), (n10, c10), (n11, c11)])


def level_info(ref):
    """The run path's level analysis of a float reference (k_levels_sample): (lam ascending, q, m) or None when the
    reference is not a usable multi-level vector.  The same fp64 operations, so q and m are the device's."""
    lam = np.unique(np.asarray(ref, dtype=np.float64))
    if not 2 <= lam.size <= 4:
        return None
    lam = [float(x) for x in lam]
    q = min(lam[i] - lam[i - 1] for i in range(1, len(lam)))
    for dv in range(1, 5):
        qq = q / dv
        m = []
        for i in range(1, len(lam)):
            r = (lam[i] - lam[i - 1]) / qq
            rr = float(np.rint(r))
            if not (abs(r - rr) <= 1e-9 * rr and 1.0 <= rr <= 8.0):
                break
            m.append(int(rr))
        else:
            return lam, qq, m
    return None


def multilevel_weights(ref, lam, m):
    """M = sum_k m_k [r >= lam_k] evaluated directly (int64)."""
    ref = np.asarray(ref, dtype=np.float64)
    M = np.zeros(ref.size, np.int64)
    for k in range(1, len(lam)):
        M += m[k - 1] * (ref >= lam[k])
    return M


def candidate_multilevel(ref, sub01, sub_levels, max_offset_samples, info=None):
    """Exact record of a two-level candidate against a multi-level float reference, as the run path defines it:
    score = ov k0 + n1x k1x + Mx1 kx1 + M11 k11 (ov k0, then three fmas) with k0 = (2 lam0 - 1) s0,
    k1x = (2 lam0 - 1)(s1 - s0), kx1 = 2q s0, k11 = 2q (s1 - s0).  ``ref`` is the float vector or a RefSpectrum of M
    (then ``info`` = level_info of the float vector)."""
    if not isinstance(ref, RefSpectrum):
        info = level_info(ref)
        assert info is not None
        ref = RefSpectrum(multilevel_weights(ref, info[0], info[2]))
    lam, q, _ = info
    sub01 = np.asarray(sub01) != 0
    R, S = ref.r.size, sub01.size
    lags = qm.lag_set(R, S, max_offset_samples)
    if lags.size == 0:
        return _empty(R, S)
    m11, n1x, mx1, ov = counts(ref, sub01, lags)
    s0, s1 = pm1(sub_levels[0]), pm1(sub_levels[1])
    base, two_q = 2.0 * lam[0] - 1.0, 2.0 * q
    k0, k1x, kx1, k11 = base * s0, base * (s1 - s0), two_q * s0, two_q * (s1 - s0)
    f = lambda x: x.astype(np.float64)
    approx = f(ov) * k0 + f(n1x) * k1x + f(mx1) * kx1 + f(m11) * k11
    abssum = np.abs(f(ov) * k0) + np.abs(f(n1x) * k1x) + np.abs(f(mx1) * kx1) + np.abs(f(m11) * k11)
    exact_at = lambda i: _chain((ov[i], k0), [(n1x[i], k1x), (mx1[i], kx1), (m11[i], k11)])
    score, offset, n_at = _pick(lags, ov, approx, abssum, exact_at)
    return dict(score=score, offset=offset, flags=0, n_at_max=n_at)


def pair(records, filter_max=None):
    """MaxScoreAligner.transform over exact candidate records (aligners.py:154-167): marks the filtered candidates
    (flag 4, in place) and returns dict(best_cand, score, offset) -- best_cand -1 when every candidate is filtered."""
    best = dict(best_cand=-1, score=0.0, offset=0)
    for j, r in enumerate(records):
        if filter_max is not None and abs(r["offset"]) > filter_max:
            r["flags"] |= FLAG_FILTERED
            continue
        if best["best_cand"] < 0 or r["score"] > best["score"]:
            best = dict(best_cand=j, score=r["score"], offset=r["offset"])
    return best


def solve(ref, cands01, ref_levels, cand_levels, max_offset_samples, filter_max=None):
    """(candidate records, pair record) of one problem; ``ref_levels`` None = a multi-level float reference."""
    if ref_levels is None:
        info = level_info(ref)
        assert info is not None
        spec = RefSpectrum(multilevel_weights(ref, info[0], info[2]))
        recs = [candidate_multilevel(spec, c, lv, max_offset_samples, info) for c, lv in zip(cands01, cand_levels)]
    else:
        spec = RefSpectrum(np.asarray(ref) != 0)
        recs = [candidate(spec, c, ref_levels, lv, max_offset_samples) for c, lv in zip(cands01, cand_levels)]
    return recs, pair(recs, filter_max)


def save_golden(path, kinds):
    """Write {kind: [record]} (records as make_exact_golden.solve_seed returns them) as one compressed .npz."""
    arrays = {}
    for kind, recs in kinds.items():
        arrays[kind + "_seed"] = np.array([g["seed"] for g in recs], np.int32)
        for f, i, dt in (("score", 0, np.float64), ("offset", 1, np.int64), ("n_at_max", 2, np.int32), ("flags", 3, np.uint8)):
            arrays[kind + "_" + f] = np.array([[c[i] for c in g["cand"]] for g in recs], dt)
        arrays[kind + "_winner"] = np.array([g["winner"][:2] for g in recs], np.int64)
        arrays[kind + "_winner_score"] = np.array([g["winner"][2] for g in recs], np.float64)
    np.savez_compressed(path, **arrays)


def load_golden(path):
    """{kind: [dict(seed, cand=[[score, offset, n_at_max, flags] ...], winner=[best_cand, offset, score])]}."""
    z = np.load(path)
    kinds = sorted({k.rsplit("_seed", 1)[0] for k in z.files if k.endswith("_seed")})
    out = {}
    for kind in kinds:
        a = {f: z[kind + "_" + f] for f in ("seed", "score", "offset", "n_at_max", "flags", "winner", "winner_score")}
        out[kind] = [dict(seed=int(a["seed"][p]),
                          cand=[[float(a["score"][p, j]), int(a["offset"][p, j]), int(a["n_at_max"][p, j]), int(a["flags"][p, j])]
                                for j in range(a["score"].shape[1])],
                          winner=[int(a["winner"][p, 0]), int(a["winner"][p, 1]), float(a["winner_score"][p])])
                     for p in range(a["seed"].size)]
    return out


def solve_spec(spec, max_offset_samples, filter_max=None):
    """A workloads.synth PairSpec (reference levels (0, 1), candidate j levels (0, amp_j))."""
    from workloads import synth

    ref, cands = synth.pair_arrays(spec)
    return solve(ref, cands, (0.0, 1.0), [(0.0, a) for a in spec.cand_amp], max_offset_samples, filter_max)
