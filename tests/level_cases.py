"""Case table of the multi-level run path (k_levels_sample, k_levels_bits, k_runs_chunk_flags_ml, k_runs_corr_ml,
k_runs_pick over multi-level tiles): level sets with the (q, m) the level analysis must return, and constructed problems
whose answers sit where that code can go wrong -- exact ties on tile edges, flat tops, broken ties, the zero rule,
winners at partial overlap, the 16-bit histogram cell at its limit, plane lengths at the extraction's chunk edges, lists
denser than the plan's stride.  tests/test_level_cases_host.py asserts what the table claims, tests/test_gpu_levels_exact.py
runs it against tests/exact_reference.py.  numpy only.

A problem is (name, float reference, [candidate 0/1 vectors], [candidate (lo, hi) levels]); its exact records are
``er.solve(ref, cands, None, cand_levels, max_off, max_off)``.
"""
import numpy as np

import exact_reference as er
from oracle import runs_model as rm

RUNS_T = 12288  # lags per run-boundary tile (csrc/ffs_runs.h)
RUNS_EDGE = 96  # list entries staged per edge-window stretch (csrc/ffs_runs.h)
STRIDE0 = 4096  # entries of a plan-owned list before the stride grows (csrc/ffsalign.hip, kRunsStride0)
F64, F32 = np.float64, np.float32


class LevelSet:
    """``levels`` ascending in ``dtype``; ``m`` / ``dv``: the multiplicities and the divisor of the smallest step the
    level analysis must find (q = smallest step / dv, formed in fp64 from the stored values); m None = not accepted."""

    def __init__(self, name, levels, m, dv=1, dtype=F64):
        self.name, self.m, self.dv, self.dtype = name, (None if m is None else list(m)), dv, dtype
        self.levels = np.asarray(levels, dtype=dtype)
        assert np.all(np.diff(self.levels.astype(F64)) > 0)

    @property
    def q(self):
        lam = [float(x) for x in self.levels.astype(F64)]
        return min(b - a for a, b in zip(lam, lam[1:])) / self.dv

    @property
    def n_planes(self):
        return self.levels.size - 1

    def __repr__(self):
        return self.name


ACCEPTED = [
    LevelSet("weighted_label_0", [0.0, 0.4, 0.6, 1.0], (2, 1, 2)),
    LevelSet("weighted_label_0.1", [0.1, 0.46, 0.64, 1.0], (2, 1, 2)),
    LevelSet("equal_steps", [0.0, 1.0 / 3.0, 2.0 / 3.0, 1.0], (1, 1, 1)),
    LevelSet("steps_1_8", [0.0, 0.1, 0.9], (1, 8)),
    LevelSet("steps_8_1", [0.0, 0.8, 0.9], (8, 1)),
    LevelSet("steps_1_8_1", [0.0, 0.1, 0.9, 1.0], (1, 8, 1)),
    LevelSet("steps_8_1_8", [0.0, 0.8, 0.9, 1.7], (8, 1, 8)),
    LevelSet("divisor_2", [0.0, 0.6, 1.0], (3, 2), dv=2),
    LevelSet("divisor_3", [0.0, 4.0 / 7.0, 1.0], (4, 3), dv=3),
    LevelSet("divisor_4", [0.0, 5.0 / 9.0, 1.0], (5, 4), dv=4),
    LevelSet("base_zero", [0.5, 0.75, 1.0], (1, 1)),  # 2 lam0 - 1 = 0: k0 and k1x vanish
    LevelSet("negative_base", [-0.25, 0.25, 1.25], (1, 2)),
    LevelSet("two_levels", [0.05, 0.8], (1,)),
    # the largest reachable sum of multiplicities: the smallest step is at most 4 quanta (divisors 1 .. 4), the others at
    # most 8, and 4 : 8 : 8 reduces to 1 : 2 : 2 -- 19 (test_level_cases_host searches every step triple)
    LevelSet("steps_3_8_8", [0.0, 3.0 / 19.0, 11.0 / 19.0, 1.0], (3, 8, 8), dv=3),
    LevelSet("dyadic_f32_2_1", [0.0, 0.5, 0.75], (2, 1), dtype=F32),
    LevelSet("dyadic_f32_1_1_2", [0.0, 0.25, 0.5, 1.0], (1, 1, 2), dtype=F32),
]
REJECTED = [
    LevelSet("steps_1_9", [0.0, 0.1, 1.0], None),  # a multiplicity above 8
    LevelSet("steps_7_5", [0.0, 7.0 / 12.0, 1.0], None),  # needs the divisor 5
    LevelSet("five_levels", [0.0, 0.25, 0.5, 0.75, 1.0], None),
    # float32 roundings of the weighted set: the rounded steps are 2 : 1 : 2 to 1.5e-7 only, the analysis asks for 1e-9, so
    # such a reference takes the transforms (DESIGN, multi-level section)
    LevelSet("weighted_rounded_f32", np.array([0.0, 0.4, 0.6, 1.0], F32), None, dtype=F32),
    LevelSet("weighted_label_0.1_rounded_f32", np.array([0.1, 0.46, 0.64, 1.0], F32), None, dtype=F32),
]
BY_NAME = {ls.name: ls for ls in ACCEPTED + REJECTED}
SUM_M_MAX = 19


def make(ls, planes):
    """The float reference of nested 0/1 planes (plane k+1 inside plane k): sample = levels[planes set at it], the
    level values themselves (lam0 + q sum_k m_k plane_k without the arithmetic)."""
    planes = [np.asarray(p) != 0 for p in planes]
    assert len(planes) == ls.n_planes
    for lo, hi in zip(planes, planes[1:]):
        assert not np.any(hi & ~lo), "planes must be nested"
    return ls.levels[np.sum(planes, axis=0, dtype=np.int64)]


def _nest(ls, a, b, c):
    """L - 1 nested planes around the middle plane ``a``: (a), (a | b, a) or (a | b, a, a & c)."""
    return {1: [a], 2: [a | b, a], 3: [a | b, a, a & c]}[ls.n_planes]


def _periodic(rng, P, mean_run):
    seg = np.maximum(1, rng.geometric(1.0 / mean_run, size=P))
    return np.repeat(rng.rand(seg.size) < 0.5, seg)[:P]


def _noise(rng, n, mean=40, p=0.4):
    seg = np.maximum(1, rng.geometric(1.0 / mean, size=n))
    return np.repeat(rng.rand(seg.size) < p, seg)[:n]


def _u8(x):
    return np.ascontiguousarray(x, dtype=np.uint8)


def window(R, S, max_off):
    """(lowest lag with samples in reach, top lag) of the window, as the tie constructions place their phases."""
    lags = er.qm.lag_set(R, S, max_off)
    return max(int(lags.min()), -S + 1), int(lags.max())


AMP = (0.0, 1.0 / 1.001)
ODD = (-0.5, 1.25)
TIE_S = 3072
TIE_R = TIE_S + 2 * RUNS_T + 500
TIE_P = RUNS_T // 8


def _periodic_parts(ls, phase, seed):
    rng = np.random.RandomState(seed)
    a, b, c = (_periodic(rng, TIE_P, 20) for _ in range(3))
    planes = [np.resize(p, TIE_R) for p in _nest(ls, a, b, c)]
    sub = _u8(np.resize(np.roll(a, -phase), TIE_S))
    return planes, sub


def periodic_ties(ls, max_off, seed=0):
    """Every plane has period P = RUNS_T / 8 and the candidate is the middle plane at a phase: on the lags of full
    overlap every d = phase (mod P) ties at the maximum.  Three phases: the tied lags on a tile's last lag, on a tile's
    first lag, on the window's top lag."""
    d_lo, d_top = window(TIE_R, TIE_S, max_off)
    probs = []
    for k, (name, phase) in enumerate((("tile_last", (d_lo + RUNS_T - 1) % TIE_P), ("tile_first", d_lo % TIE_P),
                                       ("window_top", d_top % TIE_P))):
        planes, sub = _periodic_parts(ls, phase, 100 + 10 * seed + k)
        probs.append(("periodic_" + name, make(ls, planes), [sub, _u8(np.roll(sub, 7)), sub], [(0.0, 1.0), (0.0, 1.0), AMP]))
    return probs


def min_tie_records(ls, max_off):
    """Records with two or more tied lags that the periodic and flat-top problems of one level set hold at least (the
    host test counts them with the exact reference).  Windowless and at window 6000: candidates 0 and 2 of the three
    periodic problems and all six flat-top candidates (base-zero set, windowless: the flat tops' maximum lies at
    partial overlap, one tie record there).  Seven lags: the three candidates of the 41-lag flat top."""
    if max_off == 3:
        return 3
    return 7 if ls.name == "base_zero" and max_off is None else 12


FLAT_S = RUNS_T  # a multiple of every plane period below: (1, 2 or 3) x 512 and x 2048
FLAT_R = FLAT_S + 2 * RUNS_T + 500


def flat_tops(ls, seed=0):
    """Reference runs of length a in every plane (period j's run belongs to the planes 0 .. j mod (L-1)), candidate runs
    of length b < a, one run per P samples on both sides: plateaus of a - b + 1 = 41 and 301 tied lags (S is a multiple
    of the planes' common period (L-1) P, so the counts over a full overlap do not depend on the lag).  The candidate's runs
    sit in the middle of their periods and the gaps are long, so a lag that drops a piece of the candidate from the
    overlap drops more agreeing zeros than disagreeing samples: the plateaus of full overlap are the maximum (not for
    the base-zero set, where a candidate's zeros weigh nothing)."""
    rng = np.random.RandomState(200 + seed)
    probs = []
    for a, b, P in ((60, 20, 512), (450, 150, 2048)):
        start = int(rng.randint(0, P))
        planes = [np.zeros(FLAT_R, bool) for _ in range(ls.n_planes)]
        for j, k in enumerate(range(start, FLAT_R, P)):
            for pl in planes[: 1 + j % ls.n_planes]:
                pl[k:k + a] = True
        sub = np.zeros(FLAT_S, np.uint8)
        for k in range((P - b) // 2, FLAT_S, P):
            sub[k:k + b] = 1
        probs.append(("flat_top_%d" % (a - b + 1), make(ls, planes), [sub, sub, _u8(np.roll(sub, 5))], [(0.0, 1.0), AMP, (0.0, 1.0)]))
    return probs


def broken_tie(ls, max_off, seed=0):
    """A periodic tie (the candidate: the middle plane with a few samples flipped, the same in every period) and ONE
    reference sample of the plane with the smallest m_k flipped towards the candidate, inside the first period that
    only the smallest tied lag covers: that lag gains m_k counts, every other tied lag keeps its score.
    Returns (problem, the unbroken problem, the smallest tied lag)."""
    rng = np.random.RandomState(300 + seed)
    a, b, c = (_periodic(rng, TIE_P, 20) for _ in range(3))
    cand_pat = a ^ (rng.rand(TIE_P) < 0.05)
    phase = 700
    planes = [np.resize(p, TIE_R) for p in _nest(ls, a, b, c)]
    sub = _u8(np.resize(np.roll(cand_pat, -phase), TIE_S))
    k = int(np.argmin(ls.m))
    level = np.sum(planes, axis=0)
    # the candidate's sample that meets reference position x at lag `phase` is cand_pat[x mod P]
    want_set = np.resize(cand_pat, TIE_R)
    x_all = np.arange(TIE_R)
    first = (x_all >= phase) & (x_all < phase + TIE_P)
    up = np.flatnonzero(first & (level == k) & want_set)  # plane k gains a sample the candidate has
    down = np.flatnonzero(first & (level == k + 1) & ~want_set)  # plane k loses a sample the candidate has not
    broken = [p.copy() for p in planes]
    if up.size:
        broken[k][up[0]] = True
    else:
        broken[k][down[0]] = False
    cl = [(0.0, 1.0), AMP]
    return (("broken_tie", make(ls, broken), [sub, sub], cl), ("unbroken_tie", make(ls, planes), [sub, sub], cl), phase)


ZERO_R, ZERO_S = 30000, 20000


def zero_rule(seed=0):
    """The base-zero set with candidates whose lower level is 0.5 (k0 = k1x = kx1 = 0: the score is M11 k11 alone): an
    all-zero candidate (every lag exactly 0.0: the window's largest lag wins), and equal best scores across candidates
    (a candidate padded by 300 zeros ties with the unpadded one 300 lags lower: the first maximal one wins)."""
    ls = BY_NAME["base_zero"]
    rng = np.random.RandomState(400 + seed)
    a, b = _noise(rng, ZERO_R), _noise(rng, ZERO_R, 60)
    ref = make(ls, [a | b, a])
    sub = _u8(a[5000:5000 + ZERO_S])
    sub[-300:] = 0
    zero = np.zeros(ZERO_S, np.uint8)
    padded = _u8(np.roll(sub, 300))
    return [("all_zero", ref, [zero, sub, zero], [(0.5, 1.0), (0.5, 1.0), (0.5, 0.9)]),
            ("equal_across_candidates", ref, [padded, sub, padded], [(0.5, 1.0)] * 3),
            ("equal_across_candidates_amp", ref, [sub, padded, sub], [(0.5, 0.95)] * 3)]


PARTIAL_LEVELS = [(0.0, 1.0), AMP, ODD]
PARTIAL_SETS = ["weighted_label_0", "steps_8_1_8", "base_zero", "steps_3_8_8", "negative_base"]


def partial_overlap(ls, n=64):
    """Seeded windowless problems with R, S in [2100, 12000] (R < S and R > S): each candidate is a noisy copy of the
    middle plane shifted so that it hangs over the reference's start (candidate 0) or end (candidate 1) -- the winner
    lies where Mx1 moves by up to sum m_k per lag and the prefilter's every-four-lags edge term is stale."""
    probs = []
    for seed in range(n):
        rng = np.random.RandomState(5000 + seed)
        R, S = int(rng.randint(2100, 12001)), int(rng.randint(2100, 12001))
        mean = int(rng.choice([6, 25, 80]))
        a, b, c = _noise(rng, R, mean, 0.5), _noise(rng, R, 2 * mean, 0.5), _noise(rng, R, mean, 0.5)
        ref = make(ls, _nest(ls, a, b, c))
        hang = int(rng.randint(S // 10, S // 2))  # samples of the candidate outside the reference
        hang = min(hang, S - 60)
        cands = []
        for d in (-hang, R - S + hang):
            idx = np.arange(S) + d
            ok = (idx >= 0) & (idx < R)
            sub = _noise(rng, S, mean, 0.5)
            sub[ok] = a[idx[ok]]
            sub ^= rng.rand(S) < 0.03
            cands.append(_u8(sub))
        lv = PARTIAL_LEVELS[seed % 3]
        probs.append(("partial_%d" % seed, ref, cands, [lv, lv]))
    return probs


NEG_R, NEG_S = 2500, 3500  # (a window past N - 1 - S leaves lags only when N > 2 S)


def negative_slice(ls, seed=0):
    """(problems, windows): ``max_offset_samples`` past N - 1 - S (N the reference's transform length) -- Python's
    negative slice leaves the lags [-S, max_off - N], a handful at the far negative end (-S itself has no overlap)."""
    rng = np.random.RandomState(600 + seed)
    n = er.orc.fft_length(NEG_R, NEG_S)
    probs = []
    for t in range(3):
        a, b, c = _noise(rng, NEG_R, 8, 0.5), _noise(rng, NEG_R, 20, 0.5), _noise(rng, NEG_R, 5, 0.5)
        subs = [_u8(_noise(rng, NEG_S, 6, 0.5)) for _ in range(2)]
        subs[0][-40:] = a[:40]  # the candidate's tail meets the reference's head
        probs.append(("negative_slice_%d" % t, make(ls, _nest(ls, a, b, c)), subs, [(0.0, 1.0), AMP]))
    return probs, [n - NEG_S + t for t in (0, 7, 29)]


def cell_guard(n_boundaries):
    """The 1 : 8 set, reference and candidate alternating every sample (the reference between lam[0] and lam[2], so both
    planes carry the candidate's ``n_boundaries`` boundaries), then ONE reference sample at lam[1] and one at lam[0] behind
    the candidate's end (without the middle level the analysis sees a two-level vector, m = 1): the flags kernel's bound
    of a histogram cell, sum_k m_k min(n_p, n_q), is 9 n -- 32760 at n = 3640, 32778 (over the 16-bit guard) at n = 3642."""
    ls = BY_NAME["steps_1_8"]
    assert n_boundaries % 2 == 0
    alt = np.arange(n_boundaries) % 2 == 0  # starts set, ends clear: a boundary at every position 0 .. n - 1
    planes = [np.concatenate([alt, [True, False]]), np.concatenate([alt, [False, False]])]
    return ("cell_guard_%d" % n_boundaries, make(ls, planes), [_u8(alt)], [(0.0, 1.0)])


def cell_bound(ls, ref, cand01):
    """sum_k m_k min(n_p, n_q) from the vectors' boundary counts (k_runs_chunk_flags_ml)."""
    lam, q, m = er.level_info(ref)
    n_p = rm.boundaries(cand01)[0].size
    return sum(mk * min(n_p, rm.boundaries(np.asarray(ref, F64) >= lam[k + 1])[0].size) for k, mk in enumerate(m))


TAIL_LENGTHS = sorted({16384 * k + e for k in (1, 2) for e in (-1, 0, 1)}
                      | {1024 * j + e for j in (15, 17, 31) for e in (-1, 1)}
                      | {128 * j + e for j in (127, 129, 255) for e in (-1, 1)})


def plane_tails(ls, seed=0):
    """Reference lengths around k_levels_bits' 16 384-sample chunks, 1024-sample wave stretches and 128-sample wave
    steps; the first and the last sample at the top level, the sample before the last at lam[0]; S about R / 3."""
    probs = []
    for R in TAIL_LENGTHS:
        rng = np.random.RandomState(700 + seed + R)
        a, b, c = _noise(rng, R, 30, 0.5), _noise(rng, R, 50, 0.5), _noise(rng, R, 20, 0.5)
        planes = _nest(ls, a, b, c)
        for p in planes:
            p[0] = p[-1] = True
            p[-2] = False
        S = R // 3
        shift = int(rng.randint(0, R - S))
        sub = a[shift:shift + S] ^ (rng.rand(S) < 0.02)
        probs.append(("tail_%d" % R, make(ls, planes), [_u8(sub), _u8(a[R - S:])], [(0.0, 1.0), AMP]))
    return probs


def small_problem(ls, seed, R=9000, S=6000, mean=120):
    """An ordinary pair (three candidates, one a shifted noisy copy of the middle plane) far inside every budget."""
    rng = np.random.RandomState(800 + seed)
    a, b, c = _noise(rng, R, mean, 0.5), _noise(rng, R, 2 * mean, 0.5), _noise(rng, R, mean, 0.5)
    shift = int(rng.randint(0, R - S))
    good = a[shift:shift + S] ^ (rng.rand(S) < 0.03)
    return ("small_%s_%d" % (ls.name, seed), make(ls, _nest(ls, a, b, c)), [_u8(_noise(rng, S, mean)), _u8(good), _u8(_noise(rng, S, 60))],
            [(0.0, 1.0), AMP, (0.0, 1.0)])


def odd_pair(ls, seed, R=9000, S=6000):
    """A pair whose reference the level analysis refuses (five levels, float32 roundings of the weighted set): its
    sub-batch takes the transforms.  Levels inside [0, 1], candidate levels (0, 1)."""
    rng = np.random.RandomState(900 + seed)
    level = np.minimum(np.cumsum([_noise(rng, R, 50, 0.5) for _ in range(ls.levels.size - 1)], axis=0)[-1], ls.levels.size - 1)
    ref = ls.levels[level]
    assert np.unique(ref).size == ls.levels.size
    shift = int(rng.randint(0, R - S))
    return ("odd_%s" % ls.name, ref, [_u8(level[shift:shift + S] >= 2), _u8(_noise(rng, S)), _u8(_noise(rng, S, 25))], [(0.0, 1.0)] * 3)


def dense_planes(n=9000):
    """Reference planes that alternate every sample over ``n`` samples (about n boundaries in each plane list against the
    initial stride of 4096), four pairs with one sparse candidate each (the histogram-cell bound sum_k m_k min(n_p, n_q)
    stays small): the shape of test_stride_growth_keeps_the_vector_capacity with a multi-level reference."""
    ls = BY_NAME["weighted_label_0"]
    rng = np.random.RandomState(1200)
    i = np.arange(n)
    a = i % 2 == 1
    ref = make(ls, [a | (i % 6 == 0), a, a & (i % 8 != 1)])
    return [("dense_%d" % k, ref, [_u8(_noise(rng, n - 300 * k - 7, 60))], [(0.0, 1.0)]) for k in range(4)]


def long_candidate_lists(n_pairs=3, R=20000, S=12000, seed=0):
    """ADVICE finding 1: a sparse weighted reference (every plane far below 4096 boundaries) against candidates whose
    boundary lists hold more than 4096 and fewer than 32768 entries (runs of one to three samples)."""
    ls = BY_NAME["weighted_label_0"]
    probs = []
    for p in range(n_pairs):
        rng = np.random.RandomState(1000 + seed + p)
        a, b, c = _noise(rng, R, 80, 0.5), _noise(rng, R, 150, 0.5), _noise(rng, R, 90, 0.5)
        cands = []
        for j in range(2):
            seg = rng.randint(1, 4, size=S)
            cands.append(_u8((np.repeat(np.arange(S) % 2 == j, seg)[:S])))
        probs.append(("long_lists_%d" % p, make(ls, _nest(ls, a, b, c)), cands, [(0.0, 1.0), AMP]))
    return probs


def alternating_list_candidate(ls, R=9000, S=5000, seed=0):
    """A candidate that alternates every sample: as a list-only vector its edge windows meet far more than RUNS_EDGE
    entries per stretch (list_bits32 then reads the list from global memory)."""
    rng = np.random.RandomState(1100 + seed)
    a, b, c = _noise(rng, R, 40, 0.5), _noise(rng, R, 70, 0.5), _noise(rng, R, 30, 0.5)
    alt = _u8(np.arange(S) % 2 == 0)
    mixed = alt.copy()
    mixed[1000:3000] = a[2000:4000]
    return ("alternating_list", make(ls, _nest(ls, a, b, c)), [alt, mixed, _u8(1 - alt)], [(0.0, 1.0), AMP, (0.0, 1.0)])


# ---- the transform path's rule for float references (tests/test_gpu_exact.py::test_float_references, amplitude levels):
# the offset lies in the lag set and its exact score is within the fp64 summation bound of the maximum; scores are not
# bit-compared (the transform path re-scores with a dot product over the samples)
def float_scores(ref, sub01, sub_levels, max_off):
    """(lags, fp64 FFT scores sum_i s'[i] (2 r[i+d] - 1), exact_at(lag) by math.fsum over the samples)."""
    import math

    r = 2.0 * np.asarray(ref, F64) - 1.0
    s = np.where(np.asarray(sub01) != 0, er.pm1(sub_levels[1]), er.pm1(sub_levels[0]))
    R, S = r.size, s.size
    lags = er.qm.lag_set(R, S, max_off)
    nfft = 1 << int(np.ceil(np.log2(R + S)))
    conv = np.fft.irfft(np.fft.rfft(r, nfft) * np.fft.rfft(s[::-1], nfft), nfft)
    ov = np.minimum(S, R - lags) - np.maximum(0, -lags)
    sc = np.where(ov > 0, conv[(lags + S - 1) % nfft], 0.0)

    def exact_at(d):
        i0, i1 = max(0, -d), min(S, R - d)
        return math.fsum(s[i0:i1] * r[i0 + d:i1 + d]) if i1 > i0 else 0.0

    return lags, sc, exact_at


def transform_rule_bad(ref, sub01, sub_levels, max_off, offset):
    """None when ``offset`` satisfies the rule, else a description."""
    lags, sc, exact_at = float_scores(ref, sub01, sub_levels, max_off)
    if lags.size == 0:
        return None
    if offset not in set(lags.tolist()):
        return ("not in the lag set", offset)
    near = lags[sc >= sc.max() - 1e-6]
    best = max(exact_at(int(d)) for d in near[:2000])
    at = exact_at(int(offset))
    bound = 1e-12 * (np.asarray(ref).size + np.asarray(sub01).size)  # fp64 sums of products of magnitude <= 1
    return None if at >= best - bound else ("below the maximum", offset, at, best)
