"""The case table of the transform path's solve records: one entry per plan length, 22 in all (numpy only).

The transform path (pass A, mid, pass C, k_nominees, k_rescore, pool, finalize) selects a kernel instance per column
length N1 and row length N2 of the plan, and variants by input type, paired first pass, half slots, pruned / full /
radix-3 last pass and single-transform / block-segmented mid pass.  This module states, per plan length, the inputs that
reach every one of them, what each solve is expected to launch (``expected_dispatch``: compared with
``Plan.dispatch_report()``), and the exact records (tests/exact_reference.py, cached per length, vector set and window).

Vectors fill the plan: R + S = N - 3 with R = N/2 + 1000, so the windowless plan length is exactly N and lags map onto
nearly every output index.  A call solves problems of one of two kinds:

* ``noise``: one pair, a run-structured noise reference (``_noise`` of test_gpu_exact.py, one-runs capped at 23 samples
  but for a 50-sample pattern with a run of 27 at either end) against candidates of different lengths S_j <= S that carry a copy of the reference
  planted at an offset that lands in a particular place of the transform -- d = 0 and -1, d = 0 and -1 (mod N2: a
  last-pass bin edge), d in {C - 1, C} for the column tile width C of the instance, the edges of the window -- and two
  candidates that are silent (levels (0.5, 1): zeros contribute nothing) but for that pattern at their end /
  start: their only full score is at the far ends d = 50 - S_j and d = R - 50, which wrap through m = d + N.
* ``ties``: two pairs -- ``_flat_top`` plateaus of 41 and of 700 consecutive tied lags (wider than the KNOM = 16 nominees:
  the exhaustive sweep has real work at every length) and a ``_shared_period`` candidate whose ties straddle last-pass
  bin edges (one of them on the last lag of bin 0).

Settings per length: (a) windowless; (b) window N2/2 - 1 (two last-pass bins: the pruned pass, block-segmented on
3*2^16 .. 3*2^20); (c) window N2 + 5 (four bins); (d) = (b) under FFS_DISABLE_PRUNED_PASS_C=1; (e) = (b) under
FFS_DISABLE_SEGMENTED=1 on the five segmented lengths.  The ``long`` vector set (R = S = 0.9 N, windowed only) makes the
segmented path take three blocks instead of two on 3*2^16 .. 3*2^18.
"""
import functools
from collections import namedtuple

import numpy as np

import exact_reference as er
from test_gpu_exact import _flat_top, _noise, _shared_period

KNOM = 16
POOL_CAPACITY = 1 << 20
LENGTHS = [1 << k for k in range(12, 25)] + [3 << k for k in range(12, 21)]
SEGMENTED = [3 << k for k in range(16, 21)]
THREE_BLOCK = [3 << 16, 3 << 17, 3 << 18]
C3_N1 = (192, 384, 768, 512)  # column lengths with three (two) sub-transforms per thread: k_pass_a3 / k_pass_c3
# column tile width of k_pass_c / k_pass_c_pruned per column length, and of k_pass_c3 at its four
TILE = {16: 256, 32: 128, 64: 64, 128: 32, 256: 16, 512: 16, 1024: 16, 2048: 8, 4096: 4, 48: 64, 96: 32, 192: 16, 384: 16, 768: 16}
TILE3 = {192: 64, 384: 32, 768: 16, 512: 16}
# codes of ffs_dispatch_report (include/ffsubsync_amd.h)
PASS_A, PASS_A3 = 1, 2
MID, MID_SEG_ONE_1, MID_SEG_ONE_4, MID_SEG_PIPE = 1, 2, 3, 4
LAST_FULL, LAST_C3, LAST_PRUNED = 1, 2, 3
AMP = (0.0, 1.0 / 1.001)
UNIT = (0.0, 1.0)
BURST = (0.5, 1.0)
HEAD = np.array([1] * 20 + [0] * 3 + [1] * 27, np.uint8)  # the reference's first 50 samples; mirrored, its last 50

Run = namedtuple("Run", "setting kind dtype idx vset")  # one solve: setting a-e, noise/ties, u1/u8/f32/mixed, candidate indices


def geometry(n):
    """(N1, N2) of a plan of length n: rows of at most 4096 points, columns of 16 (48 for 3*2^k) or more."""
    if n % 3 == 0:
        n2 = 4096 if n >= 48 * 4096 else n // 48
    else:
        n2 = min(n // 16, 4096)
    return n // n2, n2


def window(n, setting):
    n2 = geometry(n)[1]
    return {"a": None, "b": n2 // 2 - 1, "c": n2 + 5, "d": n2 // 2 - 1, "e": n2 // 2 - 1}[setting]


def env(setting):
    return {"d": {"FFS_DISABLE_PRUNED_PASS_C": "1"}, "e": {"FFS_DISABLE_SEGMENTED": "1"}}.get(setting, {})


def sizes(n, vset="fill"):
    if vset == "long":
        return 9 * n // 10, 9 * n // 10 - 17
    r = n // 2 + 1000
    return r, n - 3 - r


def first_tile(n):
    """Column tile width of the windowless last pass at this length."""
    n1 = geometry(n)[0]
    return TILE3.get(n1, TILE[n1])


# ---- problems -------------------------------------------------------------------------------------------------------------
def _plant(rng, ref, s_len, d):
    """Noise of length s_len that equals ref[i + d] on the middle nine tenths of the overlap at lag d."""
    sub = _noise(rng, s_len)
    i0, i1 = max(0, -d), min(s_len, ref.size - d)
    assert i1 - i0 >= 200, (s_len, d)
    a, b = i0 + (i1 - i0) // 20, i1 - (i1 - i0) // 20
    sub[a:b] = ref[a + d:b + d]
    return sub


@functools.lru_cache(maxsize=None)
def noise_problem(n, vset="fill"):
    """(ref01, [cand01], ref_levels, [cand_levels], [planted lag]): twelve candidates on the segmented lengths, eight
    elsewhere."""
    rng = np.random.RandomState(n % 100003 + (7 if vset == "long" else 0))
    R, S = sizes(n, vset)
    n2 = geometry(n)[1]
    ref = _noise(rng, R)
    ref[np.arange(R) % 31 >= 23] = 0  # no run of ones longer than 23 samples ...
    ref[:50] = HEAD                   # ... but for 27 at either end, in mirrored patterns: only there the same burst
    ref[50:58] = 0                    # puts all of its 47 ones on ones
    ref[R - 50:] = HEAD[::-1]
    ref[R - 58:R - 50] = 0
    c = first_tile(n)
    w = window(n, "b")
    lags = [0, -1, 2 * n2, -n2 - 1, c - 1, c]
    levels = [UNIT, UNIT, AMP, UNIT, UNIT, UNIT]
    cands = [_plant(rng, ref, S - 37 * j, d) for j, d in enumerate(lags)]
    for j, head in ((6, False), (7, True)):  # the far ends
        s_len = S - 37 * j
        sub = np.zeros(s_len, np.uint8)
        if head:
            sub[:50] = HEAD[::-1]
        else:
            sub[s_len - 50:] = HEAD
        cands.append(sub)
        levels.append(BURST)
        lags.append(R - 50 if head else 50 - s_len)
    if n in SEGMENTED:  # the pruned pass's tile edge (16 columns at these N1) and the window's own edges
        for j, d in ((8, 15), (9, 16), (10, -w), (11, w)):
            cands.append(_plant(rng, ref, S - 37 * j, d))
            levels.append(UNIT if j != 10 else AMP)
            lags.append(d)
    return ref, cands, UNIT, levels, lags


@functools.lru_cache(maxsize=None)
def ties_problems(n, vset="fill"):
    """Two problems of three candidates each, as (ref01, [cand01], ref_levels, [cand_levels]): flat tops of 41 and 700
    tied lags (plateaus from lag 5 on), and a shared period with ties at d = 11 (mod P), one of them on d = N2 - 1."""
    rng = np.random.RandomState(n % 100019 + 1)
    R, S = sizes(n, vset)
    n2 = geometry(n)[1]
    P = 3072 if S >= 3072 else 1024
    s_f = S // P * P
    r_f = s_f + (R - S)  # (a longer reference lets lags of partial overlap beat the plateau)
    ref_f, wide = _flat_top(r_f, s_f, P, 900, 201, start=5)
    _, narrow = _flat_top(r_f, s_f, P, 900, 860, start=5)
    flat = (ref_f, [wide, narrow, wide[: max(P, s_f - P)]], UNIT, [UNIT, UNIT, AMP])
    P2 = n2 // 4 - 3
    ref_p, sub = _shared_period(rng, R, S - min(3 * n2, S // 2), P2, (n2 - 1) % P2)
    periodic = (ref_p, [sub, np.roll(sub, 7), sub], UNIT, [UNIT, UNIT, AMP])
    return flat, periodic


def problems(n, run):
    """The problems of one solve as (name, ref01, [cand01], ref_levels, [cand_levels]) (test_gpu_exact.py's form)."""
    if run.kind == "noise":
        ref, cands, rl, cl, _ = noise_problem(n, run.vset)
        return [("noise", ref, [cands[j] for j in run.idx], rl, [cl[j] for j in run.idx])]
    return [(name, p[0], [p[1][j] for j in run.idx], p[2], [p[3][j] for j in run.idx])
            for name, p in zip(("flat", "periodic"), ties_problems(n, run.vset))]


@functools.lru_cache(maxsize=None)
def _record(n, vset, kind, which, j, max_off):
    """The exact record of candidate j of one problem (cached: settings and candidate subsets share them)."""
    if kind == "noise":
        ref, cands, rl, cl, _ = noise_problem(n, vset)
    else:
        ref, cands, rl, cl = ties_problems(n, vset)[which]
    return er.candidate(_spectrum(n, vset, kind, which), cands[j], rl, cl[j], max_off)


@functools.lru_cache(maxsize=4)
def _spectrum(n, vset, kind, which):
    ref = noise_problem(n, vset)[0] if kind == "noise" else ties_problems(n, vset)[which][0]
    return er.RefSpectrum(np.asarray(ref) != 0)


def expected(n, run):
    """[(candidate records, pair record)] of one solve, as exact_reference.solve returns them (filter = window)."""
    max_off = window(n, run.setting)
    out = []
    for which in range(1 if run.kind == "noise" else 2):
        recs = [dict(_record(n, run.vset, run.kind, which, j, max_off)) for j in run.idx]
        out.append((recs, er.pair(recs, max_off)))
    return out


# ---- what a solve is expected to launch ------------------------------------------------------------------------------------
def expected_dispatch(n, run, sub_batches=1):
    """ffs_dispatch_report of one solve, from the description of the dispatch (csrc/ffsalign.hip)."""
    n_cand = len(run.idx)
    seg = n in SEGMENTED and run.setting in "bc"
    m = n // 3 if seg else n
    n1, n2 = geometry(m)
    half_ref = n2 == 4096
    half_last = half_ref and n_cand % 2 == 1
    bits = run.dtype in ("u1", "mixed")
    a3 = bits and n1 in C3_N1
    pair_ok = run.dtype == "u1" and half_ref and half_last and (a3 or n1 % 3 != 0)
    slots = (n_cand + 1) // 2
    pruned = run.setting in "bce"
    return dict(transform_sub_batches=sub_batches, transform_length=m, n1=n1, n2=n2,
                seg_blocks=(3 if run.vset == "long" else 2) if seg else 0,
                half_flags=(1 if half_ref else 0) | (2 if half_last else 0),
                pass_a_family=PASS_A3 if a3 else PASS_A, pass_a_ref_family=PASS_A if run.dtype == "mixed" else 0,
                pass_a_paired=0 if not pair_ok else (1 if n_cand == 1 else 2),
                mid_family=MID if not seg else MID_SEG_ONE_1 if slots == 1 else MID_SEG_ONE_4 if slots <= 4 else MID_SEG_PIPE,
                last_family=LAST_PRUNED if pruned else LAST_C3 if n1 in C3_N1 else LAST_FULL,
                sweep_family=LAST_PRUNED if pruned else LAST_FULL)


# ---- the table ---------------------------------------------------------------------------------------------------------------
BIG = [1 << 22, 1 << 23, 1 << 24, 3 << 20]  # three candidates only: the CPU reference dominates there
UNIT_IDX = (0, 1, 3, 4, 5)  # candidates with levels (0, 1): what float inputs hold bit-exact
MIXED = {1 << 14: "a", 1 << 18: "a", 3 << 13: "a", 3 << 17: "b"}  # F64 reference, bit-packed candidates (row_sel launches)


def _first_of_n1(n):
    n1 = geometry(n)[0]
    return n == min(x for x in LENGTHS if geometry(x)[0] == n1)


@functools.lru_cache(maxsize=None)
def runs(n):
    """Every solve of plan length n."""
    N = lambda setting, dtype, idx, vset="fill": Run(setting, "noise", dtype, tuple(idx), vset)
    T = lambda setting, dtype, idx, vset="fill": Run(setting, "ties", dtype, tuple(idx), vset)
    out = []
    if n in BIG:
        three = (3, 5, 6)
        out += [N("a", "u1", three), N("b", "u1", three), N("a", "u8", three[:2]), N("b", "u8", three),
                T("a", "u1", (0,)), T("b", "u8", (0,)), N("a", "f32", (3, 5))]
        if n == 3 << 20:  # the three segmented mid kernels need 1, 3 and 9 candidates
            out += [N("b", "u1", (1,)), N("b", "u1", range(9))]
    else:
        out += [N("a", "u1", range(1, 8)), N("a", "u1", (0,)), N("a", "u8", (0, 1, 2)), N("a", "u8", (6, 7)),
                N("b", "u1", (0, 1)), N("b", "u1", (4, 5, 6)), N("b", "u8", range(0, 7)), N("b", "u1", (2,)),
                N("c", "u1", (0, 3, 5)), N("d", "u1", (0, 1, 4)), N("d", "u1", (0, 5)),
                T("a", "u1", (0, 1, 2)), T("a", "u8", (0, 1)), T("b", "u1", (0, 1, 2)), T("b", "u8", (0,)), T("c", "u1", (0, 1)),
                T("d", "u1", (0, 1, 2))]
        if _first_of_n1(n):
            out += [N("a", "f32", (0, 4, 5)), N("b", "f32", (0, 1)), T("a", "f32", (0, 1))]
    if n in SEGMENTED:
        out += [N("e", "u1", range(0, 7)), N("e", "u1", (0, 1)), N("e", "u1", (5,)), T("e", "u1", (0, 1, 2))]
        if n not in BIG:
            out += [N("b", "u1", range(k)) for k in (8, 9, 10, 12)]
            out += [N("b", "u8", range(9)), N("b", "f32", UNIT_IDX), N("c", "u1", range(10))]
        if n == 3 << 18:
            out += [N("b", "u1", range(k)) for k in (1, 3, 7)]
    if n in THREE_BLOCK:
        out += [N("b", "u1", (0,), "long"), N("b", "u1", range(0, 7), "long"), N("b", "u1", range(9), "long"),
                N("b", "u8", range(12), "long"), T("b", "u1", (0, 1, 2), "long")]
    if n in MIXED:
        out += [N(MIXED[n], "mixed", UNIT_IDX[:3]), N(MIXED[n], "mixed", UNIT_IDX[:4]), T(MIXED[n], "mixed", (0, 1))]
    return out


def margin(n, r_len, s_len, ref_levels, cand_levels):
    """The nominee margin of a candidate: eps * log2 N * sqrt(R S) * |s|max * |r|max over the mapped
    levels 2x - 1 -- lags whose fp32 value lies within it of the maximum are re-scored exactly, so the fp32 chain's own
    error has to stay below it for the true peak to be nominated at all."""
    a_s = max(abs(2 * cand_levels[0] - 1), abs(2 * cand_levels[1] - 1))
    a_r = max(abs(2 * ref_levels[0] - 1), abs(2 * ref_levels[1] - 1))
    return 5.9604645e-08 * int(np.floor(np.log2(n))) * np.sqrt(float(r_len) * float(s_len)) * a_s * a_r
