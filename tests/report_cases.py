"""TEST INFRASTRUCTURE ONLY -- the problems and settings shared by tests/test_report_reference_host.py (the models on
the CPU) and tests/test_gpu_report_optimum.py (the device): the shape lists of tests/test_gpu_split_optimum.py and
tests/drift_path_cases.py, plus the groups that exist for the reports alone -- more than 1024 blocks, more than eight
segments or pieces, an offset spread beyond one chunk of the flat maximum, a shift set of one shift, neighbour shifts
outside the shift set at new block lengths."""
import math

import numpy as np

import drift_path_cases as cases
import drift_path_reference as dpr
import piecewise_reference as pw
from test_gpu_drift_report import _edge_problem
from test_gpu_split_optimum import I0, I1, RANGE_GROUPS, WINDOW_GROUPS, _range_pairs

# the segment report's settings on every window group: the defaults' neighbourhood, many cheap moves, free moves with no
# jumps, and the max_step = 0 "split records"
SEGMENT_SETTINGS = [cases.SETTINGS[0], cases.SETTINGS[1], cases.SETTINGS[2], cases.SETTINGS[8]]
PIECE_PENALTIES = [3.0, 60.0]
TOP_KS = (1, 3, 8)

# refinement: (radius, beta) -- every radius with every beta
REFINE_RADII = (1, 300, 131072)
REFINE_BETAS = (None, 0.0, 0.25, 64.0)
REFINE_WINDOW_GROUPS = [1, 2, 3, 4, 6, 7, 8]  # indices into WINDOW_GROUPS: every group at K = 288, 800, 2080, 32768
REFINE_SETTINGS = (0, 1, 3)  # indices into SEGMENT_SETTINGS: the settings whose paths can hold jumps (P finite)


def peak_args(call, n_full):
    """(top_k, exclusion distance) of report call number ``call``: the entry points take one of each per call, so they
    vary per (group, setting) over {1, 3, 8} x {1, 50, a value >= n_lags} (``n_full`` = the lag set's size)."""
    combo = call % 9
    return TOP_KS[combo % 3], (1, 50, max(int(n_full), 51))[combo // 3]


def _pair(rb, sb, k, lo, hi, r_lv=I0, s_lv=I0):
    return dict(rb=rb, sb=sb, r_lv=r_lv, s_lv=s_lv, ref=np.where(rb, r_lv[1], r_lv[0]),
                sub=np.where(sb, s_lv[1], s_lv[0]), lo=lo, hi=hi, k=k)


def _runs(rng, n, run=40.0):
    seg = np.maximum(1, rng.geometric(1.0 / run, size=n // 4 + 16))
    rb = np.repeat(rng.rand(seg.size) < 0.45, seg)[:n]
    return np.concatenate([rb, np.zeros(n - rb.size, bool)])


def piecewise_bits(rng, R, S, cuts, shifts, flip, period=None):
    """A reference of random runs (repeated with ``period`` when given) and a subtitle that follows it at shifts[i]
    between cuts[i - 1] and cuts[i], a fraction ``flip`` of its samples inverted; both levels present in both."""
    rb = _runs(rng, R) if period is None else np.tile(_runs(rng, period), R // period + 1)[:R]
    i = np.arange(S)
    idx = i + np.asarray(shifts)[np.searchsorted(np.asarray(cuts), i, side="right")]
    sb = np.zeros(S, bool)
    ok = (idx >= 0) & (idx < R)
    sb[ok] = rb[idx[ok]]
    sb ^= rng.rand(S) < flip
    sb[0], sb[1] = True, False
    rb[0], rb[1] = True, False
    return rb, sb


def long_pair():
    """More than 1024 blocks: K = 256, W = 40, S = 1030 * 256 + 31, breaks at samples 1023 * 256, 1024 * 256 and
    1025 * 256 + 100 (a jump at the last block of the first 1024-block chunk, at the first of the second and one past
    it), and nine more every 100 blocks so that the pair takes two rounds of eight segments."""
    k, w = 256, 40
    S = 1030 * k + 31
    cuts = [100 * j * k for j in range(1, 10)] + [1023 * k, 1024 * k, 1025 * k + 100]
    shifts = [(-30, -10, 10, 30, 0, 20, -20)[j % 7] for j in range(len(cuts) + 1)]
    rb, sb = piecewise_bits(np.random.RandomState(21001), S + 200, S, cuts, shifts, flip=0.01)
    return _pair(rb, sb, k, -w + 1, w)


def extra_window_groups():
    """{name: (K, W, pairs, [(P, max_step, Q)])} of the groups added for the segment report."""
    out = {}
    out["long"] = (256, 40, [long_pair()], [(3.0, 7, 0.25), (3.0, 0, 1.0)])
    # more than 8 segments: 24 blocks, a break every second block, P = 0.5; next to it a pair of one segment, whose
    # slots past the count return early beside the full ones
    k, w = 256, 200
    S = 24 * k
    cuts = [2 * j * k for j in range(1, 12)]
    shifts = [(-150, 90, -40, 160, 10, -190, 120, -80, 199, -120, 60, -10)[j] for j in range(12)]
    rb, sb = piecewise_bits(np.random.RandomState(21002), S + 400, S, cuts, shifts, flip=0.02)
    rb1, sb1 = piecewise_bits(np.random.RandomState(21003), 5 * k + 300, 5 * k + 7, [], [33], flip=0.0)
    out["rounds"] = (k, w, [_pair(rb, sb, k, -w + 1, w), _pair(rb1, sb1, k, -w + 1, w)],
                     [(0.5, 1, 16.0), (0.5, 0, 1.0)])
    # o_max - o_min >= 1024: the subtitle drifts 7 lags per block over 160 blocks; the second pair's reference has
    # period 512, so the constant-lag curve repeats every 512 lags and its maxima tie across the 1024-lag chunks
    k, w = 256, 1000
    S = 160 * k + 1
    rb, sb = dpr.drifting_bits(np.random.RandomState(21004), S + 1200, S, -600, 36)
    prng = np.random.RandomState(21005)
    tile = _runs(prng, 512)
    rp = np.tile(tile, (S + 1200) // 512 + 1)[:S + 1200]
    i = np.arange(S)
    sp = rp[i - 200 + i // 36].copy()
    sp[:200] = False  # the samples whose partner lies before the reference at the path's own lag
    rp[0], rp[1] = True, False
    out["wide"] = (k, w, [_pair(rb, sb, k, -w + 1, w), _pair(rp, sp, k, -w + 1, w)],
                   [(math.inf, 7, 0.0), (8192.0, 7, 0.0)])
    # a shift set of one shift: W = 1 (lags 0 and 1), a path that visits both
    k, w = WINDOW_GROUPS[0][0], WINDOW_GROUPS[0][1]
    assert w == 1
    S = 4 * k + 5
    rb, sb = pw.two_offset_bits(np.random.RandomState(21006), S + 50, S, (0, 1), flip=0.01, cut=2 * k)
    out["single"] = (k, w, [_pair(rb, sb, k, 0, 1)], [(math.inf, 7, 0.0), (60.0, 2, 1.0)])
    # neighbour shifts outside the shift set (NaN inside a pair), at K = 288 and K = 800
    for name, (seed, k, w) in (("edge288", (3, 288, 40)), ("edge800", (3, 800, 40))):
        pr = _edge_problem(seed, k, w)
        out[name] = (k, w, [_pair(pr["rb"], pr["sb"], k, -w + 1, w)], [(pr["p"], pr["s"], pr["q"])])
    return out


EXTRA_WINDOW_NAMES = ("long", "rounds", "wide", "single", "edge288", "edge800")


def extra_range_groups():
    """{name: (K, pairs)} of the pairs added for the piece report over a range."""
    out = {}
    # pieces of 32 768-sample blocks hold 1024 subtitle words: more than one 512-word work item each
    k = 32768
    S = 3 * k + 33
    R = 70000
    rb, sb = pw.two_offset_bits(np.random.RandomState(22001), R, S, (500, -700), flip=0.003, run=300.0, cut=2 * k)
    out["words"] = (k, [_pair(rb, sb, k, -(S - 1), R - 1, I0, I1)])
    # more than 8 pieces: 24 blocks, a break every second block
    k = 256
    S = 24 * k
    cuts = [2 * j * k for j in range(1, 12)]
    shifts = [(-450, 900, -40, 1400, 10, -190, 1200, -80, 700, -320, 60, 1490)[j] for j in range(12)]
    rb, sb = piecewise_bits(np.random.RandomState(22002), S + 1600, S, cuts, shifts, flip=0.02)
    out["rounds"] = (k, [_pair(rb, sb, k, -500, 1500, I1, I0)])
    return out


EXTRA_RANGE_NAMES = ("words", "rounds")


def given_offsets():
    """(K, pair, block offsets) for the piece report of GIVEN offsets (``cut_report.report_batch``): the "rounds" pair at
    its planted offsets, but two pieces a few lags beside theirs.  A solve puts every piece at the maximum of its own
    curve (the largest lag on ties, as peak 1), so with integer levels only given offsets can raise OWN_NOT_PEAK."""
    k, (pr,) = extra_range_groups()["rounds"]
    planted = (-450, 900, -40, 1400, 10, -190, 1200, -80, 700, -320, 60, 1490)
    offsets = np.repeat(np.array(planted, dtype=np.int32), 2)
    offsets[4:6] += 3
    offsets[20:22] -= 2
    return k, pr, offsets


def range_pairs(gi):
    """The pairs of RANGE_GROUPS[gi] as tests/test_gpu_split_optimum.py builds them, with their block length."""
    k = RANGE_GROUPS[gi][0]
    return [dict(pr, k=k) for pr in _range_pairs(gi)]


def flagged_pair():
    """Hand-made jump flags for the refinement: set where the offset does not change (block 2) and in two adjacent
    blocks (4 and 5), so that the windows between them are clipped at the midpoints, K / 2 samples wide.  Returns
    (pair, block offsets, jump flags)."""
    k = 288
    S = 8 * k + 17
    rb, sb = piecewise_bits(np.random.RandomState(23001), S + 300, S, [4 * k + 60], [25, -40], flip=0.03)
    offsets = np.array([25, 25, 25, 26, -40, -41, -40, -40, -40], dtype=np.int32)
    jump = np.array([0, 0, 1, 0, 1, 1, 0, 0, 0], dtype=np.uint8)
    return _pair(rb, sb, k, -100, 100), offsets, jump


def conditions_hold(seg, piece, jumps):
    """What the comparison must have covered: ``seg`` / ``piece`` the ``report_reference.Facts`` of every segment and
    piece record compared, ``jumps`` {K: jumps refined}."""
    both = lambda name: getattr(seg, name) + getattr(piece, name)
    return (seg.records >= 40 and seg.both_neighbours >= 15 and seg.stepping >= 10
            and len(seg.many_tags | piece.many_tags) >= 3 and seg.first_1024 >= 1 and seg.single_shift >= 1
            and seg.nan_inside >= 2 and seg.flat_second_chunk >= 1 and both("second_peak") >= 5
            and both("one_peak_by_exclusion") >= 5 and both("own_not_peak") >= 2
            and sum(jumps.values()) >= 20 and sum(1 for v in jumps.values() if v > 0) >= 4)
