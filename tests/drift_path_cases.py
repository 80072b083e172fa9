"""TEST INFRASTRUCTURE ONLY -- the problems and settings shared by tests/test_drift_path_reference_host.py (the models
on the CPU) and tests/test_gpu_drift_optimum.py (the device): the shape lists of tests/test_gpu_split_optimum.py with
bits from ``drift_path_reference.drifting_bits``, so that optimal paths hold real moves and real jumps."""
import math
import sys

import numpy as np

import drift_path_reference as dpr
import piecewise_reference as pw
from test_gpu_split_optimum import FULL, I0, I1, RANGE_GROUPS, WINDOW_GROUPS

DBL_MAX = sys.float_info.max
TILE = 2048  # lags per workgroup of the range aligner's step kernel (RANGE_TILE of csrc/ffs_split_range.h)

# (P, max_step, Q): every one runs on every group
SETTINGS = [
    (60.0, 2, 1.0),  # the defaults' neighbourhood
    (3.0, 7, 0.25),
    (math.inf, 7, 0.0),  # free moves, no jumps
    (DBL_MAX, 7, 0.0),  # records byte-identical to P = inf
    (0.5, 1, 16.0),  # Q a > P: the move is dominated by the jump
    (8192.0, 3, 0.0),
    (0.0, 2, 1.0),  # free jumps: "ties do not jump"
    (-0.0, 2, 1.0),  # byte-identical to P = 0
    (60.0, 0, 1.0),  # the split aligners' records
]
I_INF, I_MAX, I_ZERO, I_NZERO, I_SPLIT, I_U8 = 2, 3, 6, 7, 8, 0
assert SETTINGS[I_INF][0] == math.inf and SETTINGS[I_MAX][0] == DBL_MAX and SETTINGS[I_SPLIT][1] == 0
assert SETTINGS[I_ZERO][0] == 0.0 and math.copysign(1.0, SETTINGS[I_NZERO][0]) < 0

# range groups beyond RANGE_GROUPS, as (K, pairs_in_flight, [(R, S, reference levels, subtitle levels, (lag_lo, lag_hi),
# lag index the drift starts at or None, every or None)]): five lags under max_step = 7, and paths that step across a
# tile edge of the step kernel in either direction (two lags per block; the true lag index is a multiple of TILE minus 1
# after 7 steps, in the file's fourth block, or the multiple itself on the way down)
EXTRA_RANGE_GROUPS = [
    (256, None, [(6000, 256 * 10, I0, I0, (-500, 1500), None, None), (3000, 1500, I0, I0, (10, 14), None, None),
                 (2000, 900, I1, I0, (-7, -3), None, None),
                 (9000, 256 * 8 + 31, I0, I0, (-100, 4400), TILE - 1 - 7, 128),
                 (9000, 256 * 8 + 1, I0, I1, (-2500, 2500), 2 * TILE + 7, -128),
                 (9000, 256 * 6 + 33, I1, I1, (300, 300 + 2 * TILE), TILE - 1 - 7, 128)]),
]

SMOOTH_SETTINGS = [(1, 0, 64.0), (2, 2, 0.5), (3, 16, 0.0)]  # (knot_blocks, radius, bend_cost)
SMOOTH_DRIFT_SETTINGS = [SETTINGS[0], SETTINGS[2]]
SMOOTH_WINDOW_GROUPS = [2, 5]  # indices into WINDOW_GROUPS: K = 288 / W = 31 and K = 1024 / W = 1000
SMOOTH_RANGE_GROUPS = [1, 3]  # indices into all_range_groups(): K = 288 and K = 1024
PARITY_WINDOW_GROUP = 5  # its pairs also run on the range aligner at [-W + 1, W]


def all_range_groups():
    """RANGE_GROUPS in the extra groups' form, then the extra groups."""
    out = [(k, pif, [spec + (None, None) for spec in specs]) for k, pif, specs in RANGE_GROUPS]
    return out + EXTRA_RANGE_GROUPS


def make_pair(seed, R, S, r_lv, s_lv, lo, hi, k, with_break, start=None, every=None):
    """One problem over the lag set [lo, hi]: the subtitle drifts about 1.5 lags per block (as far as the lag set has
    room; in either direction), with a break of 5 to 300 lags (as far as the lag set has room) where asked."""
    rng = np.random.RandomState(seed)
    L = hi - lo + 1
    room = L - 1
    if every is None:
        steps = min(room, max(1, (3 * S) // (2 * k)))
        every = S + 1 if steps == 0 else max(1, -(-S // steps))
        if rng.rand() < 0.5:
            every = -every
    moved = (S - 1) // every  # the drift at the last sample (negative for a downward drift)
    if start is None:
        first_lo, first_hi = lo - min(moved, 0), hi - max(moved, 0)
        start = int(rng.randint(first_lo, first_hi + 1)) - lo if first_hi >= first_lo else 0
    shift = lo + int(start)
    break_at, break_by = None, 0
    if with_break and S > k:
        break_at = int(rng.randint(k // 2, S - k // 4))
        side = int(rng.choice([-1, 1])) * int(rng.randint(5, 301))
        break_by = int(np.clip(shift + moved + side, lo, hi)) - (shift + moved)
    rb, sb = dpr.drifting_bits(rng, R, S, shift, every, break_at, break_by)
    return dict(rb=rb, sb=sb, r_lv=r_lv, s_lv=s_lv, ref=np.where(rb, r_lv[1], r_lv[0]),
                sub=np.where(sb, s_lv[1], s_lv[0]), lo=lo, hi=hi, k=k)


def _broken(sub_lens, k):
    """The pair of a group that gets the break: the first of those with the most blocks (a third of all pairs; a break
    needs blocks on both sides of it, and moves next to it, to show as a jump AND moves in one solution)."""
    blocks = [-(-S // k) for S in sub_lens]
    return blocks.index(max(blocks))


def window_pairs(gi):
    k, w, _, specs = WINDOW_GROUPS[gi]
    broken = _broken([spec[1] for spec in specs], k)
    return [make_pair(18000 + 100 * gi + i, R, S, r_lv, s_lv, -w + 1, w, k, i == broken and w >= 6)
            for i, (R, S, r_lv, s_lv) in enumerate(specs)]


def range_pairs(gi):
    k, _, specs = all_range_groups()[gi]
    out, broken = [], _broken([spec[1] for spec in specs], k)
    for i, (R, S, r_lv, s_lv, rng_, start, every) in enumerate(specs):
        lo, hi = (-(S - 1), R - 1) if rng_ == FULL else rng_
        out.append(make_pair(19000 + 100 * gi + i, R, S, r_lv, s_lv, lo, hi, k, i == broken and hi - lo >= 11, start,
                             every))
    return out


def reference(pr):
    return pw.Reference(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], pr["lo"], pr["hi"])


class Tally:
    """What keeps the checks from being vacuous, counted over (problem, setting) solutions that passed them."""

    def __init__(self):
        self.checked = self.with_move = self.with_jump = self.with_both = self.with_tie = 0

    def add(self, ref, setting, block_offsets, block_jump):
        moves, jumps, ties = dpr.path_facts(ref, *setting, block_offsets, block_jump)
        self.checked += 1
        self.with_move += moves > 0
        self.with_jump += jumps > 0
        self.with_both += moves > 0 and jumps > 0
        self.with_tie += ties > 0

    def merge(self, other):
        for name in ("checked", "with_move", "with_jump", "with_both", "with_tie"):
            setattr(self, name, getattr(self, name) + getattr(other, name))
        return self

    def counts(self):
        return dict(checked=self.checked, move=self.with_move, jump=self.with_jump, both=self.with_both,
                    tie=self.with_tie)

    def enough(self):
        return self.with_move >= 30 and self.with_jump >= 30 and self.with_both >= 10 and self.with_tie >= 5
