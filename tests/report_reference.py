"""TEST INFRASTRUCTURE ONLY -- an independent statement of what is computed AFTER a solve: the drift solve's segment
path report (csrc/ffs_drift_report.h), the per-piece report over a lag range (csrc/ffs_cut_report.h) and, through the
segment table, the numbering the refinement kernels share.

The report models (drift_report_model, cut_report_model, split_report_model) read the same per-block count table the
kernels read and restate their index arithmetic, so a mistake they share goes unseen.  This module shares nothing with
them.  It stands on ``piecewise_reference.Reference``, whose ``rows[b, j]`` are the block scores I_b(d) from their
definition (mapped levels 2 * level - 1, direct sums or an integer FFT rounded to integers, samples outside the
reference absent, exactly 0 where nothing overlaps) and whose ``interval(a, c)`` is I over the blocks [a, c), and states
over the lag set [lo, hi] (the window case is [-W + 1, W]):

  segment table   maximal runs [f, e) of blocks with no flagged block after the first; samples [f K, min(e K, S));
                  first / last / min / max of the run's block offsets.  A piece is a maximal run of EQUAL offsets.
  path curve      p(delta) = sum_b rows[b, (o_b + delta) - lo] for delta in [lo - o_min, hi - o_max]: the
                  n_lags = (hi - lo + 1) - (o_max - o_min) shifts of the whole path that keep every block inside the
                  lag set.  A piece's curve is interval(f, e) over the whole lag set (n_lags = hi - lo + 1).
  own, prev, next p(0); p at the shift last_(i-1) - first_i that continues the previous segment and at
                  first_(i+1) - last_i that continues the next; NaN without that neighbour or outside the shift set.
                  For a piece: its curve at its own and at the neighbours' offsets.
  flat            max over d in [o_min, o_max] of sum_b rows[b, d], the largest d on ties.
  peaks           round k takes the largest value among the indices at least E from every earlier peak, the largest
                  index on ties, until top_k peaks are taken or no index is left.
  flags           FLAT iff every value of the curve is equal; OWN_NOT_PEAK iff there is no peak or peak 1 is not
                  shift 0 (for a piece: not the piece's offset).
  mean, std       numpy's float64 mean and population standard deviation of the curve.

Exactness.  With integer mapped levels (``pw.integer_levels``) every term is an integer and every sum stays below 2^53,
so a sum of block scores and the kernels' one expression of summed counts are the same number: scores, peak positions,
flags and the exact 0.0 of an empty overlap compare as float64 bit patterns.  Mean and std compare within
1e-12 * max(|mean|, std), the margin tests/test_gpu_split_optimum.py uses for the same device helper.

Non-integer levels.  ``tolerance`` bounds what the reference's value and a correct fp64 evaluation of the same real sum
can differ by, as ``Reference.tolerance`` does, counted in roundings of at most eps * sum|terms| each (sum|terms| =
``Reference.abs_terms``, the bound of the sum of |products| of any slice at any lag, so of every partial sum too):
  - a block score or an interval row is within 3 roundings of its real sum (``Reference``'s docstring); the errors of the
    blocks of a segment are relative to their own blocks' terms, so together they stay within 3 roundings of the whole;
  - a segment sum of n <= B block scores adds n - 1 times, each addition one rounding of a partial sum;
  - the kernels' expression of four products and three additions of the summed counts makes 7 roundings;
so (B + 9) eps sum|terms| covers both sides; ``tolerance`` uses (B + 10).  The bound is this reference's own property and
is never tuned on device output.  Within it a peak or the flat maximum may sit at another index: then the reference's two
contenders must lie within the bound of each other, and the comparison of later peaks stops (the rule of
tests/test_gpu_quality.py); mean and std get the bound added to their margin (a mean of values within the bound is
within the bound, and so is the root mean square of their deviations).
"""
import math

import numpy as np

import piecewise_reference as pw

EPS = pw.EPS
FLAT, OWN_NOT_PEAK = 1, 4
MAX_PEAKS = 8
FLAT_CHUNK = 1024  # lags of [o_min, o_max] the device's flat maximum takes at a time (a fact for the tallies only)
MOMENT_MARGIN = 1e-12

SEGMENT_INT = ("first_block", "end_block", "start_sample", "end_sample", "first_offset", "last_offset", "min_offset",
               "max_offset")
PIECE_INT = ("first_block", "end_block", "start_sample", "end_sample", "offset")


def tolerance(ref):
    """0 on the exact path; otherwise (B + 10) eps sum|terms|, see the module docstring."""
    return 0.0 if ref.exact else (ref.B + 10) * EPS * ref.abs_terms


# ---- tables ----------------------------------------------------------------------------------------------------------

def segment_table(block_offsets, block_jump, block_samples, sub_len):
    """One dict per segment (the fields of SEGMENT_INT), in plain Python."""
    o = [int(x) for x in block_offsets]
    jump = [int(x) for x in block_jump]
    k, S = int(block_samples), int(sub_len)
    assert len(o) == len(jump) == (S + k - 1) // k
    out, f = [], 0
    for b in range(1, len(o) + 1):
        if b == len(o) or jump[b] != 0:
            run = o[f:b]
            out.append(dict(first_block=f, end_block=b, start_sample=f * k, end_sample=min(b * k, S),
                            first_offset=run[0], last_offset=run[-1], min_offset=min(run), max_offset=max(run)))
            f = b
    return out


def piece_table(block_offsets, block_samples, sub_len):
    """One dict per piece (the fields of PIECE_INT), in plain Python."""
    o = [int(x) for x in block_offsets]
    k, S = int(block_samples), int(sub_len)
    assert len(o) == (S + k - 1) // k
    out, f = [], 0
    for b in range(1, len(o) + 1):
        if b == len(o) or o[b] != o[f]:
            out.append(dict(first_block=f, end_block=b, start_sample=f * k, end_sample=min(b * k, S), offset=o[f]))
            f = b
    return out


# ---- curves and what is derived from them ----------------------------------------------------------------------------

def path_curve(ref, first_block, end_block, block_offsets):
    """(p over the shift set, the shift of index 0) of the blocks [first_block, end_block) at ``block_offsets``."""
    o = [int(block_offsets[b]) for b in range(first_block, end_block)]
    o_min, o_max = min(o), max(o)
    assert ref.lo <= o_min and o_max <= ref.hi, (o_min, o_max, ref.lo, ref.hi)
    shift_lo, shift_hi = ref.lo - o_min, ref.hi - o_max
    n = shift_hi - shift_lo + 1
    assert n == ref.L - (o_max - o_min) >= 1
    p = np.zeros(n, dtype=np.float64)
    for b, ob in zip(range(first_block, end_block), o):
        j0 = (ob + shift_lo) - ref.lo  # the lag index of block b at the first shift
        p = p + ref.rows[b, j0:j0 + n]
    return p, shift_lo


def flat_curve(ref, first_block, end_block, o_min, o_max):
    """sum_b rows[b, d] for d in [o_min, o_max]."""
    j0, j1 = ref.lag_index(o_min), ref.lag_index(o_max) + 1
    q = np.zeros(j1 - j0, dtype=np.float64)
    for b in range(first_block, end_block):
        q = q + ref.rows[b, j0:j1]
    return q


def last_argmax(values, allowed=None):
    """The largest index of the largest value (among the allowed indices); None when there is none."""
    idx = np.arange(values.size) if allowed is None else np.flatnonzero(allowed)
    if idx.size == 0:
        return None
    top = np.max(values[idx])
    return int(idx[np.flatnonzero(values[idx] == top)[-1]])


def greedy_peaks(values, top_k, exclusion):
    """[(value, index)]: the greedy peak rounds, one literal round at a time."""
    allowed = np.ones(values.size, dtype=bool)
    index = np.arange(values.size)
    out = []
    for _ in range(int(top_k)):
        j = last_argmax(values, allowed)
        if j is None:
            break
        out.append((float(values[j]), j))
        allowed &= np.abs(index - j) >= int(exclusion)
    return out


def _summary(curve, top_k, exclusion):
    return dict(curve=curve, n_lags=int(curve.size), mean=float(np.mean(curve)), std=float(np.std(curve)),
                flat=bool(np.all(curve == curve[0])), peaks=greedy_peaks(curve, top_k, exclusion))


def segment_records(ref, block_offsets, block_jump, top_k, exclusion):
    """The segment path report of one solution: the table's dicts with the curve and everything derived from it."""
    table = segment_table(block_offsets, block_jump, ref.K, ref.S)
    for i, g in enumerate(table):
        curve, shift_lo = path_curve(ref, g["first_block"], g["end_block"], block_offsets)
        g.update(_summary(curve, top_k, exclusion))
        g["shift_lo"] = shift_lo

        def at(shift, curve=curve, shift_lo=shift_lo):
            q = shift - shift_lo
            return float(curve[q]) if 0 <= q < curve.size else math.nan

        g["own_score"] = at(0)
        g["prev_score"] = at(table[i - 1]["last_offset"] - g["first_offset"]) if i > 0 else math.nan
        g["next_score"] = at(table[i + 1]["first_offset"] - g["last_offset"]) if i + 1 < len(table) else math.nan
        g["flat_curve"] = flat_curve(ref, g["first_block"], g["end_block"], g["min_offset"], g["max_offset"])
        j = last_argmax(g["flat_curve"])
        g["flat_score"], g["flat_offset"] = float(g["flat_curve"][j]), g["min_offset"] + j
        g["peak_pos"] = [j + shift_lo for _, j in g["peaks"]]  # as shifts; 0 is the path itself
        g["own_pos"] = 0
    return table


def piece_records(ref, block_offsets, top_k, exclusion):
    """The per-piece report of one solution over the reference's lag set."""
    table = piece_table(block_offsets, ref.K, ref.S)
    for i, g in enumerate(table):
        a, c = g["first_block"], g["end_block"]
        g.update(_summary(ref.interval(a, c), top_k, exclusion))
        g["shift_lo"] = ref.lo
        g["own_score"] = ref.at(a, c, g["offset"])
        g["prev_score"] = ref.at(a, c, table[i - 1]["offset"]) if i > 0 else math.nan
        g["next_score"] = ref.at(a, c, table[i + 1]["offset"]) if i + 1 < len(table) else math.nan
        g["peak_pos"] = [j + ref.lo for _, j in g["peaks"]]  # as offsets
        g["own_pos"] = g["offset"]
    return table


# ---- comparison with a report's records ------------------------------------------------------------------------------

def _bits(x):
    return np.float64(x).tobytes()


def _same_score(got, want, tol):
    got, want = float(got), float(want)
    if math.isnan(want) or math.isnan(got):
        return math.isnan(want) and math.isnan(got)
    return _bits(got) == _bits(want) if tol == 0.0 else abs(got - want) <= tol


class Facts:
    """What keeps the comparison from being vacuous, counted over the records that were compared."""

    NAMES = ("records", "both_neighbours", "stepping", "many", "first_1024", "single_shift", "nan_inside",
             "flat_second_chunk", "second_peak", "one_peak_by_exclusion", "own_not_peak", "no_overlap")

    def __init__(self):
        for name in self.NAMES:
            setattr(self, name, 0)
        self.worst = 0.0  # the largest |score difference| seen on the tolerance path
        self.worst_tol = 0.0
        self.many_tags = set()  # the pairs (by the caller's tag) with more than eight records

    def merge(self, other):
        for name in self.NAMES:
            setattr(self, name, getattr(self, name) + getattr(other, name))
        if other.worst >= self.worst:
            self.worst, self.worst_tol = other.worst, other.worst_tol
        self.many_tags |= other.many_tags
        return self

    def counts(self):
        return {name: getattr(self, name) for name in self.NAMES}


def compare(ref, want, got, count, top_k, kind, facts=None, tag=None):
    """Problems (empty list = none) of a report's records against the reference's: ``want`` = ``segment_records`` /
    ``piece_records``, ``got`` = the pair's row of SEGMENT_REPORT_DTYPE / PIECE_REPORT_DTYPE records (every slot of the
    row: those past ``count`` must be zero), ``kind`` = "segment" or "piece".  ``facts`` counts what was compared, ``tag`` names the pair in its tallies."""
    assert kind in ("segment", "piece")
    pos_field = "peak_shift" if kind == "segment" else "peak_offset"
    bad = []
    tol = tolerance(ref)
    facts = Facts() if facts is None else facts
    if int(count) != len(want):
        return [("count", int(count), len(want))]
    if np.asarray(got[len(want):]).tobytes().strip(b"\0"):
        bad.append(("records past the count are not zero",))
    if len(want) > 8:
        facts.many += 1
        facts.many_tags.add(tag)
    for i, (g, rec) in enumerate(zip(want, got)):
        where = (kind, i, g["first_block"], g["end_block"])
        for name in (SEGMENT_INT if kind == "segment" else PIECE_INT) + ("n_lags",):
            if int(rec[name]) != g[name]:
                bad.append(where + (name, int(rec[name]), g[name]))
        fields = ("own_score", "prev_score", "next_score") + (("flat_score",) if kind == "segment" else ())
        for name in fields:
            if not _same_score(rec[name], g[name], tol):
                bad.append(where + (name, float(rec[name]), g[name], tol))
            elif tol and not math.isnan(g[name]) and abs(float(rec[name]) - g[name]) >= facts.worst:
                facts.worst, facts.worst_tol = abs(float(rec[name]) - g[name]), tol
        if kind == "segment" and int(rec["flat_offset"]) != g["flat_offset"]:
            j = int(rec["flat_offset"]) - g["min_offset"]
            inside = 0 <= j < g["flat_curve"].size
            if tol == 0.0 or not inside or abs(float(g["flat_curve"][j]) - g["flat_score"]) > tol:
                bad.append(where + ("flat_offset", int(rec["flat_offset"]), g["flat_offset"]))
        scale = max(abs(g["mean"]), g["std"])
        for name in ("mean", "std"):
            if not abs(float(rec[name]) - g[name]) <= MOMENT_MARGIN * scale + tol:
                bad.append(where + (name, float(rec[name]), g[name]))
        # peaks: in order; on the tolerance path a peak may sit elsewhere when the reference's contenders are that close
        n_got, diverged = int(rec["n_peaks"]), False
        for z, ((score, j), pos) in enumerate(zip(g["peaks"], g["peak_pos"])):
            if z >= n_got:
                break
            got_pos = int(rec[pos_field][z])
            if got_pos != pos:
                q = got_pos - g["shift_lo"]
                if tol == 0.0 or not 0 <= q < g["n_lags"] or abs(float(g["curve"][q]) - score) > tol:
                    bad.append(where + ("peak position", z, got_pos, pos))
                diverged = True
                break
            if not _same_score(rec["peak_score"][z], score, tol):
                bad.append(where + ("peak score", z, float(rec["peak_score"][z]), score, tol))
        if not diverged:
            if n_got != len(g["peaks"]):
                bad.append(where + ("n_peaks", n_got, len(g["peaks"])))
            if any(float(x) != 0.0 for x in rec["peak_score"][n_got:]) or any(int(x) for x in rec[pos_field][n_got:]):
                bad.append(where + ("peak slots past n_peaks are not zero",))
            own_not_peak = not g["peaks"] or g["peak_pos"][0] != g["own_pos"]
            flags = (FLAT if g["flat"] else 0) | (OWN_NOT_PEAK if own_not_peak else 0)
            if int(rec["flags"]) != flags:
                bad.append(where + ("flags", int(rec["flags"]), flags))
            facts.own_not_peak += own_not_peak
        elif (int(rec["flags"]) & FLAT) != (FLAT if g["flat"] else 0):
            bad.append(where + ("flag FLAT", int(rec["flags"]), g["flat"]))
        # what this record exercised
        facts.records += 1
        facts.both_neighbours += 0 < i < len(want) - 1
        facts.nan_inside += (i > 0 and math.isnan(g["prev_score"])) + (i + 1 < len(want) and math.isnan(g["next_score"]))
        facts.second_peak += len(g["peaks"]) >= 2
        facts.one_peak_by_exclusion += top_k > 1 and len(g["peaks"]) == 1
        facts.single_shift += g["n_lags"] == 1
        facts.first_1024 += g["first_block"] == 1024
        facts.no_overlap += bool(g["flat"] and g["mean"] == 0.0 and g["n_lags"] > 1)
        if kind == "segment":
            facts.stepping += g["min_offset"] != g["max_offset"]
            facts.flat_second_chunk += (g["max_offset"] - g["min_offset"] >= FLAT_CHUNK
                                        and g["flat_offset"] - g["min_offset"] >= FLAT_CHUNK)
    return bad
