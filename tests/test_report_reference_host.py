"""The independent report reference (tests/report_reference.py) on the CPU: its path and piece curves against direct
counting on small problems, and the report models (drift_report_model, cut_report_model) held to it on the exact group
and setting lists of tests/test_gpu_report_optimum.py -- so the case table is shown to hold what the reports have to get
right (segments with both neighbours, stepping paths, more than eight segments, a segment that starts at block 1024, a
shift set of one shift, NaN neighbours inside a pair, a flat maximum that ties across two 1024-lag chunks, second peaks,
exclusion distances that leave one peak, OWN_NOT_PEAK, jumps to refine at four block lengths) before any device runs it.

Every group of the device test runs here: none is left out."""
import functools

import numpy as np

import cut_model as cm
import cut_report_model as crm
import drift_path_cases as cases
import drift_refine_model as jrm
import drift_report_model as drm
import piecewise_reference as pw
import report_cases as rc
import report_reference as rr
import split_model as sm
from test_gpu_split_optimum import F, I0, I1, RANGE_GROUPS, WINDOW_GROUPS


def test_path_curve_equals_direct_counting():
    """Small seeded problems, block lengths off the powers of two, tail blocks, R < S, random stepping paths: the
    reference's path curve == drift_report_model.brute_path_curve (no block counts, no prefix sums), == for integer
    levels, within the reference's bound otherwise."""
    n, partial = 0, 0
    for seed in range(24):
        rng = np.random.RandomState(31000 + seed)
        k, w = (256, 288, 320)[seed % 3], int(rng.randint(1, 24))
        nb, tail = int(rng.randint(1, 5)), int(rng.choice([0, 1, 31, 33]))
        S = nb * k + tail
        R = S + 40 if seed % 4 else S - 150
        r_lv, s_lv = [(I0, I0), (I1, I0), (I0, I1), (I1, F)][seed % 4]
        rb, sb = pw.two_offset_bits(rng, R, S, (int(rng.randint(-w + 1, w + 1)), int(rng.randint(-w + 1, w + 1))))
        ref = pw.Reference(rb, sb, r_lv, s_lv, k, -w + 1, w)
        offsets = rng.randint(-w + 1, w + 1, size=ref.B)
        f = int(rng.randint(0, ref.B))
        e = int(rng.randint(f + 1, ref.B + 1))
        got, shift_lo = rr.path_curve(ref, f, e, offsets)
        want = drm.brute_path_curve(rb, sb, r_lv, s_lv, k, w, f, e, offsets)
        assert shift_lo == -w + 1 - int(offsets[f:e].min()) and got.shape == want.shape
        if ref.exact:
            assert np.array_equal(got, want), (seed, got, want)
        else:
            assert np.all(np.abs(got - want) <= rr.tolerance(ref)) and rr.tolerance(ref) > 0
        n += 1
        partial += R < S
    assert n == 24 and partial >= 4


def test_piece_curve_equals_direct_counting():
    """The piece curve over ranges that reach past both ends of the overlap, one-lag ranges and ranges without overlap
    == cut_report_model.brute_curve."""
    n, empty = 0, 0
    for seed in range(24):
        rng = np.random.RandomState(32000 + seed)
        k = (256, 288, 320)[seed % 3]
        nb, tail = int(rng.randint(1, 5)), int(rng.choice([0, 1, 31, 33]))
        S = nb * k + tail
        R = int(rng.randint(200, 1500))
        lo, hi = [(-S - 5, -S + 30), (R - 20, R + 20), (-40, 40), (7, 7), (R + 3, R + 9), (-S - 9, -S - 2)][seed % 6]
        r_lv, s_lv = [(I0, I0), (I1, I0), (I0, I1), (I1, F)][seed % 4]
        rb, sb = pw.two_offset_bits(rng, R, S, (3, -8))
        ref = pw.Reference(rb, sb, r_lv, s_lv, k, lo, hi)
        a = int(rng.randint(0, ref.B))
        c = int(rng.randint(a + 1, ref.B + 1))
        got = ref.interval(a, c)
        want = crm.brute_curve(rb, sb, r_lv, s_lv, a * k, min(c * k, S), lo, hi)
        if ref.exact:
            assert np.array_equal(got, want), (seed, got, want)
        else:
            assert np.all(np.abs(got - want) <= rr.tolerance(ref))
        n += 1
        empty += not want.any()
    assert n == 24 and empty >= 6


def test_greedy_peaks_and_tables_by_hand():
    v = np.array([1.0, 5.0, 5.0, 2.0, 5.0, 0.0])
    assert rr.greedy_peaks(v, 8, 1) == [(5.0, 4), (5.0, 2), (5.0, 1), (2.0, 3), (1.0, 0), (0.0, 5)]
    assert rr.greedy_peaks(v, 8, 2) == [(5.0, 4), (5.0, 2), (1.0, 0)]
    assert rr.greedy_peaks(v, 2, 3) == [(5.0, 4), (5.0, 1)]
    assert rr.greedy_peaks(v, 8, 6) == [(5.0, 4)]
    table = rr.segment_table([3, 4, 4, 9, 9], [1, 0, 1, 1, 0], 256, 4 * 256 + 7)  # the flag of block 0 is ignored
    assert [(g["first_block"], g["end_block"], g["end_sample"]) for g in table] == [(0, 2, 512), (2, 3, 768), (3, 5, 1031)]
    assert [(g["first_offset"], g["last_offset"], g["min_offset"], g["max_offset"]) for g in table] == \
        [(3, 4, 3, 4), (4, 4, 4, 4), (9, 9, 9, 9)]
    pieces = rr.piece_table([3, 4, 4, 9, 9], 256, 4 * 256 + 7)
    assert [(g["first_block"], g["end_block"], g["offset"]) for g in pieces] == [(0, 1, 3), (1, 3, 4), (3, 5, 9)]


# ---- the models on the device test's groups --------------------------------------------------------------------------

def _segment_group(name, k, w, pairs, settings, first_call):
    """(problems, Facts, [(pair, setting index, block offsets, jump flags, reference records)]) of the drift report model
    on one group."""
    bad, facts, solves = [], rr.Facts(), []
    for i, pr in enumerate(pairs):
        ref = cases.reference(pr)
        counts = sm.block_counts(pr["rb"], pr["sb"], k, w)
        for si, setting in enumerate(settings):
            top_k, excl = rc.peak_args(first_call + si, 2 * w)
            (offs, _, jump, _), recs, _ = drm.report(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, w, *setting, top_k,
                                                     excl, n11_blocks=counts)
            want = rr.segment_records(ref, offs, jump, top_k, excl)
            probs = rr.compare(ref, want, recs, len(recs), top_k, "segment", facts, (name, i))
            if probs:
                bad.append((name, i, setting, probs[:3]))
            solves.append((i, si, offs, jump, want))
    return bad, facts, solves


@functools.lru_cache(maxsize=None)
def _window_group(gi):
    k, w, _, _ = WINDOW_GROUPS[gi]
    return _segment_group("window K=%d W=%d" % (k, w), k, w, cases.window_pairs(gi), rc.SEGMENT_SETTINGS,
                          gi * len(rc.SEGMENT_SETTINGS))


@functools.lru_cache(maxsize=None)
def _extra_window_group(name):
    k, w, pairs, settings = rc.extra_window_groups()[name]
    return _segment_group(name, k, w, pairs, settings, rc.EXTRA_WINDOW_NAMES.index(name) * 2 + 1)


def _piece_group(name, k, pairs, first_call):
    bad, facts = [], rr.Facts()
    n_full = max(pr["hi"] - pr["lo"] + 1 for pr in pairs)  # one exclusion distance per device call
    for i, pr in enumerate(pairs):
        ref = pw.Reference(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, pr["lo"], pr["hi"])
        for pi, p in enumerate(rc.PIECE_PENALTIES):
            top_k, excl = rc.peak_args(first_call + pi, n_full)
            offs = cm.solve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, pr["lo"], pr["hi"], p)[0]
            recs, _ = crm.report(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, pr["lo"], pr["hi"], offs, top_k, excl)
            want = rr.piece_records(ref, offs, top_k, excl)
            probs = rr.compare(ref, want, recs, len(recs), top_k, "piece", facts, (name, i))
            if probs:
                bad.append((name, i, p, probs[:3]))
    return bad, facts


@functools.lru_cache(maxsize=None)
def _range_group(gi):
    return _piece_group("range K=%d" % RANGE_GROUPS[gi][0], RANGE_GROUPS[gi][0], rc.range_pairs(gi), 2 * gi)


@functools.lru_cache(maxsize=None)
def _extra_range_group(name):
    k, pairs = rc.extra_range_groups()[name]
    return _piece_group("range " + name, k, pairs, 2 * rc.EXTRA_RANGE_NAMES.index(name) + 1)


def test_segment_report_model_equals_the_reference_on_every_window_group():
    bad = []
    for gi in range(len(WINDOW_GROUPS)):
        b, _, solves = _window_group(gi)
        assert len(solves) == len(WINDOW_GROUPS[gi][3]) * len(rc.SEGMENT_SETTINGS)  # every pair, every setting
        bad += b
    assert not bad, bad[:5]


def test_segment_report_model_equals_the_reference_on_the_added_groups():
    groups = rc.extra_window_groups()
    assert tuple(groups) == rc.EXTRA_WINDOW_NAMES
    bad = []
    for name in rc.EXTRA_WINDOW_NAMES:
        bad += _extra_window_group(name)[0]
    assert not bad, bad[:5]
    # each group holds what it was added for
    firsts = {g["first_block"] for _, _, _, _, want in _extra_window_group("long")[2] for g in want}
    assert 1024 in firsts and (1023 in firsts or 1025 in firsts), sorted(firsts)[-6:]
    for i, _, _, _, want in _extra_window_group("rounds")[2]:
        assert len(want) > 8 if i == 0 else len(want) == 1, (i, len(want))
    for i, _, _, _, want in _extra_window_group("wide")[2]:
        spread = [g for g in want if g["max_offset"] - g["min_offset"] >= rr.FLAT_CHUNK]
        assert spread, (i, [(g["min_offset"], g["max_offset"]) for g in want])
        if i == 1:  # the periodic pair: equal maxima in both chunks, and the largest such lag wins
            for g in spread:
                q = g["flat_curve"]
                assert q[:rr.FLAT_CHUNK].max() == q[rr.FLAT_CHUNK:].max() == g["flat_score"]
                assert g["flat_offset"] - g["min_offset"] >= rr.FLAT_CHUNK
    for _, _, _, _, want in _extra_window_group("single")[2]:
        assert [(g["n_lags"], len(g["peaks"]), g["flat"]) for g in want] == [(1, 1, True)]
    for name in ("edge288", "edge800"):
        assert _extra_window_group(name)[1].nan_inside >= 1, name


def test_piece_report_model_equals_the_reference_on_every_range_group():
    bad, facts = [], rr.Facts()
    for gi in range(len(RANGE_GROUPS)):
        b, f = _range_group(gi)
        bad += b
        facts.merge(f)
    for name in rc.EXTRA_RANGE_NAMES:
        b, f = _extra_range_group(name)
        bad += b
        facts.merge(f)
    assert not bad, bad[:5]
    assert facts.no_overlap >= 4 and _extra_range_group("rounds")[1].many == 2, facts.counts()
    assert facts.worst <= facts.worst_tol and facts.worst_tol > 0  # the F pair of the first group was compared


@functools.lru_cache(maxsize=None)
def _given_offsets():
    k, pr, offs = rc.given_offsets()
    ref = pw.Reference(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, pr["lo"], pr["hi"])
    recs, _ = crm.report(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, pr["lo"], pr["hi"], offs, 3, 50)
    facts = rr.Facts()
    return rr.compare(ref, rr.piece_records(ref, offs, 3, 50), recs, len(recs), 3, "piece", facts, "given"), facts


def test_given_offsets_beside_the_maximum_raise_own_not_peak():
    bad, facts = _given_offsets()
    assert not bad, bad[:5]
    assert facts.records == 12 and facts.own_not_peak >= 2, facts.counts()


def _refine_jumps():
    """{K: jumps} of the paths the device test refines: the drift model's on the refinement groups at the settings whose
    paths can hold jumps, and the long pair's."""
    out = {}
    for gi in rc.REFINE_WINDOW_GROUPS:
        k = WINDOW_GROUPS[gi][0]
        out[k] = out.get(k, 0) + sum(len(jrm.jumps_of(jump)) for _, si, _, jump, _ in _window_group(gi)[2]
                                      if si in rc.REFINE_SETTINGS)
    for _, si, _, jump, _ in _extra_window_group("long")[2]:
        if si == 0:
            out[256] = out.get(256, 0) + len(jrm.jumps_of(jump))
    return out


def test_the_case_table_is_not_vacuous():
    """The conditions of the device test, on the models' paths."""
    seg, piece = rr.Facts(), rr.Facts()
    for gi in range(len(WINDOW_GROUPS)):
        seg.merge(_window_group(gi)[1])
    for name in rc.EXTRA_WINDOW_NAMES:
        seg.merge(_extra_window_group(name)[1])
    for gi in range(len(RANGE_GROUPS)):
        piece.merge(_range_group(gi)[1])
    for name in rc.EXTRA_RANGE_NAMES:
        piece.merge(_extra_range_group(name)[1])
    piece.merge(_given_offsets()[1])
    jumps = _refine_jumps()
    print("segment report:", seg.counts(), "piece report:", piece.counts(), "jumps to refine:", jumps)
    assert rc.conditions_hold(seg, piece, jumps), (seg.counts(), piece.counts(), jumps)
    combos = {rc.peak_args(c, 10 ** 6) for c in range(len(WINDOW_GROUPS) * len(rc.SEGMENT_SETTINGS))}
    assert len(combos) == 9  # every top_k with every exclusion distance


# ---- the three planted mistakes --------------------------------------------------------------------------------------

def _scan_table(block_jump, chunk, keep_carry=True):
    """A restated copy of the device's segment numbering: the blocks are taken ``chunk`` at a time, a block's segment is
    the number of starts at or before it in its chunk, minus one, plus the starts of the earlier chunks (the carry).
    Returns [(first_block, end_block)] as the records would hold them."""
    B = len(block_jump)
    first, end, carry = {}, {}, 0
    for b0 in range(0, B, chunk):
        starts = [b == 0 or block_jump[b] != 0 for b in range(b0, min(b0 + chunk, B))]
        seen = 0
        for t, start in enumerate(starts):
            b = b0 + t
            seen += start
            idx = carry + seen - 1
            if start:
                first[idx] = b
            if b == B - 1 or block_jump[b + 1] != 0:
                end[idx] = b + 1
        if keep_carry:
            carry += seen
    return [(first.get(i), end.get(i)) for i in range(max(first) + 1)]


def test_dropping_the_carry_of_the_segment_numbering_is_caught():
    _, _, solves = _extra_window_group("long")
    _, _, _, jump, want = solves[0]
    table = [(g["first_block"], g["end_block"]) for g in want]
    assert _scan_table(list(jump), 1024) == table
    assert _scan_table(list(jump), 1024, keep_carry=False) != table
    assert _scan_table(list(jump), 4096, keep_carry=False) == table  # one chunk: the long pair is what catches it
