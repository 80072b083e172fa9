"""What the device computes AFTER a solve, against the independent report reference (tests/report_reference.py) and not
against the step-for-step report models: the drift solve's segment path report (k_drift_segments, k_drift_path_sums,
k_drift_segment_report), the per-piece report over a lag range (k_cut_piece_counts, k_cut_piece_report) and jump / break
refinement (k_drift_refine_jumps, k_refine_breaks and their cut kernels; these against their per-sample models) -- at the
shapes of tests/test_gpu_split_optimum.py and tests/drift_path_cases.py, which no report test reaches on the device: K
that are not powers of two and K = 32 768 (uint16 count rows, pieces of more than 512 subtitle words), tail blocks of 1
to 33 samples, W = 1 and 2W = 262 144, one-lag ranges, ranges without overlap and 282 999 lags; and at the groups of
tests/report_cases.py: more than 1024 blocks (the carry of the table kernels' chunk loop, jumps at blocks 1023, 1024 and
1025), more than eight segments or pieces (the rounds' reused row workspace, a slot past a pair's count beside a full
one), an offset spread of more than 1024 lags (the chunk loop of the flat maximum, with a tie across two chunks), a shift
set of one shift, and neighbour shifts outside the shift set at K = 288 and 800.

Every fp and int field of every record is compared; integer-level pairs as float64 bit patterns, NaN equal to NaN, mean
and std within 1e-12 * max(|mean|, std); the F-level pairs within the bound the reference derives.  The entry points
take one top_k and one exclusion distance per call, so these vary per (group, setting) over {1, 3, 8} x {1, 50, a value
>= n_lags}.  tests/test_report_reference_host.py holds the models to the same reference on the same lists on the CPU."""
import functools

import numpy as np
import pytest

import drift_path_cases as cases
import drift_path_reference as dpr
import drift_refine_model as jrm
import piecewise_reference as pw
import report_cases as rc
import report_reference as rr
import split_refine_model as brm
from test_gpu_split_optimum import RANGE_GROUPS, WINDOW_GROUPS, _device_pairs

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _path_problems(ref, setting, res, optimum):
    """The returned path holds together (its objective is the returned total, jumps move, unflagged steps stay within
    max_step); with ``optimum`` the total is also the maximum over all lag paths (the groups no aligner test runs)."""
    tol = dpr.tolerance(ref, *setting)
    path = [ref.lag_index(o) for o in res.block_offsets]
    got, bad = dpr.objective(ref.rows, path, [int(x) for x in res.block_jump], *setting)
    if not abs(got - float(res.total)) <= tol:
        bad.append(("path objective != total", got, float(res.total)))
    if optimum and not abs(dpr.optimum(ref.rows, *setting) - float(res.total)) <= tol:
        bad.append(("total", float(res.total), dpr.optimum(ref.rows, *setting)))
    return bad


def _split_identity_problems(recs, counts, split_recs, split_counts):
    """max_step = 0: a segment is a piece, and its record equals split_report_batch's."""
    bad = []
    if not np.array_equal(counts, split_counts):
        return [("piece counts", counts.tolist(), split_counts.tolist())]
    for p in range(len(counts)):
        a, b = recs[p, :counts[p]], split_recs[p, :counts[p]]
        live = np.arange(rr.MAX_PEAKS)[None, :] < a["n_peaks"][:, None]
        same = (all(np.array_equal(a[f], b[f]) for f in ("first_block", "end_block", "start_sample", "end_sample",
                                                           "n_lags", "n_peaks", "flags"))
                and all(np.array_equal(_bits(a[f]), _bits(b[f])) for f in ("own_score", "prev_score", "next_score",
                                                                           "mean", "std", "peak_score"))
                and np.array_equal((a["peak_shift"] + b["offset"][:, None])[live], b["peak_offset"][live])
                and all(np.array_equal(a[f], b["offset"]) for f in ("first_offset", "last_offset", "min_offset",
                                                                     "max_offset", "flat_offset"))
                and np.array_equal(_bits(a["flat_score"]), _bits(a["own_score"])))
        if not same:
            bad.append(("max_step = 0 differs from split_report_batch", p))
    return bad


def _segment_group(name, k, w, pif, pairs, settings, first_call, optimum):
    from ffsubsync_amd import drift_report as dr
    from ffsubsync_amd import split_align as sa
    from ffsubsync_amd import split_report as sr

    refs = [cases.reference(pr) for pr in pairs]
    db = _device_pairs(pairs)
    bad, facts, results, checked = [], rr.Facts(), [], 0
    for si, setting in enumerate(settings):
        top_k, excl = rc.peak_args(first_call + si, 2 * w)
        res, recs, counts = dr.drift_report_batch(db, w, k, *setting, top_k, excl, pairs_in_flight=pif, raw=True)
        assert len(res) == len(pairs) and recs.shape[0] == len(pairs)
        results.append(res)
        for i, ref in enumerate(refs):
            probs = _path_problems(ref, setting, res[i], optimum)
            if not probs:
                want = rr.segment_records(ref, res[i].block_offsets, res[i].block_jump, top_k, excl)
                probs = rr.compare(ref, want, recs[i], int(counts[i]), top_k, "segment", facts, (name, i))
            checked += 1
            if probs:
                bad.append((name, i, setting, (top_k, excl), probs[:3]))
        if setting[1] == 0:
            _, split_recs, split_counts = sr.split_report_batch(db, w, k, setting[0], top_k, excl, pairs_in_flight=pif,
                                                                raw=True)
            bad += [(name, setting) + p for p in _split_identity_problems(recs, counts, split_recs, split_counts)]
    dr.clear_plan_cache()
    sa.clear_plan_cache()  # split_report_batch solves on split_align's plan
    return dict(bad=bad, facts=facts, checked=checked, pairs=pairs, db=db, results=results, k=k, settings=settings)


@functools.lru_cache(maxsize=None)
def _window_group(gi):
    k, w, pif, _ = WINDOW_GROUPS[gi]
    return _segment_group("window K=%d W=%d" % (k, w), k, w, pif, cases.window_pairs(gi), rc.SEGMENT_SETTINGS,
                          gi * len(rc.SEGMENT_SETTINGS), False)


@functools.lru_cache(maxsize=None)
def _extra_window_group(name):
    k, w, pairs, settings = rc.extra_window_groups()[name]
    return _segment_group(name, k, w, None, pairs, settings, rc.EXTRA_WINDOW_NAMES.index(name) * 2 + 1, True)


@pytest.mark.parametrize("gi", range(len(WINDOW_GROUPS)))
def test_segment_report_equals_the_reference(gi):
    g = _window_group(gi)
    assert g["checked"] == len(WINDOW_GROUPS[gi][3]) * len(rc.SEGMENT_SETTINGS)  # every pair, every setting
    assert not g["bad"], g["bad"][:5]


@pytest.mark.parametrize("name", rc.EXTRA_WINDOW_NAMES)
def test_segment_report_equals_the_reference_on_the_added_groups(name):
    g = _extra_window_group(name)
    assert g["checked"] == len(g["pairs"]) * len(g["settings"])
    assert not g["bad"], g["bad"][:5]
    f = g["facts"]
    if name == "long":  # a segment starts at block 1024, another at 1023 or 1025
        firsts = {s.first_block for res in g["results"] for s in res[0].segments}
        assert 1024 in firsts and (1023 in firsts or 1025 in firsts) and f.first_1024 >= 1, sorted(firsts)[-6:]
    if name == "rounds":  # more than 8 segments beside a pair of one segment
        assert all(len(res[0].segments) > 8 and len(res[1].segments) == 1 for res in g["results"])
    if name == "wide":  # the flat maximum took more than one chunk; on the periodic pair the second chunk's lag wins
        assert all(max(r.block_offsets) - min(r.block_offsets) >= rr.FLAT_CHUNK for res in g["results"] for r in res)
        assert f.flat_second_chunk >= 1, f.counts()
    if name == "single":
        assert f.single_shift == f.records == len(g["settings"]), f.counts()
    if name.startswith("edge"):
        assert f.nan_inside >= 1, f.counts()


# ---- the piece report over a range -----------------------------------------------------------------------------------

def _piece_group(name, k, pif, pairs, first_call, optimum):
    from ffsubsync_amd import cut_report as cr

    refs = [pw.Reference(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, pr["lo"], pr["hi"]) for pr in pairs]
    ranges = [(pr["lo"], pr["hi"]) for pr in pairs]
    db = _device_pairs(pairs)
    bad, facts, checked = [], rr.Facts(), 0
    for pi, p in enumerate(rc.PIECE_PENALTIES):
        top_k, excl = rc.peak_args(first_call + pi, max(ref.L for ref in refs))
        res, recs, counts = cr.split_range_report_batch(db, ranges, k, p, top_k, excl, pairs_in_flight=pif, raw=True)
        assert len(res) == len(pairs) and recs.shape[0] == len(pairs)
        for i, ref in enumerate(refs):
            probs = pw.check_solution(ref, p, res[i].block_offsets, res[i].total, res[i].block_scores) if optimum else []
            if not probs:
                want = rr.piece_records(ref, res[i].block_offsets, top_k, excl)
                probs = rr.compare(ref, want, recs[i], int(counts[i]), top_k, "piece", facts, (name, i))
                empty = ref.lo > ref.R - 1 or ref.hi < -(ref.S - 1)  # no lag of the range overlaps
                if empty and not probs:
                    for rec in recs[i, :int(counts[i])]:
                        n = int(rec["n_peaks"])
                        if not (int(rec["flags"]) & rr.FLAT and float(rec["mean"]) == 0.0 and float(rec["std"]) == 0.0
                                and n >= 1 and not _bits(rec["peak_score"][:n]).any() and int(rec["n_lags"]) == ref.L):
                            probs.append(("a range without overlap", rec))
            checked += 1
            if probs:
                bad.append((name, i, p, (top_k, excl), probs[:3]))
    cr.clear_plan_cache()
    return dict(bad=bad, facts=facts, checked=checked, pairs=pairs)


@functools.lru_cache(maxsize=None)
def _range_group(gi):
    k, pif, _ = RANGE_GROUPS[gi]
    return _piece_group("range K=%d" % k, k, pif, rc.range_pairs(gi), 2 * gi, False)


@functools.lru_cache(maxsize=None)
def _extra_range_group(name):
    k, pairs = rc.extra_range_groups()[name]
    return _piece_group("range " + name, k, None, pairs, 2 * rc.EXTRA_RANGE_NAMES.index(name) + 1, True)


@pytest.mark.parametrize("gi", range(len(RANGE_GROUPS)))
def test_piece_report_over_a_range_equals_the_reference(gi):
    g = _range_group(gi)
    assert g["checked"] == len(RANGE_GROUPS[gi][2]) * len(rc.PIECE_PENALTIES)  # every pair (the F pair too), both P
    assert not g["bad"], g["bad"][:5]
    if gi in (0, 3):  # the groups with a range without overlap
        assert g["facts"].no_overlap >= 2, g["facts"].counts()


@pytest.mark.parametrize("name", rc.EXTRA_RANGE_NAMES)
def test_piece_report_over_a_range_equals_the_reference_on_the_added_pairs(name):
    g = _extra_range_group(name)
    assert g["checked"] == len(g["pairs"]) * len(rc.PIECE_PENALTIES)
    assert not g["bad"], g["bad"][:5]
    if name == "rounds":
        assert g["facts"].many == len(rc.PIECE_PENALTIES), g["facts"].counts()


@functools.lru_cache(maxsize=None)
def _given_offsets():
    from ffsubsync_amd import cut_report as cr

    k, pr, offs = rc.given_offsets()
    ref = pw.Reference(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, pr["lo"], pr["hi"])
    recs, counts = cr.report_batch(_device_pairs([pr]), [offs], [(pr["lo"], pr["hi"])], k, 3, 50)
    cr.clear_plan_cache()
    facts = rr.Facts()
    return rr.compare(ref, rr.piece_records(ref, offs, 3, 50), recs[0], int(counts[0]), 3, "piece", facts, "given"), facts


def test_given_offsets_beside_the_maximum_raise_own_not_peak():
    bad, facts = _given_offsets()
    assert not bad, bad[:5]
    assert facts.records == 12 and facts.own_not_peak >= 2, facts.counts()


# ---- refinement at these shapes, against the per-sample models, bit for bit ------------------------------------------

def _same_records(got, want):
    return got.shape == want.shape and all(got[f].tobytes() == want[f].tobytes() for f in want.dtype.names)


def _refine_problems(name, db, pairs, results, k):
    """refine_jumps_batch of ``results`` at every radius and beta against drift_refine_model.refine; returns (problems,
    jumps refined)."""
    from ffsubsync_amd import drift_refine as jr

    bad = []
    n_jumps = sum(len(jrm.jumps_of(r.block_jump)) for r in results)
    if not n_jumps:
        return bad, 0
    for radius in rc.REFINE_RADII:
        for beta in rc.REFINE_BETAS:
            recs, counts = jr.refine_jumps_batch(db, results, k, radius, beta, raw=True)
            for i, (pr, r) in enumerate(zip(pairs, results)):
                want = jrm.refine(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], r.block_offsets, r.block_jump, k, radius,
                                  beta)
                n = int(counts[i])
                if n != len(want) or not _same_records(recs[i, :n], want) or recs[i, n:].tobytes().strip(b"\0"):
                    bad.append((name, i, radius, beta, n, len(want)))
    return bad, n_jumps


@functools.lru_cache(maxsize=None)
def _refined_window_group(gi):
    g = _window_group(gi)
    bad, n_jumps = [], 0
    for si in rc.REFINE_SETTINGS:
        b, n = _refine_problems("window group %d setting %d" % (gi, si), g["db"], g["pairs"], g["results"][si], g["k"])
        bad += b
        n_jumps += n
    return bad, n_jumps


@pytest.mark.parametrize("gi", rc.REFINE_WINDOW_GROUPS)
def test_jump_refinement_at_the_hostile_block_lengths_equals_the_model(gi):
    bad, _ = _refined_window_group(gi)
    assert not bad, bad[:5]


@functools.lru_cache(maxsize=None)
def _refined_long_pair():
    from ffsubsync_amd import split_refine as br

    g = _extra_window_group("long")
    bad, n_jumps = _refine_problems("long", g["db"], g["pairs"], g["results"][0], g["k"])
    blocks = jrm.jumps_of(g["results"][0][0].block_jump)
    # the break refinement's table kernel shares the chunk loop: the max_step = 0 path of the same pair
    pr, res = g["pairs"][0], g["results"][1][0]
    for radius, beta in ((300, 0.25), (131072, None)):
        recs, counts = br.refine_breaks_batch(g["db"], [res], g["k"], radius, beta, raw=True)
        want = brm.refine(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], res.block_offsets, g["k"], radius, beta)
        n = int(counts[0])
        if n != len(want) or not _same_records(recs[0, :n], want) or recs[0, n:].tobytes().strip(b"\0"):
            bad.append(("long: breaks", radius, beta, n, len(want)))
        blocks = blocks + [int(b) for b in want["block"]]
    return bad, n_jumps, blocks


def test_refinement_past_1024_blocks_equals_the_models():
    """Jumps and breaks at blocks 1023 .. 1026: the carry of both table kernels' 1024-block chunk loop."""
    bad, n_jumps, blocks = _refined_long_pair()
    assert not bad, bad[:5]
    assert 1024 in blocks and (1023 in blocks or 1025 in blocks) and min(blocks) < 1023 and n_jumps >= 4, blocks


def test_refinement_of_hand_made_flags_equals_the_model():
    """Flags where the offset does not change and in two adjacent blocks: windows clipped at the midpoints."""
    from ffsubsync_amd import _native
    from ffsubsync_amd import drift_refine as jr
    from ffsubsync_amd.drift_align import DriftResult

    pr, offs, jump = rc.flagged_pair()
    k = pr["k"]
    res = DriftResult([], 0.0, offs, np.zeros(offs.size), jump)
    db = _device_pairs([pr])
    for radius, beta in ((300, 0.25), (1, None), (131072, 64.0)):
        recs, counts = jr.refine_jumps_batch(db, [res], k, radius, beta, raw=True)
        want = jrm.refine(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], offs, jump, k, radius, beta)
        n = int(counts[0])
        assert n == len(want) == 3 and _same_records(recs[0, :n], want), (radius, beta, recs[0, :n], want)
        assert not recs[0, n:].tobytes().strip(b"\0")
        got = recs[0, :n]
        assert got["block"].tolist() == [2, 4, 5] and int(got["offset_prev"][0]) == int(got["offset_next"][0])
        if radius > k // 2:  # the two adjacent jumps share a midpoint K / 2 from each cut
            assert int(got["hi"][1] - got["cut"][1]) == int(got["cut"][2] - got["lo"][2]) == k // 2
            assert all(int(f) & _native.REFINE_CLIPPED for f in got["flags"][1:])


# ---- the table was not vacuous on the device ---------------------------------------------------------------------------

def test_the_comparison_covered_what_the_reports_have_to_get_right():
    """Counted on the device's records that passed the comparison (a group not run yet in this process runs here)."""
    seg, piece, bad = rr.Facts(), rr.Facts(), []
    for g in [_window_group(gi) for gi in range(len(WINDOW_GROUPS))] + \
            [_extra_window_group(name) for name in rc.EXTRA_WINDOW_NAMES]:
        seg.merge(g["facts"])
        bad += g["bad"]
    for g in [_range_group(gi) for gi in range(len(RANGE_GROUPS))] + \
            [_extra_range_group(name) for name in rc.EXTRA_RANGE_NAMES]:
        piece.merge(g["facts"])
        bad += g["bad"]
    piece.merge(_given_offsets()[1])
    jumps = {}
    for gi in rc.REFINE_WINDOW_GROUPS:
        k = WINDOW_GROUPS[gi][0]
        jumps[k] = jumps.get(k, 0) + _refined_window_group(gi)[1]
    jumps[256] = _refined_long_pair()[1]
    print("segment report on the device:", seg.counts(), "piece report:", piece.counts(), "jumps refined:", jumps)
    print("F-level pairs: largest |score - reference| %.3g (segments, bound %.3g), %.3g (pieces, bound %.3g)"
          % (seg.worst, seg.worst_tol, piece.worst, piece.worst_tol))
    assert not bad, bad[:5]
    assert rc.conditions_hold(seg, piece, jumps), (seg.counts(), piece.counts(), jumps)
    assert seg.worst <= seg.worst_tol and piece.worst <= piece.worst_tol and seg.worst_tol > 0 and piece.worst_tol > 0
