"""The segment path report over a lag range on the device (k_range_path_counts, k_range_path_scores,
k_range_segment_report; ffsubsync_amd.drift_range_report) against the independent report reference
(tests/report_reference.py) at the hostile shapes of tests/test_gpu_split_optimum.py's range groups and the groups of
tests/drift_range_report_cases.py; byte for byte against the windowed segment report at [-W+1, W], the piece report
over a range at max_step = 0 and drift_align_range_batch's own outputs; on given paths; refused calls; the plan's
workspace; and under the hostile input layouts of tests/layout_cases.py.  tests/test_drift_range_report_host.py holds
the numpy model to the same reference on the same lists and shows that the coverage conditions asserted here are
reachable."""
import functools

import numpy as np
import pytest

import drift_path_cases as cases
import drift_range_report_cases as dc
import layout_cases as lc
import piecewise_reference as pw
import report_cases as rc
import report_reference as rr
from test_gpu_report_optimum import _path_problems, _split_identity_problems
from test_gpu_split_optimum import RANGE_GROUPS, WINDOW_GROUPS, _device_pairs

pytestmark = pytest.mark.gpu


def _reference(pr, k):
    return pw.Reference(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, pr["lo"], pr["hi"])


def _result_bytes(res):
    return [(np.asarray(r.block_offsets).tobytes(), np.asarray(r.block_scores).tobytes(),
             np.asarray(r.block_jump).tobytes(), np.float64(r.total).tobytes()) for r in res]


def _group(name, k, pif, pairs, settings, first_call, optimum):
    from ffsubsync_amd import cut_report as cr
    from ffsubsync_amd import drift_range as dg
    from ffsubsync_amd import drift_range_report as drr

    refs = [_reference(pr, k) for pr in pairs]
    ranges = [(pr["lo"], pr["hi"]) for pr in pairs]
    db = _device_pairs(pairs)
    bad, facts, checked, all_recs = [], rr.Facts(), 0, []
    for si, setting in enumerate(settings):
        top_k, excl = rc.peak_args(first_call + si, max(ref.L for ref in refs))
        res, recs, counts = drr.drift_range_report_batch(db, ranges, k, *setting, top_k, excl, pairs_in_flight=pif, raw=True)
        assert len(res) == len(pairs) and recs.shape[0] == len(pairs)
        all_recs.append((recs, counts, top_k, excl))
        for i, ref in enumerate(refs):
            probs = _path_problems(ref, setting, res[i], optimum)
            if not probs:
                want = rr.segment_records(ref, res[i].block_offsets, res[i].block_jump, top_k, excl)
                probs = rr.compare(ref, want, recs[i], int(counts[i]), top_k, "segment", facts, (name, i))
                empty = ref.lo > ref.R - 1 or ref.hi < -(ref.S - 1)  # no lag of the range overlaps
                if empty and not probs:
                    for rec in recs[i, :int(counts[i])]:
                        spread = int(rec["max_offset"] - rec["min_offset"])
                        if not (int(rec["flags"]) & rr.FLAT and float(rec["mean"]) == 0.0 and float(rec["std"]) == 0.0
                                and int(rec["n_lags"]) == ref.L - spread):
                            probs.append(("a range without overlap", rec))
            checked += 1
            if probs:
                bad.append((name, i, setting, (top_k, excl), probs[:3]))
        # (c) the drift outputs beside the report are drift_align_range_batch's
        alone = dg.drift_align_range_batch(db, ranges, k, *setting, pairs_in_flight=pif)
        if _result_bytes(alone) != _result_bytes(res):
            bad.append((name, setting, "the drift outputs differ from drift_align_range_batch's"))
        # (b) max_step = 0: a segment is a piece, and its record equals split_range_report_batch's
        if setting[1] == 0:
            _, split_recs, split_counts = cr.split_range_report_batch(db, ranges, k, setting[0], top_k, excl,
                                                                      pairs_in_flight=pif, raw=True)
            bad += [(name, setting) + p for p in _split_identity_problems(recs, counts, split_recs, split_counts)]
    drr.clear_plan_cache()
    dg.clear_plan_cache()
    cr.clear_plan_cache()
    return dict(bad=bad, facts=facts, checked=checked, pairs=pairs, settings=settings, db=db, ranges=ranges, k=k,
                recs=all_recs)


@functools.lru_cache(maxsize=None)
def _range_group(gi):
    k, pif, _ = RANGE_GROUPS[gi]
    return _group("range K=%d" % k, k, pif, rc.range_pairs(gi), rc.SEGMENT_SETTINGS, gi * len(rc.SEGMENT_SETTINGS), False)


@functools.lru_cache(maxsize=None)
def _extra_group(name):
    k, pairs, settings = dc.extra_groups()[name]
    return _group(name, k, None, pairs, settings, dc.EXTRA_NAMES.index(name) * 2 + 1, True)


# ---- 1, 2: against the independent reference ---------------------------------------------------------------------------

@pytest.mark.parametrize("gi", range(len(RANGE_GROUPS)))
def test_report_equals_the_reference_on_the_range_groups(gi):
    g = _range_group(gi)
    assert g["checked"] == len(RANGE_GROUPS[gi][2]) * len(rc.SEGMENT_SETTINGS)  # every pair (the F pair too), every setting
    assert not g["bad"], g["bad"][:5]
    if gi in (0, 3):  # the groups with one-lag ranges; group 0 also holds the range without overlap
        assert g["facts"].single_shift >= 1, g["facts"].counts()
    if gi == 0:
        assert g["facts"].no_overlap >= 2, g["facts"].counts()


@pytest.mark.parametrize("name", dc.EXTRA_NAMES)
def test_report_equals_the_reference_on_the_added_groups(name):
    g = _extra_group(name)
    assert g["checked"] == len(g["pairs"]) * len(g["settings"])
    assert not g["bad"], g["bad"][:5]
    f = g["facts"]
    if name == "rounds":  # more than 8 segments beside a pair of one segment
        assert f.many == len(g["settings"]), f.counts()
        assert all(int(counts[0]) > 8 and int(counts[1]) == 1 for _, counts, _, _ in g["recs"])
    if name == "long":
        assert f.first_1024 >= 1, f.counts()
    if name == "wide":  # a step every block over a spread of at least 1024 lags
        assert all(int(r["max_offset"] - r["min_offset"]) >= rr.FLAT_CHUNK for recs, _, _, _ in g["recs"] for r in recs[:, 0])
        assert f.flat_second_chunk >= 1 and f.stepping >= 2, f.counts()
    if name == "single":
        assert f.single_shift == f.records == len(g["settings"]), f.counts()
    if name.startswith("edge"):
        assert f.nan_inside >= 1, f.counts()


def test_the_comparison_covered_what_the_report_has_to_get_right():
    facts, bad = rr.Facts(), []
    for g in [_range_group(gi) for gi in range(len(RANGE_GROUPS))] + [_extra_group(name) for name in dc.EXTRA_NAMES]:
        facts.merge(g["facts"])
        bad += g["bad"]
    print("segment report over a range on the device:", facts.counts())
    print("F-level pairs: largest |score - reference| %.3g (bound %.3g)" % (facts.worst, facts.worst_tol))
    assert not bad, bad[:5]
    assert dc.conditions_hold(facts), facts.counts()
    assert facts.worst <= facts.worst_tol and facts.worst_tol > 0


# ---- 3a: the windowed report, byte for byte ----------------------------------------------------------------------------

@pytest.mark.parametrize("gi", range(len(WINDOW_GROUPS)))
def test_symmetric_windows_equal_the_windowed_report(gi):
    """The path report of drift_align_batch's path at [-W+1, W] is ffs_align_drift_report_batch's, F pairs included."""
    from ffsubsync_amd import drift_range_report as drr
    from ffsubsync_amd import drift_report as dr

    k, w, pif, _ = WINDOW_GROUPS[gi]
    pairs = cases.window_pairs(gi)
    db = _device_pairs(pairs)
    for si, setting in enumerate(rc.SEGMENT_SETTINGS):
        top_k, excl = rc.peak_args(gi + si, 2 * w)
        res, want, want_counts = dr.drift_report_batch(db, w, k, *setting, top_k, excl, pairs_in_flight=pif, raw=True)
        got, counts = drr.drift_range_path_report_batch(db, res, (-w + 1, w), k, top_k, excl, pairs_in_flight=pif, raw=True)
        assert np.array_equal(counts, want_counts), (gi, setting)
        assert got.tobytes() == want.tobytes(), (gi, setting, [i for i in range(len(pairs))
                                                               if got[i].tobytes() != want[i].tobytes()])
    dr.clear_plan_cache()
    drr.clear_plan_cache()


# ---- 4: given paths ----------------------------------------------------------------------------------------------------

def test_hand_made_flags_equal_the_reference():
    """A jump flagged where the offset does not change, and two adjacent flagged blocks."""
    from ffsubsync_amd import drift_range_report as drr

    pr, offs, jump = rc.flagged_pair()
    ref = _reference(pr, pr["k"])
    recs, counts = drr.drift_range_path_report_batch(_device_pairs([pr]), ([offs], [jump]), [(pr["lo"], pr["hi"])], pr["k"],
                                                     3, 50, raw=True)
    drr.clear_plan_cache()
    facts = rr.Facts()
    bad = rr.compare(ref, rr.segment_records(ref, offs, jump, 3, 50), recs[0], int(counts[0]), 3, "segment", facts, "flags")
    assert not bad, bad[:5]
    assert int(counts[0]) == 4 and recs[0]["first_block"][:4].tolist() == [0, 2, 4, 5] and facts.stepping == 2


def test_given_offsets_beside_the_maximum_raise_own_not_peak():
    from ffsubsync_amd import drift_range_report as drr

    k, pr, offs = rc.given_offsets()
    jump = np.concatenate([[0], np.diff(offs) != 0]).astype(np.uint8)
    ref = _reference(pr, k)
    segs = drr.drift_range_path_report_batch(_device_pairs([pr]), ([offs], [jump]), [(pr["lo"], pr["hi"])], k, 3, 50)
    recs, counts = drr.drift_range_path_report_batch(_device_pairs([pr]), ([offs], [jump]), [(pr["lo"], pr["hi"])], k, 3, 50,
                                                     raw=True)
    drr.clear_plan_cache()
    facts = rr.Facts()
    bad = rr.compare(ref, rr.segment_records(ref, offs, jump, 3, 50), recs[0], int(counts[0]), 3, "segment", facts, "given")
    assert not bad, bad[:5]
    assert facts.records == 12 and facts.own_not_peak >= 2, facts.counts()
    assert len(segs[0]) == 12 and sum(not q.own_is_peak for q in segs[0]) == facts.own_not_peak


# ---- 5, 6: refusals and the plan ---------------------------------------------------------------------------------------

def _plan_problem():
    pairs = rc.range_pairs(1)  # K = 288: a range of 3501 lags and a full range
    k = RANGE_GROUPS[1][0]
    db = _device_pairs(pairs)
    lo = np.array([pr["lo"] for pr in pairs], np.int64)
    hi = np.array([pr["hi"] for pr in pairs], np.int64)
    sub_len = db.lens[:, 1].astype(np.int64)
    max_b = int(((sub_len + k - 1) // k).max())
    return pairs, k, db, lo, hi, max_b


def test_refused_calls_leave_the_outputs_untouched():
    import torch

    from ffsubsync_amd import _native

    pairs, k, db, lo, hi, max_b = _plan_problem()
    n, dev = len(pairs), db.data.device
    plan = _native.DriftRangePlan(n, max_b, int((hi - lo + 1).max()), int(db.lens.max()), 2)
    try:
        offs, scores, totals = (torch.empty(n * max_b, dtype=torch.int32, device=dev),
                                torch.empty(n * max_b, dtype=torch.float64, device=dev),
                                torch.empty(n, dtype=torch.float64, device=dev))
        jumps = torch.empty(n * max_b, dtype=torch.uint8, device=dev)
        arrays = db.pair_arrays()
        plan.align(*arrays, k, lo, hi, 60.0, 2, 1.0, offs, scores, jumps, totals)
        rep = torch.full((n * max_b * _native.SEGMENT_REPORT_BYTES + 8,), 0xAB, dtype=torch.uint8, device=dev)
        cnt = torch.full((n,), -9, dtype=torch.int32, device=dev)
        outside = offs.clone()
        outside[max_b] = int(hi[1]) + 1  # the second pair's first block
        before = [t.clone() for t in (offs, jumps, rep, cnt, outside)]
        ws0 = plan.workspace_bytes
        good = dict(offs=offs, top_k=3, e=50, rep=rep[:-8], k=k, sub_len=arrays[5])
        for case in (dict(offs=outside), dict(top_k=0), dict(top_k=9), dict(e=0), dict(rep=rep[4:-4]), dict(k=300),
                     dict(sub_len=np.zeros(n, np.int64))):
            a = dict(good)
            a.update(case)
            with pytest.raises(_native.NativeError) as ei:
                plan.report(*arrays[:5], a["sub_len"], *arrays[6:], a["k"], lo, hi, a["offs"], jumps, a["top_k"], a["e"],
                            a["rep"], cnt)
            assert ei.value.code == (-5 if "sub_len" in case else -1), case  # FFS_E_EMPTY / FFS_E_INVALID
        torch.cuda.synchronize()
        for a, b in zip(before, (offs, jumps, rep, cnt, outside)):
            assert torch.equal(a, b)
        assert plan.workspace_bytes == ws0  # nothing was allocated by a refused call
    finally:
        plan.close()


def test_the_plan_grows_once_and_the_solve_is_unchanged():
    import torch

    from ffsubsync_amd import _native

    pairs, k, db, lo, hi, max_b = _plan_problem()
    n, dev = len(pairs), db.data.device
    plan = _native.DriftRangePlan(1, max_b, int((hi - lo + 1).max()), int(db.lens.max()), 2)  # two sub-batches
    try:
        arrays = db.pair_arrays()

        def solve():
            outs = (torch.zeros(n * max_b, dtype=torch.int32, device=dev), torch.zeros(n * max_b, dtype=torch.float64, device=dev),
                    torch.zeros(n * max_b, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.float64, device=dev))
            plan.align(*arrays, k, lo, hi, 60.0, 2, 1.0, *outs)
            torch.cuda.synchronize()
            return outs

        ws0 = plan.workspace_bytes
        first = solve()
        assert plan.workspace_bytes == ws0  # a plan that never reports keeps its size
        rep = torch.zeros(n * max_b * _native.SEGMENT_REPORT_BYTES // 8, dtype=torch.int64, device=dev)
        cnt = torch.zeros(n, dtype=torch.int32, device=dev)
        plan.report(*arrays, k, lo, hi, first[0], first[2], 3, 50, rep, cnt)
        torch.cuda.synchronize()
        assert plan.workspace_bytes == ws0 + plan.report_bytes()  # the documented amount
        again = rep.clone()
        plan.report(*arrays, k, lo, hi, first[0], first[2], 3, 50, rep, cnt)
        torch.cuda.synchronize()
        assert plan.workspace_bytes == ws0 + plan.report_bytes() and torch.equal(rep, again)
        second = solve()
        assert all(torch.equal(a, b) for a, b in zip(first, second))  # identical bytes after a report call
    finally:
        plan.close()


def test_sub_batches_give_the_same_records():
    from ffsubsync_amd import drift_range_report as drr

    k, pairs, settings = dc.extra_groups()["rounds"]
    pairs = pairs + rc.range_pairs(0)[:3]  # K = 256 as well: five pairs, the first with more than 8 segments
    ranges = [(pr["lo"], pr["hi"]) for pr in pairs]
    db = _device_pairs(pairs)
    a = drr.drift_range_report_batch(db, ranges, k, *settings[0], 3, 50, raw=True)
    drr.clear_plan_cache()
    b = drr.drift_range_report_batch(db, ranges, k, *settings[0], 3, 50, pairs_in_flight=1, raw=True)
    drr.clear_plan_cache()
    assert _result_bytes(a[0]) == _result_bytes(b[0])
    assert a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2]) and int(a[2][0]) > 8


# ---- 7: hostile layouts ------------------------------------------------------------------------------------------------

def _layout_pairs():
    """Seven K = 256 pairs whose lengths cover every residue ``layout_cases.length_gaps`` names (the last subtitle keeps
    19 samples): four of range group 0, the pair of more than 8 segments and the one-segment pair beside it."""
    picked = rc.range_pairs(0)[:4] + list(dc.extra_groups()["rounds"][1])
    short = rc.range_pairs(0)[0]
    picked.append(dict(short, sb=short["sb"][:300], lo=-10, hi=40))
    lens = lc.cover_lengths([n for pr in picked for n in (pr["rb"].size, pr["sb"].size)])
    return [dict(pr, rb=pr["rb"][:lens[2 * i]], sb=pr["sb"][:lens[2 * i + 1]]) for i, pr in enumerate(picked)]


@pytest.mark.parametrize("layout", lc.LAYOUTS)
def test_hostile_layouts(layout):
    import torch

    from ffsubsync_amd import _native

    k, pairs = 256, _layout_pairs()
    n = len(pairs)
    img = lc.build([v for pr in pairs for v in (pr["rb"], pr["sb"])], lc.U1, layout).upload()
    db = img.device_batch((n, 2), [[pr["r_lv"][0], pr["s_lv"][0]] for pr in pairs],
                          [[pr["r_lv"][1], pr["s_lv"][1]] for pr in pairs], lc.U1)
    lo = np.array([pr["lo"] for pr in pairs], np.int64)
    hi = np.array([pr["hi"] for pr in pairs], np.int64)
    max_b = int(max(-(-pr["sb"].size // k) for pr in pairs))
    hostile = layout != "clean"
    res4, res8 = (4, 12, 20, 60), (8, 24, 56, 40)
    can = lc.Canaries([n * max_b * 4, n * max_b * 8, n * max_b, n * 8, n * max_b * _native.SEGMENT_REPORT_BYTES, n * 4],
                      [res4[1], res8[0], 1, res8[1], res8[2], res4[0]] if hostile else [0] * 6)
    offs, scores = can.tensor(0, torch.int32), can.tensor(1, torch.float64)
    jumps, totals = can.tensor(2, torch.uint8), can.tensor(3, torch.float64)
    rep, cnt = can.tensor(4), can.tensor(5, torch.int32)
    plan = _native.DriftRangePlan(4, max_b, int((hi - lo + 1).max()), int(db.lens.max()), 2)  # two sub-batches
    try:
        arrays = db.pair_arrays()
        plan.align(*arrays, k, lo, hi, 3.0, 2, 1.0, offs, scores, jumps, totals)
        plan.report(*arrays, k, lo, hi, offs, jumps, 3, 50, rep, cnt)
        torch.cuda.synchronize()
    finally:
        plan.close()
    img.assert_inputs_untouched("drift range report")
    can.assert_canaries_intact("drift range report [%s]" % layout)
    recs = rep.cpu().numpy().view(_native.SEGMENT_REPORT_DTYPE).reshape(n, max_b)
    counts = cnt.cpu().numpy()
    offs_h, jumps_h = offs.cpu().numpy().reshape(n, max_b), jumps.cpu().numpy().reshape(n, max_b)
    bad = []
    for i, pr in enumerate(pairs):
        ref = _reference(pr, k)
        o, j = offs_h[i, :ref.B], jumps_h[i, :ref.B]
        want = rr.segment_records(ref, o, j, 3, 50)
        probs = rr.compare(ref, want, recs[i], int(counts[i]), 3, "segment")
        if probs:
            bad.append((layout, i, probs[:3]))
    assert not bad, bad[:3]
    assert int(counts.max()) > 8


# ---- 8: verdicts -------------------------------------------------------------------------------------------------------

VERDICT_CLASSES = ("clean", "drift", "steep", "wrong")  # four problems of each (one hour, full range)


def _calibration():
    import json
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    doc = json.load(open(os.path.join(root, "profiles", "drift_range_report_calibration.json")))
    return {(r["cls"], r["seed"]): r for r in doc["problems"]}, doc["defaults"]


def test_verdicts_are_the_calibration_s():
    """checked_cut_drift_sync decides what profiles/drift_range_report_calibration.json records for the problem (the
    device is bit-identical to the model that wrote it: none is left out); wrong pairs keep their cue times; every
    problem decided "drift" has cut_drift_sync's cue times."""
    from ffsubsync_amd import cut_align as ca
    from ffsubsync_amd import cut_report as cr
    from ffsubsync_amd import drift_range as dg
    from ffsubsync_amd import drift_range_report as drr
    from workloads import cut_drift

    recorded, defaults = _calibration()
    assert defaults == dict(min_segment_psr=drr.DEFAULT_MIN_SEGMENT_PSR, min_gain=drr.DEFAULT_MIN_GAIN,
                            min_drift_gain=drr.DEFAULT_MIN_DRIFT_GAIN)  # (profiles/... --rescore after a change)
    keys, items = [], []
    for cls in VERDICT_CLASSES:
        for seed in sorted(s for c, s in recorded if c == cls)[:4]:
            if cls == "wrong":
                track, ref = cut_drift.make_problem(seed).track, cut_drift.make_problem(seed + 1).ref
            else:
                p = cut_drift.make_problem(seed, clean=cls == "clean", fixed=cls == "steep")
                track, ref = p.track, p.ref
            keys.append((cls, seed))
            items.append((ref.astype(float), track))
    assert len(items) == 16
    got = drr.checked_cut_drift_sync(items)
    plain = dg.cut_drift_sync(items)
    for m in (drr, dg, cr, ca):
        m.clear_plan_cache()
    n_drift = 0
    for key, (_, (start_us, end_us, _meta)), g, c in zip(keys, items, got, plain):
        want = recorded[key]
        # (the device rasterises the track itself, the calibration as workloads/drift.py does: a cue edge may differ by
        # a sample, so the figures are printed and the DECISION is what is held)
        print(key, g.decision, "psr", [round(q.psr, 3) for q in g.segment_quality], "recorded",
              [round(s["psr"], 3) for s in want["segments"]])
        assert g.ratio_index == want["ratio_index"], key
        assert (g.decision == "drift") == bool(want["drift"]), (key, g.decision, g.reasons, want["reasons"])
        assert (g.fallback is None) == (g.decision == "drift"), key
        if g.decision == "drift":
            n_drift += 1
            assert g.reasons == [] and np.array_equal(g.cue_start_us, c.cue_start_us), key
            assert np.array_equal(g.cue_end_us, c.cue_end_us) and np.array_equal(g.cue_segment, c.cue_segment), key
        if key[0] == "wrong":
            assert g.decision == "untrusted", (key, g.decision)
            assert np.array_equal(g.cue_start_us, np.asarray(start_us, np.int64)), key
            assert np.array_equal(g.cue_end_us, np.asarray(end_us, np.int64)), key
    assert n_drift >= 4  # the defaults let real drift solves through
