"""Sampled alignment on the device (csrc/ffs_sampled.h through ``_native.ProgPlan``) against the numpy model
tests/sampled_model.py after EVERY append: peaks bit for bit, mean and std at tests/test_gpu_progressive.py's tolerance.
Shapes from tests/sampled_cases.py; the record helpers are tests/test_gpu_progressive.py's."""
import numpy as np
import pytest

import progressive_cases as pc
import progressive_model as pm
import quality_model as qm
import sampled_cases as sc
import sampled_model as sm
from test_gpu_progressive import GUARD, Cands, Outputs, _bits, _check, _dev, _open, _words

pytestmark = pytest.mark.gpu


def _open_sampled(plan, slots, cases, cands, rows=None):
    mc = plan.max_cand
    rows = range(len(cases)) if rows is None else rows
    n = len(slots)
    ptr, length = np.zeros((n, mc), np.uint64), np.ones((n, mc), np.int64)
    lo, hi = np.zeros((n, mc)), np.ones((n, mc))
    for i, row in enumerate(rows):
        for c, (s, lv) in enumerate(cases[row]["cands"]):
            ptr[i, c], length[i, c], lo[i, c], hi[i, c] = cands.ptr(row, c), len(s), lv[0], lv[1]
    sel = [cases[r] for r in rows]
    plan.open_sampled(slots, [len(k["cands"]) for k in sel], ptr, length, lo, hi, [k["ref_levels"][0] for k in sel],
                      [k["ref_levels"][1] for k in sel], [k["W"] for k in sel], [k["T"] for k in sel])


def _plan_for(cases, n_slots=None, max_lags=None):
    from ffsubsync_amd import _native

    return _native.ProgPlan(n_slots or len(cases), max(len(k["cands"]) for k in cases),
                            max_lags or 2 * max(k["W"] for k in cases), max(k["T"] for k in cases),
                            max(len(s) for k in cases for s, _ in k["cands"]))


def _reference_bits(plan, slot, T):
    """The plan's reference bits of a slot as a bool array of T samples (after a synchronisation)."""
    import torch

    from ffsubsync_amd.progressive import _DeviceWords

    ptr, n = plan.reference(slot)
    assert n == T
    torch.cuda.synchronize()
    words = torch.as_tensor(_DeviceWords(ptr, (T + 31) // 32), device="cuda").cpu().numpy().view(np.uint32)
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:T].astype(bool), words


def _run_script(case, script, poison=True, max_lags=None):
    """One sampled slot through its appends, checked against the model after each; returns (raw bytes after the last,
    the model slot).  ``max_lags``: the plan's, where it is not the case's own 2W."""
    n_cand = len(case["cands"])
    plan = _plan_for([case], max_lags=max_lags)
    cands = Cands([case])
    slot = sm.Slot(case["cands"], case["ref_levels"], case["W"], case["T"])
    last = None
    try:
        assert plan.sampled_bytes() == 0
        _open_sampled(plan, [0], [case], cands)
        assert plan.sampled_bytes() >= 12 * 2 * case["W"] * n_cand
        if poison:
            cands.data.fill_(-1)  # queued right behind open: the plan works on its own copy
        for a, n, fb in script:
            chunk = case["ref"][a:a + n]
            words = _dev(_words(chunk, fb))  # every bit around the handed ones is set
            out = Outputs(1, n_cand)
            plan.append_at([0], [words.data_ptr()], [fb], [a], [n], case["top_k"], case["e"], *out.views())
            if poison:
                words.fill_(0x55555555)  # queued right behind the append
            recs, states = out.read()
            reps, mstate = slot.append_at(a, chunk, case["top_k"], case["e"])
            _check(recs[0], states[0], reps, mstate, n_cand, case["top_k"], ("a", a, "n", n))
            assert [tuple(x) for x in plan.known(0)] == slot.intervals, (a, n)
            last = recs.tobytes() + states.tobytes()
        bits, words = _reference_bits(plan, 0, case["T"])
        assert (bits == (slot.ref & slot.known)).all(), "the reference holds the known bits and zeros elsewhere"
        if case["T"] % 32:
            assert int(words[-1]) >> (case["T"] % 32) == 0, "bits beyond T"
    finally:
        plan.close()
    return last, slot


SHAPES = sc.shape_cases()


@pytest.mark.parametrize("name,case,script", SHAPES, ids=[c[0] for c in SHAPES])
def test_every_named_shape_equals_the_model_after_every_append(name, case, script):
    """S1 on 2W = 64, 4096 and 4098 with first_bit 0, 5 and 31: what each script holds is in tests/sampled_cases.py."""
    _run_script(case, script)


TILES = sc.tile_cases()


@pytest.mark.parametrize("name,case,script", TILES, ids=[c[0] for c in TILES])
def test_windows_of_whole_tiles_the_tie_run_and_the_limit_window(name, case, script):
    """2W = 4096, 4098 and 8192 with the candidates planted on the tile edges, the peaks picked from a run of exact 0.0
    scores that crosses a tile edge, and the ABI limit 2W = 262 144 on a plan of exactly that many lags (64 tiles,
    lpad = max_lags): what each script holds is in tests/sampled_cases.py and asserted in
    tests/test_sampled_model_host.py."""
    from ffsubsync_amd import _native

    assert 2 * case["W"] <= _native.PROG_MAX_LAGS == pc.MAX_LAGS
    limit = 2 * case["W"] == _native.PROG_MAX_LAGS
    _run_script(case, script, max_lags=_native.PROG_MAX_LAGS if limit else None)


def test_three_windows_in_one_call_leave_the_surplus_tiles_alone():
    """W = 2048, 4096 and 16 in three sampled slots appended in one call: the grid has the two tiles of the widest window
    for every slot, and the workgroups of a tile beyond a slot's own window must return."""
    cases, rounds = sc.tile_slot_cases()
    plan = _plan_for(cases)
    cands = Cands(cases)
    models = [sm.Slot(k["cands"], k["ref_levels"], k["W"], k["T"]) for k in cases]
    mc = plan.max_cand
    try:
        _open_sampled(plan, [0, 1, 2], cases, cands)
        for rnd, spec in enumerate(rounds):
            chunks = [k["ref"][a:a + n] for k, (a, n) in zip(cases, spec)]
            keep = [_dev(_words(ch, 8 + i)) for i, ch in enumerate(chunks)]
            out = Outputs(3, mc)
            plan.append_at([0, 1, 2], [w.data_ptr() for w in keep], [8, 9, 10], [a for a, _ in spec], [n for _, n in spec], 8,
                           40, *out.views())
            recs, states = out.read()
            for i, k in enumerate(cases):
                reps, mstate = models[i].append_at(spec[i][0], chunks[i], 8, 40)
                _check(recs[i], states[i], reps, mstate, len(k["cands"]), 8, ("round", rnd, "slot", i))
                assert [tuple(x) for x in plan.known(i)] == models[i].intervals
    finally:
        plan.close()


ROW_ENDS = sc.row_end_cases()


@pytest.mark.parametrize("T,cases,steps", ROW_ENDS, ids=["T%d" % c[0] for c in ROW_ENDS])
def test_a_segment_ending_at_the_plans_max_ref_samples_stays_inside_the_slots_row(T, cases, steps):
    """Two sampled slots on a plan with ``max_ref_samples`` = T = the slots' declared length, T % 32 = 0, 1 and 31 and no
    padding word behind a row: slot 0 takes a segment ending at T, slot 1 -- the next row of ``ref`` and ``pre_r`` -- is
    fed before and after, its later segments over the words a stray write would land in.  A reference word written past
    slot 0's row shows in slot 1's reference bits, and in its records once a segment is fed over it; a stray ``pre_r``
    entry would not show (every record reads differences of ``pre_r`` from the appended interval's first word on, and the
    append recomputes the row from there: DESIGN 3.23)."""
    plan = _plan_for(cases)
    assert plan.max_cand == 2
    cands = Cands(cases)
    models = [sm.Slot(k["cands"], k["ref_levels"], k["W"], T) for k in cases]
    try:
        _open_sampled(plan, [0, 1], cases, cands)
        for s, a, n, fb in steps:
            chunk = cases[s]["ref"][a:a + n]
            words = _dev(_words(chunk, fb))
            out = Outputs(1, 2)
            plan.append_at([s], [words.data_ptr()], [fb], [a], [n], 3, 8, *out.views())
            recs, states = out.read()
            reps, mstate = models[s].append_at(a, chunk, 3, 8)
            _check(recs[0], states[0], reps, mstate, 2, 3, ("slot", s, "a", a, "n", n))
        for s in (0, 1):
            bits, words = _reference_bits(plan, s, T)
            assert (bits == (models[s].ref & models[s].known)).all(), ("slot", s)
            if T % 32:
                assert int(words[-1]) >> (T % 32) == 0, "bits beyond T"
            assert [tuple(x) for x in plan.known(s)] == models[s].intervals
    finally:
        plan.close()


def test_a_segment_beyond_every_subtitles_reach_alone_is_flat_zero():
    case, script = sc.edge_case()
    n_cand = len(case["cands"])
    plan = _plan_for([case])
    cands = Cands([case])
    a, n, fb = script[0]
    try:
        _open_sampled(plan, [0], [case], cands)
        out = Outputs(1, n_cand)
        words = _dev(_words(np.ones(n, bool), fb))  # all speech, and still nothing to score
        plan.append_at([0], [words.data_ptr()], [fb], [a], [n], case["top_k"], case["e"], *out.views())
        recs, states = out.read()
        for c in range(n_cand):
            assert int(recs[0, c]["flags"]) == qm.FLAT and float(recs[0, c]["mean"]) == 0.0 == float(recs[0, c]["std"])
            assert all(_bits(x) == 0 for x in recs[0, c]["peak_score"]) and int(recs[0, c]["peak_offset"][0]) == case["W"]
        assert int(states[0]["ref_len"]) == n and int(states[0]["flags"]) == qm.FLAT
    finally:
        plan.close()


def test_three_slots_with_different_interval_counts_in_one_call():
    cases, rounds = sc.slot_cases()
    plan = _plan_for(cases)
    cands = Cands(cases)
    models = [sm.Slot(k["cands"], k["ref_levels"], k["W"], k["T"]) for k in cases]
    mc = plan.max_cand
    try:
        _open_sampled(plan, [2, 0, 1], cases, cands, rows=[2, 0, 1])
        for rnd, spec in enumerate(rounds):
            order = [(rnd + i) % 3 for i in range(3)]  # the slots in another order each round
            chunks = [cases[i]["ref"][spec[i][0]:spec[i][0] + spec[i][1]] for i in order]
            keep = [_dev(_words(ch, 5 + i)) for i, ch in enumerate(chunks)]
            out = Outputs(3, mc)
            plan.append_at(order, [w.data_ptr() for w in keep], [5, 6, 7], [spec[i][0] for i in order],
                           [spec[i][1] for i in order], 8, 40, *out.views())
            recs, states = out.read()
            for row, i in enumerate(order):
                reps, mstate = models[i].append_at(spec[i][0], chunks[row], 8, 40)
                _check(recs[row], states[row], reps, mstate, len(cases[i]["cands"]), 8, ("round", rnd, "slot", i))
        assert [len(plan.known(i)) for i in range(3)] == [len(m.intervals) for m in models]
        assert len({len(m.intervals) for m in models}) == 3
    finally:
        plan.close()


def test_records_do_not_depend_on_order_or_cutting():
    """S2: three orders, two cuttings each, byte-identical records on the same K."""
    case, segs = sc.s2_case()
    seen = [_run_script(case, script, poison=False)[0] for script in sc.s2_scripts()]
    assert len(seen) == 6 and all(x == seen[0] for x in seen[1:])


def test_a_prefix_equals_the_prefix_slot_byte_for_byte():
    """S3: slot 0 sampled and fed [0, L) at its positions, slot 1 of the same plan a prefix slot fed the same cuts."""
    case, cuts = sc.s3_case()
    n_cand = len(case["cands"])
    plan = _plan_for([case], n_slots=2)
    cands = Cands([case])
    try:
        _open_sampled(plan, [0], [case], cands)
        _open(plan, [1], [case], cands)
        o = 0
        for i, n in enumerate(cuts):
            chunk = case["ref"][o:o + n]
            wa, wp = _dev(_words(chunk, 31)), _dev(_words(chunk, i % 32))
            oa, op = Outputs(1, n_cand), Outputs(1, n_cand)
            plan.append_at([0], [wa.data_ptr()], [31], [o], [n], case["top_k"], case["e"], *oa.views())
            plan.append([1], [wp.data_ptr()], [i % 32], [n], case["top_k"], case["e"], *op.views())
            o += n
            (ra, sa), (rp, sp) = oa.read(), op.read()
            assert ra.tobytes() == rp.tobytes() and sa.tobytes() == sp.tobytes(), o
            assert int(sa[0]["ref_len"]) == o
        assert o == case["T"] and [tuple(x) for x in plan.known(0)] == [(0, o)]
    finally:
        plan.close()


def _float_batch(torch, ref, cands):
    """DeviceBatch of one pair: an FFS_DTYPE_F32 reference, bit-packed candidates."""
    from ffsubsync_amd import _native
    from ffsubsync_amd.batch import DeviceBatch, _layout

    lens = np.array([[ref.size] + [len(s) for s, _ in cands]], np.int64)
    nbytes = lens.copy()
    nbytes[:, 0] = lens[:, 0] * 4
    nbytes[:, 1:] = (lens[:, 1:] + 31) // 32 * 4
    offs, total = _layout(lens, nbytes)
    host = np.zeros(total, np.uint8)
    r = np.ascontiguousarray(ref, dtype=np.float32)
    assert np.array_equal(r.astype(np.float64), ref)  # the type holds the three levels exactly
    host[offs[0, 0]:offs[0, 0] + r.nbytes] = r.view(np.uint8)
    lo, hi = np.zeros(lens.shape), np.ones(lens.shape)
    lo[0, 0], hi[0, 0] = float(r.min()), float(r.max())
    for j, (s, lv) in enumerate(cands):
        raw = np.packbits(np.asarray(s).astype(np.uint8), bitorder="little")
        host[offs[0, 1 + j]:offs[0, 1 + j] + raw.size] = raw
        lo[0, 1 + j], hi[0, 1 + j] = lv
    return DeviceBatch(torch.from_numpy(host).cuda(), offs, lens, lo, hi, _native.FFS_DTYPE_U1, ref_dtype=_native.FFS_DTYPE_F32)


def test_the_decision_equals_align_batch_and_the_reference_aligner_on_the_half_filled_vector():
    """S4: wherever the reference's lag mask is the window (asserted), (best_cand, offset) after every append equal
    ffs_align_batch's on the float32 reference with levels {lo, (lo + hi) / 2, hi} and the unmodified reference
    aligner's on that vector; scores within the model's slack.  The exact top-2 gap of every state is above 0.5
    (asserted here and in tests/test_sampled_model_host.py): nothing is skipped for a tie."""
    import torch

    from ffsubsync_amd import batch
    from oracle import aligners_oracle as ao

    case, script = sc.s4_case()
    n_cand, W = len(case["cands"]), case["W"]
    assert all(pm.window_is_reference_mask(case["T"], len(s), W) for s, _ in case["cands"])
    plan = _plan_for([case])
    cands = Cands([case])
    slot = sm.Slot(case["cands"], case["ref_levels"], W, case["T"])
    try:
        _open_sampled(plan, [0], [case], cands)
        for a, n, fb in script:
            chunk = case["ref"][a:a + n]
            words = _dev(_words(chunk, fb))
            out = Outputs(1, n_cand)
            plan.append_at([0], [words.data_ptr()], [fb], [a], [n], case["top_k"], case["e"], *out.views())
            recs, states = out.read()
            slot.append_at(a, chunk, case["top_k"], case["e"])
            gap, want = sm.decision_gap(slot)
            assert gap > 0.5, (a, gap)
            st = states[0]
            assert (int(st["best_cand"]), int(st["offset"])) == want, a
            filled = slot.filled(0.5)
            db = _float_batch(torch, filled, case["cands"])
            al = batch.BatchAligner(db.required_fft_length(W), n_cand, W, pairs_in_flight=1, algorithm="runs")
            try:
                _, pres = al.solve(db)
            finally:
                al.close()
            slack = slot.slack(want[0])  # scores_from_counts' slack of the winning candidate
            assert (int(pres[0]["best_cand"]), int(pres[0]["offset"])) == want, a
            assert abs(float(pres[0]["score"]) - float(st["score"])) <= slack, a
            (score, offset), index = ao.max_score_align(filled, [np.where(s, lv[1], lv[0]) for s, lv in slot.cands], W)
            assert (index, offset) == want and abs(score - float(st["score"])) <= slack, a
    finally:
        plan.close()


def test_a_slot_reopened_as_a_prefix_slot_and_back():
    first, prefix, again = sc.reopen_cases()
    cases = [first, prefix, again]
    plan = _plan_for(cases)
    cands = Cands(cases)
    mc = plan.max_cand

    def feed_sampled(row, model, appends):
        for a, n in appends:
            chunk = cases[row]["ref"][a:a + n]
            w = _dev(_words(chunk, 5))
            out = Outputs(1, mc)
            plan.append_at([0], [w.data_ptr()], [5], [a], [n], 3, 40, *out.views())
            recs, states = out.read()
            reps, mstate = model.append_at(a, chunk, 3, 40)
            _check(recs[0], states[0], reps, mstate, len(cases[row]["cands"]), 3, ("row", row, a, n))

    try:
        _open_sampled(plan, [0], cases, cands, rows=[0])
        feed_sampled(0, sm.Slot(first["cands"], first["ref_levels"], first["W"], first["T"]), [(2000, 1000), (0, 700), (1000, 33)])
        _open(plan, [0], cases, cands, rows=[1])  # stale reference bits, prefix sums or curves would show
        model, o = pm.Slot(prefix["cands"], prefix["ref_levels"], prefix["W"]), 0
        for n in (100, 33, 567):
            chunk = prefix["ref"][o:o + n]
            o += n
            w = _dev(_words(chunk, 31))
            out = Outputs(1, mc)
            plan.append([0], [w.data_ptr()], [31], [n], 3, 40, *out.views())
            recs, states = out.read()
            reps, mstate = model.append(chunk, 3, 40)
            _check(recs[0], states[0], reps, mstate, 2, 3, ("prefix", o))
        _open_sampled(plan, [0], cases, cands, rows=[2])
        assert len(plan.known(0)) == 0
        feed_sampled(2, sm.Slot(again["cands"], again["ref_levels"], again["W"], again["T"]), [(3000, 100), (50, 64), (0, 50)])
    finally:
        plan.close()


def test_open_and_six_appends_queued_on_a_side_stream():
    import torch

    case, script = sc.queue_case()
    n_cand = len(case["cands"])
    plan = _plan_for([case])
    cands = Cands([case])
    side = torch.cuda.Stream()
    outs, words = [], []
    for a, n, fb in script:
        words.append(_dev(_words(case["ref"][a:a + n], fb)))
        outs.append(Outputs(1, n_cand))
    assert len(script) == 6
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side):
            _open_sampled(plan, [0], [case], cands)
            for w, out, (a, n, fb) in zip(words, outs, script):
                plan.append_at([0], [w.data_ptr()], [fb], [a], [n], case["top_k"], case["e"], *out.views())
        side.synchronize()
        slot = sm.Slot(case["cands"], case["ref_levels"], case["W"], case["T"])
        for out, (a, n, fb) in zip(outs, script):
            recs, states = out.read()
            reps, mstate = slot.append_at(a, case["ref"][a:a + n], case["top_k"], case["e"])
            _check(recs[0], states[0], reps, mstate, n_cand, case["top_k"], ("queued", a, n))
    finally:
        plan.close()


def test_256_one_sample_intervals_are_accepted_and_the_257th_is_refused():
    from ffsubsync_amd import _native

    case = sc.interval_limit_case()
    plan = _plan_for([case])
    cands = Cands([case])
    try:
        _open_sampled(plan, [0], [case], cands)
        out = None
        for k in range(sc.MAX_INTERVALS):
            a = 2 * k
            w = _dev(_words(case["ref"][a:a + 1], 31))
            out = Outputs(1, 1)
            plan.append_at([0], [w.data_ptr()], [31], [a], [1], case["top_k"], case["e"], *out.views())
            if k % 64 == 63:
                recs, states = out.read()
                assert int(states[0]["ref_len"]) == k + 1
        known = plan.known(0)
        assert known.shape == (256, 2) and (known[:, 0] == 2 * np.arange(256)).all() and (known[:, 1] == known[:, 0] + 1).all()
        recs, states = out.read()
        model = sm.Slot(case["cands"], case["ref_levels"], case["W"], case["T"])
        for a in range(0, 512, 2):
            reps, mstate = model.append_at(a, case["ref"][a:a + 1], case["top_k"], case["e"])
        _check(recs[0], states[0], reps, mstate, 1, case["top_k"], "256 intervals")
        w = _dev(_words(case["ref"][512:513], 0))
        guard = Outputs(1, 1)
        with pytest.raises(_native.NativeError, match="more than 256 known intervals") as err:
            plan.append_at([0], [w.data_ptr()], [0], [512], [1], case["top_k"], case["e"], *guard.views())
        assert err.value.code == -1
        guard.read()
        assert bool((guard.cand == 0xA5).all()) and bool((guard.state == 0xA5).all())
        assert len(plan.known(0)) == 256
        for a in (1, 511):  # one that joins two (255 intervals), one that extends the last (still 255)
            w = _dev(_words(case["ref"][a:a + 1], 5))
            out = Outputs(1, 1)
            plan.append_at([0], [w.data_ptr()], [5], [a], [1], case["top_k"], case["e"], *out.views())
            recs, states = out.read()
            reps, mstate = model.append_at(a, case["ref"][a:a + 1], case["top_k"], case["e"])
            _check(recs[0], states[0], reps, mstate, 1, case["top_k"], ("join", a))
        assert [tuple(x) for x in plan.known(0)] == model.intervals and len(model.intervals) == 255
    finally:
        plan.close()


def test_every_refusal_leaves_state_and_outputs_untouched():
    import torch

    from ffsubsync_amd import _native

    case = sc.refusal_case()
    T = case["T"]
    plan = _native.ProgPlan(3, 2, 32, T, 700)
    cands = Cands([case])
    slot = sm.Slot(case["cands"], case["ref_levels"], case["W"], T)
    good = dict(slot=[0], n_cand=[2], ptr=[[cands.ptr(0, 0), cands.ptr(0, 1)]], length=[[700, 33]], lo=[[0.0, 0.0]],
                hi=[[1.0, case["cands"][1][1][1]]], r_lo=[0.0], r_hi=[1.0], w=[16], total=[T])

    def open_with(**kw):
        a = dict(good, **kw)
        plan.open_sampled(a["slot"], a["n_cand"], a["ptr"], a["length"], a["lo"], a["hi"], a["r_lo"], a["r_hi"], a["w"], a["total"])

    try:
        open_with()
        plan.open([1], good["n_cand"], good["ptr"], good["length"], good["lo"], good["hi"], [0.0], [1.0], [16])  # a prefix slot
        free = iter(range(100, T - 10, 9))

        def valid(n):
            a = next(free)
            chunk = case["ref"][a:a + n]
            out = Outputs(1, 2)
            w = _dev(_words(chunk, 8))
            plan.append_at([0], [w.data_ptr()], [8], [a], [n], 2, 5, *out.views())
            recs, states = out.read()
            reps, mstate = slot.append_at(a, chunk, 2, 5)
            _check(recs[0], states[0], reps, mstate, 2, 2, ("after refusal", a))
            assert [tuple(x) for x in plan.known(0)] == slot.intervals

        w = _dev(_words(case["ref"][:64], 0))
        out = Outputs(2, 2)  # (room for the call that names a slot twice)
        co, so = out.views()
        plan_known = lambda: [tuple(x) for x in plan.known(0)]
        first = Outputs(1, 2)
        plan.append_at([0], [w.data_ptr()], [0], [40], [20], 2, 5, *first.views())  # K = [40, 60)
        slot.append_at(40, case["ref"][:20], 2, 5)
        first.read()
        bad_appends = [
            dict(ptr=[0]), dict(ptr=[w.data_ptr() + 2]), dict(fb=[32]), dict(fb=[-1]), dict(n=[-1]),
            dict(a=[-1]), dict(a=[T - 4]), dict(a=[T + 1], n=[0]), dict(a=[0], n=[T + 1]),  # outside [0, T)
            dict(a=[40]), dict(a=[59]), dict(a=[36]), dict(a=[30], n=[40]), dict(a=[45], n=[1]),  # overlaps K
            dict(slot=[1]),  # a prefix slot
            dict(slot=[3]), dict(slot=[-1]), dict(slot=[2]),  # out of range; not open
            dict(slot=[0, 0], ptr=[w.data_ptr()] * 2, fb=[0, 0], a=[0, 10], n=[5, 5]), dict(top_k=0), dict(top_k=9), dict(e=0),
            dict(cand=out.cand[GUARD - 7:]), dict(state=out.state[GUARD - 4:]),
        ]
        for bad in bad_appends:
            a = dict(dict(slot=[0], ptr=[w.data_ptr()], fb=[0], a=[0], n=[5], top_k=2, e=5, cand=co, state=so), **bad)
            before = plan_known()
            with pytest.raises(_native.NativeError) as err:
                plan.append_at(a["slot"], a["ptr"], a["fb"], a["a"], a["n"], a["top_k"], a["e"], a["cand"], a["state"])
            assert err.value.code == -1, bad
            torch.cuda.synchronize()
            assert bool((out.cand == 0xA5).all()) and bool((out.state == 0xA5).all()), bad
            assert plan_known() == before, bad
            valid(7)
        with pytest.raises(_native.NativeError, match="sampled slot") as err:  # ffs_prog_append on a sampled slot
            plan.append([0], [w.data_ptr()], [0], [5], 2, 5, co, so)
        assert err.value.code == -1
        torch.cuda.synchronize()
        assert bool((out.cand == 0xA5).all()) and bool((out.state == 0xA5).all())
        valid(3)
        nan = float("nan")
        bad_opens = [dict(total=[0]), dict(total=[-5]), dict(total=[T + 1]), dict(slot=[3]), dict(n_cand=[0]), dict(n_cand=[3]),
                     dict(length=[[0, 33]]), dict(length=[[701, 33]]), dict(w=[0]), dict(w=[17]), dict(hi=[[nan, 1.0]]),
                     dict(r_lo=[float("inf")]), dict(ptr=[[0, cands.ptr(0, 1)]]),
                     dict(slot=[2, 2], n_cand=[2, 2], ptr=good["ptr"] * 2, length=good["length"] * 2, lo=good["lo"] * 2,
                          hi=good["hi"] * 2, r_lo=[0.0] * 2, r_hi=[1.0] * 2, w=[16, 16], total=[T, T])]
        for bad in bad_opens:
            with pytest.raises(_native.NativeError) as err:
                open_with(**bad)
            assert err.value.code == -1, bad
            valid(3)  # slot 0 is still the open problem it was
        for call in (lambda: plan.known(1), lambda: plan.known(2), lambda: plan.known(3)):  # prefix, not open, out of range
            with pytest.raises(_native.NativeError):
                call()
        valid(0)
        assert plan.reference(0)[1] == T and plan.reference(1)[1] == 0
        plan.close_slots([0])
        with pytest.raises(_native.NativeError, match="not open"):
            plan.append_at([0], [w.data_ptr()], [0], [0], [5], 2, 5, co, so)
    finally:
        plan.close()


def test_a_refusal_at_the_second_of_two_slots_leaves_the_first_untouched():
    """Every per-slot check of every named slot comes before any slot's state changes: a call that names [0, 1] with a
    good entry for slot 0 and a bad one for slot 1 is refused whole, and slot 0 knows no more than before."""
    import torch

    from ffsubsync_amd import _native

    case = sc.refusal_case()
    T = case["T"]
    plan = _native.ProgPlan(3, 2, 32, T, 700)
    cands = Cands([case])
    models = [sm.Slot(case["cands"], case["ref_levels"], case["W"], T) for _ in range(2)]

    def valid(starts, ns):
        chunks = [case["ref"][a:a + n] for a, n in zip(starts, ns)]
        keep = [_dev(_words(c, 8)) for c in chunks]
        out = Outputs(2, 2)
        plan.append_at([0, 1], [k.data_ptr() for k in keep], [8, 8], starts, ns, 2, 5, *out.views())
        recs, states = out.read()
        for s in range(2):
            reps, mstate = models[s].append_at(starts[s], chunks[s], 2, 5)
            _check(recs[s], states[s], reps, mstate, 2, 2, ("slot", s, "a", starts[s]))
            assert [tuple(x) for x in plan.known(s)] == models[s].intervals, s

    try:
        _open_sampled(plan, [0, 1], [case], cands, rows=[0, 0])
        valid([100, 40], [20, 20])  # slot 1 knows [40, 60)
        w = _dev(_words(case["ref"][:64], 0))
        out = Outputs(2, 2)
        co, so = out.views()
        bad_second = [dict(ptr=0), dict(ptr=w.data_ptr() + 2), dict(fb=32), dict(n=-1), dict(a=T - 4), dict(a=58),
                      dict(other_kind=True)]
        for bad in bad_second:
            a = dict(dict(ptr=w.data_ptr(), fb=0, a=200, n=5), **bad)
            if bad.get("other_kind"):  # slot 1 is a prefix slot for this one call
                _open(plan, [1], [case], cands, rows=[0])
            before, length = [tuple(x) for x in plan.known(0)], plan.reference(0)[1]
            with pytest.raises(_native.NativeError) as err:
                plan.append_at([0, 1], [w.data_ptr(), a["ptr"]], [0, a["fb"]], [0, a["a"]], [5, a["n"]], 2, 5, co, so)
            assert err.value.code == -1, bad
            torch.cuda.synchronize()
            assert bool((out.cand == 0xA5).all()) and bool((out.state == 0xA5).all()), bad
            assert [tuple(x) for x in plan.known(0)] == before == models[0].intervals, bad
            assert plan.reference(0)[1] == length == T, bad
            if bad.get("other_kind"):  # and a fresh sampled slot again
                _open_sampled(plan, [1], [case], cands, rows=[0])
                models[1] = sm.Slot(case["cands"], case["ref_levels"], case["W"], T)
        valid([0, 200], [7, 9])
    finally:
        plan.close()
