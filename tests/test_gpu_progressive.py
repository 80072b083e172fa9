"""Progressive alignment on the device (csrc/ffs_progressive.h through ``_native.ProgPlan``) against the
numpy model tests/progressive_model.py after EVERY append: peaks bit for bit, mean and std at the tolerance
tests/test_gpu_quality.py uses for the same record.  Shapes from tests/progressive_cases.py."""
import numpy as np
import pytest

import progressive_cases as pc
import progressive_model as pm

pytestmark = pytest.mark.gpu
REC, STATE = 160, 64
GUARD = 64  # bytes of 0xA5 in front of and behind each output


def _bits(x):
    return np.float64(x).view(np.int64)


def _same_float(a, b):
    return (np.isnan(a) and np.isnan(b)) or _bits(a) == _bits(b)


def _close(got, want, sum_bound):
    """tests/test_gpu_quality.py's tolerance for mean and std (1e-9 relative), plus the model's own summation error:
    where the scores cancel (a mean of exactly 0.0 on the device, -7e-19 in numpy) a relative bound alone asks for
    digits that neither side has."""
    return abs(got - want) <= 1e-9 * abs(want) + sum_bound


def _words(bits, first_bit=0, fill=True):
    """uint32 words that hold ``bits`` from bit ``first_bit``; every other bit is ``fill``."""
    n = len(bits)
    n_words = max((first_bit + n + 31) // 32, 1)
    flat = np.full(32 * n_words, fill, bool)
    flat[first_bit:first_bit + n] = bits
    return np.packbits(flat, bitorder="little").view(np.uint32)


def _dev(words):
    import torch

    return torch.from_numpy(words.view(np.int32).copy()).cuda()


class Cands:
    """The candidates of some cases in ONE buffer, one guard word of ones between neighbours, tail bits set."""

    def __init__(self, cases):
        parts, self.at = [np.array([0xFFFFFFFF], np.uint32)], []
        for case in cases:
            row = []
            for s, _ in case["cands"]:
                row.append(sum(p.size for p in parts))
                parts += [_words(s), np.array([0xFFFFFFFF], np.uint32)]
            self.at.append(row)
        self.data = _dev(np.concatenate(parts))
        self.clone = self.data.clone()

    def ptr(self, i, c):
        return self.data.data_ptr() + 4 * self.at[i][c]


class Outputs:
    """Record outputs of a call on n slots, with guard bytes around both."""

    def __init__(self, n, max_cand):
        import torch

        self.n, self.mc = n, max_cand
        self.cand = torch.full((2 * GUARD + n * max_cand * REC,), 0xA5, dtype=torch.uint8, device="cuda")
        self.state = torch.full((2 * GUARD + n * STATE,), 0xA5, dtype=torch.uint8, device="cuda")

    def views(self):
        return self.cand[GUARD:GUARD + self.n * self.mc * REC], self.state[GUARD:GUARD + self.n * STATE]

    def read(self):
        from ffsubsync_amd import _native

        c, s = self.cand.cpu().numpy(), self.state.cpu().numpy()
        for buf in (c, s):
            assert (buf[:GUARD] == 0xA5).all() and (buf[-GUARD:] == 0xA5).all(), "guard bytes written"
        return (c[GUARD:-GUARD].view(_native.QUALITY_RESULT_DTYPE).reshape(self.n, self.mc),
                s[GUARD:-GUARD].view(_native.PROG_STATE_DTYPE))


def _open(plan, slots, cases, cands, rows=None):
    mc = plan.max_cand
    rows = range(len(cases)) if rows is None else rows
    n = len(slots)
    ptr, length = np.zeros((n, mc), np.uint64), np.ones((n, mc), np.int64)
    lo, hi = np.zeros((n, mc)), np.ones((n, mc))
    for i, row in enumerate(rows):
        for c, (s, lv) in enumerate(cases[row]["cands"]):
            ptr[i, c], length[i, c], lo[i, c], hi[i, c] = cands.ptr(row, c), len(s), lv[0], lv[1]
    sel = [cases[r] for r in rows]
    plan.open(slots, [len(k["cands"]) for k in sel], ptr, length, lo, hi, [k["ref_levels"][0] for k in sel],
              [k["ref_levels"][1] for k in sel], [k["W"] for k in sel])


def _check(recs, state, reps, mstate, n_cand, top_k, where):
    """One slot's device records against the model's."""
    for c in range(recs.size):
        r = recs[c]
        if c >= n_cand:
            assert r.tobytes() == bytes(REC), (where, c, "records beyond n_cand must be zeros")
            continue
        rep = reps[c]
        assert int(r["n_lags"]) == rep["n_lags"] and int(r["n_peaks"]) == len(rep["peaks"]), (where, c, r, rep)
        for k, (ms, mo) in enumerate(rep["peaks"]):
            assert int(r["peak_offset"][k]) == mo and _bits(r["peak_score"][k]) == _bits(ms), \
                (where, c, k, float(r["peak_score"][k]), int(r["peak_offset"][k]), ms, mo)
        assert _close(float(r["mean"]), rep["mean"], rep["sum_bound"]), (where, c, float(r["mean"]), rep)
        assert _close(float(r["std"]), rep["std"], rep["sum_bound"]), (where, c, float(r["std"]), rep)
        assert (int(r["flags"]) & 1) == (rep["flags"] & 1), (where, c)
    b = int(state["best_cand"])
    assert (int(state["ref_len"]), b, int(state["offset"])) == (mstate["ref_len"], mstate["best_cand"], mstate["offset"]), \
        (where, state, mstate)
    for name in ("score", "runner_up", "other_best"):
        assert _same_float(state[name], mstate[name]), (where, name, state, mstate)
    assert _bits(state["mean"]) == _bits(recs[b]["mean"]) and _bits(state["std"]) == _bits(recs[b]["std"]), where
    assert int(state["flags"]) == int(recs[b]["flags"]), where


def _run_single(case, cuts, first_bit, poison=True):
    """One slot through its appends, checked against the model after each; returns the raw bytes per L."""
    from ffsubsync_amd import _native

    n_cand = len(case["cands"])
    plan = _native.ProgPlan(1, max(n_cand, 1), 2 * case["W"], max(case["ref"].size, 1), max(len(s) for s, _ in case["cands"]))
    cands = Cands([case])
    slot = pm.Slot(case["cands"], case["ref_levels"], case["W"])
    seen = {}
    try:
        _open(plan, [0], [case], cands)
        if poison:
            cands.data.fill_(-1)  # queued right behind open: the plan works on its own copy
        o = 0
        for n in cuts:
            chunk = case["ref"][o:o + n]
            o += n
            words = _dev(_words(chunk, first_bit))
            keep = words.clone()
            out = Outputs(1, n_cand)
            plan.append([0], [words.data_ptr()], [first_bit], [n], case["top_k"], case["e"], *out.views())
            if poison:
                words.fill_(0x55555555)  # queued right behind the append
            recs, states = out.read()
            if not poison:
                assert bool((words == keep).all()), "the chunk was written"
            reps, mstate = slot.append(chunk, case["top_k"], case["e"])
            _check(recs[0], states[0], reps, mstate, n_cand, case["top_k"], ("L", o, "n", n))
            seen[o] = recs.tobytes() + states.tobytes()
        if not poison:
            assert bool((cands.data == cands.clone).all()), "the candidates were written"
    finally:
        plan.close()
    return seen


TOTAL_CASES = pc.total_cases()
WINDOW_CASES = pc.window_cases()


@pytest.mark.parametrize("name,case,kind,first_bit", TOTAL_CASES, ids=[c[0] for c in TOTAL_CASES])
def test_totals_and_cuts_equal_the_model_after_every_append(name, case, kind, first_bit):
    _run_single(case, pc.cut(case["ref"].size, kind, seed=len(name)), first_bit)


@pytest.mark.parametrize("name,case,kind,first_bit", WINDOW_CASES, ids=[c[0] for c in WINDOW_CASES])
def test_windows_against_subtitle_lengths(name, case, kind, first_bit):
    _run_single(case, pc.cut(case["ref"].size, kind, seed=len(name)), first_bit, poison=False)


TILE_CASES = pc.tile_cases()


@pytest.mark.parametrize("name,case,cuts,first_bit", TILE_CASES, ids=[c[0] for c in TILE_CASES])
def test_windows_of_whole_tiles_and_the_limit_window(name, case, cuts, first_bit):
    """2W = 4096, 4098 and 8192 lags (one full tile of k_prog_counts, a tile and two lags, two full tiles) and the ABI
    limit 2W = 262 144 on a plan of exactly that many lags: 64 tiles, lpad = max_lags."""
    from ffsubsync_amd import _native

    assert 2 * case["W"] <= _native.PROG_MAX_LAGS == pc.MAX_LAGS
    _run_single(case, cuts, first_bit)


def test_three_windows_in_one_call_leave_the_surplus_tiles_alone():
    """W = 2048, 4096 and 16 in three slots appended in one call: the grid has the two tiles of the largest window for
    every slot, and the workgroups of a tile beyond a slot's own window must return."""
    from ffsubsync_amd import _native

    cases, rounds = pc.tile_slot_cases()
    plan = _native.ProgPlan(3, 2, 8192, 1000, 5000)
    cands = Cands(cases)
    models = [pm.Slot(k["cands"], k["ref_levels"], k["W"]) for k in cases]
    pos = [0, 0, 0]
    try:
        _open(plan, [0, 1, 2], cases, cands)
        for rnd, ns in enumerate(rounds):
            chunks = [k["ref"][p:p + n] for k, p, n in zip(cases, pos, ns)]
            pos = [p + n for p, n in zip(pos, ns)]
            keep = [_dev(_words(ch, 8 + i)) for i, ch in enumerate(chunks)]
            out = Outputs(3, 2)
            plan.append([0, 1, 2], [w.data_ptr() for w in keep], [8, 9, 10], list(ns), 8, 40, *out.views())
            recs, states = out.read()
            for i, k in enumerate(cases):
                reps, mstate = models[i].append(chunks[i], 8, 40)
                _check(recs[i], states[i], reps, mstate, len(k["cands"]), 8, ("round", rnd, "slot", i))
    finally:
        plan.close()


def test_records_equal_quality_batch_at_a_full_tile():
    """E2 at W = 2048, L = S = 2100: wherever the reference's own mask is the window (checked on the host; L = 2100 is
    such a place) the records are byte-identical to quality_batch(raw=True)."""
    from ffsubsync_amd import _native, batch, quality
    from ffsubsync_amd.subtitle_raster import DeviceRaster

    case, cuts = pc.tile_e2_case()
    W, (s, lv) = case["W"], case["cands"][0]
    plan = _native.ProgPlan(1, 1, 2 * W, 2100, 2100)
    cands = Cands([case])
    checked = []
    try:
        _open(plan, [0], [case], cands)
        o = 0
        for n in cuts:
            chunk = case["ref"][o:o + n]
            o += n
            out = Outputs(1, 1)
            words = _dev(_words(chunk, 31))
            plan.append([0], [words.data_ptr()], [31], [n], case["top_k"], case["e"], *out.views())
            recs, _ = out.read()
            if not pm.window_is_reference_mask(o, len(s), W):
                continue
            ref = DeviceRaster(_dev(_words(case["ref"][:o], fill=False)), 0.0, 1.0, o)
            sub = DeviceRaster(_dev(_words(s, fill=False)), lv[0], lv[1], len(s))
            want = quality.quality_batch(batch.pack_pairs([(ref, [sub])]), W, case["top_k"], case["e"], raw=True)
            assert want.tobytes() == recs[0, :1].tobytes(), o
            checked.append(o)
    finally:
        plan.close()
    assert 2100 in checked and len(checked) >= 2


def test_an_append_longer_than_the_staged_piece():
    from ffsubsync_amd import _native

    piece = _native.PROG_PIECE_SAMPLES
    case = pc.make_case(900, 2 * piece + 1500, [pc.PIECE_SUB, 700], 2500, top_k=3, exclusion=300)
    _run_single(case, [100, piece + 777, 5, piece + 1500 - 882], 8)


def test_records_do_not_depend_on_the_cuts():
    """E3: two cuts of the same reference, byte-identical records at every common L."""
    case = pc.make_case(901, 1000, [700, 33, 5000], 600, (0.1, 1.0), top_k=4)
    cycle = pc.cut(1000, "cycle")
    meet = [0] + [int(x) for x in np.cumsum(cycle)[4::6]] + [1000]  # every sixth L of the first cut, reached otherwise
    other = [n for i, (lo, hi) in enumerate(zip(meet, meet[1:])) for n in pc.cut(hi - lo, "random", seed=i)]
    a = _run_single(case, cycle, 0)
    b = _run_single(case, other, 31)
    c = _run_single(case, [1000], 1)
    common = sorted(set(a) & set(b))
    assert len(common) >= 4 and 1000 in common and other != cycle
    for L in common:
        assert a[L] == b[L], L
    assert a[1000] == c[1000]


def test_records_equal_quality_batch_and_the_solve_where_the_masks_coincide():
    """E2: at W < L and W <= S + 1 (checked with the reference's own mask on the host) the candidate records are
    byte-identical to quality_batch(raw=True) and (best_cand, offset, score) is align_batch's pair record."""
    from ffsubsync_amd import _native, batch, quality
    from ffsubsync_amd.subtitle_raster import DeviceRaster

    case = pc.make_case(902, 1000, [700, 600, 5000], 33, (0.0, 1.0), top_k=3, exclusion=10)
    n_cand, W = 3, 33
    plan = _native.ProgPlan(1, n_cand, 2 * W, 1000, 5000)
    cands = Cands([case])
    checked = 0
    try:
        _open(plan, [0], [case], cands)
        o = 0
        for n in (20, 14, 66, 400, 500):
            chunk = case["ref"][o:o + n]
            o += n
            out = Outputs(1, n_cand)
            words = _dev(_words(chunk, 8))
            plan.append([0], [words.data_ptr()], [8], [n], 3, 10, *out.views())
            recs, states = out.read()
            if not all(pm.window_is_reference_mask(o, len(s), W) for s, _ in case["cands"]):
                continue
            ref = DeviceRaster(_dev(_words(case["ref"][:o], fill=False)), 0.0, 1.0, o)
            subs = [DeviceRaster(_dev(_words(s, fill=False)), lv[0], lv[1], len(s)) for s, lv in case["cands"]]
            for c in range(n_cand):
                want = quality.quality_batch(batch.pack_pairs([(ref, [subs[c]])]), W, 3, 10, raw=True)
                assert want.tobytes() == recs[0, c:c + 1].tobytes(), (o, c)
            db = batch.pack_pairs([(ref, subs)])
            al = batch.BatchAligner(db.required_fft_length(W), n_cand, W, pairs_in_flight=1)
            try:
                _, pres = al.solve(db)
            finally:
                al.close()
            st = states[0]
            assert (int(st["best_cand"]), int(st["offset"])) == (int(pres[0]["best_cand"]), int(pres[0]["offset"])), o
            assert _bits(st["score"]) == _bits(pres[0]["score"]), o
            checked += 1
    finally:
        plan.close()
    assert checked >= 3


def _slot_cases():
    return [pc.make_case(910, 700, [700, 33], 600, (0.0, 1.0)), pc.make_case(911, 95, [5000], 33, (0.1, 1.0)),
            pc.make_case(912, 1000, [31, 700, 1, 33, 700, 5000, 31, 33], 16), pc.make_case(913, 333, [700, 700, 700], 2500),
            pc.make_case(914, 64, [33], 1), pc.make_case(915, 200, [31, 700], 16, (0.1, 1.0))]  # [5]: reopened on slot 1


def test_slots_interleaved_subsets_permuted_and_one_reopened():
    from ffsubsync_amd import _native

    cases = _slot_cases()
    plan = _native.ProgPlan(5, 8, 5000, 1000, 5000)
    cands = Cands(cases)
    models = [pm.Slot(k["cands"], k["ref_levels"], k["W"]) for k in cases]
    which = [0, 1, 2, 3, 4]  # the case a slot holds
    pos = [0] * 6
    rng = np.random.RandomState(3)
    try:
        _open(plan, [3, 0, 4, 1, 2], cases, cands, rows=[3, 0, 4, 1, 2])
        for rnd in range(14):
            if rnd == 6:  # slot 1 is closed and reopened on a shorter problem: stale curves or prefix sums would show
                plan.close_slots([1])
                _open(plan, [1], cases, cands, rows=[5])
                which[1] = 5
            slots = [int(s) for s in rng.permutation(5)[:int(rng.randint(1, 6))]]
            ns, ptrs, keep, chunks = [], [], [], []
            for s in slots:
                k = which[s]
                n = min(int(rng.randint(0, 120)), cases[k]["ref"].size - pos[k])
                chunks.append(cases[k]["ref"][pos[k]:pos[k] + n])
                pos[k] += n
                keep.append(_dev(_words(chunks[-1], s)))
                ptrs.append(keep[-1].data_ptr())
                ns.append(n)
            out = Outputs(len(slots), 8)
            plan.append(slots, ptrs, slots, ns, 3, 40, *out.views())  # (first_bit = the slot's number)
            recs, states = out.read()
            for i, s in enumerate(slots):
                k = which[s]
                reps, mstate = models[k].append(chunks[i], 3, 40)
                _check(recs[i], states[i], reps, mstate, len(cases[k]["cands"]), 3, ("round", rnd, "slot", s))
        ptr, n = plan.reference(1)
        assert n == pos[5] > 0
    finally:
        plan.close()


def test_open_and_six_appends_queued_on_a_side_stream():
    import torch

    from ffsubsync_amd import _native

    case = pc.make_case(920, 700, [700, 5000, 33], 600, (0.1, 1.0))
    plan = _native.ProgPlan(1, 3, 1200, 700, 5000)
    cands = Cands([case])
    cuts = [100, 1, 0, 333, 65, 201]
    side = torch.cuda.Stream()
    outs, words = [], []
    o = 0
    for n in cuts:
        words.append(_dev(_words(case["ref"][o:o + n], 1)))
        outs.append(Outputs(1, 3))
        o += n
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side):
            _open(plan, [0], [case], cands)
            for w, out, n in zip(words, outs, cuts):
                plan.append([0], [w.data_ptr()], [1], [n], 3, 75, *out.views())
        side.synchronize()
        slot = pm.Slot(case["cands"], case["ref_levels"], case["W"])
        o = 0
        for out, n in zip(outs, cuts):
            recs, states = out.read()
            reps, mstate = slot.append(case["ref"][o:o + n], 3, 75)
            o += n
            _check(recs[0], states[0], reps, mstate, 3, 3, ("queued", o))
    finally:
        plan.close()


def test_every_refusal_leaves_state_and_outputs_untouched():
    import torch

    from ffsubsync_amd import _native

    case = pc.make_case(930, 300, [700, 33], 16)
    plan = _native.ProgPlan(2, 2, 32, 300, 700)
    cands = Cands([case])
    slot = pm.Slot(case["cands"], case["ref_levels"], case["W"])
    good = dict(slot=[0], n_cand=[2], ptr=[[cands.ptr(0, 0), cands.ptr(0, 1)]], length=[[700, 33]], lo=[[0.0, 0.0]],
                hi=[[1.0, case["cands"][1][1][1]]], r_lo=[0.0], r_hi=[1.0], w=[16])

    def open_with(**kw):
        a = dict(good, **kw)
        plan.open(a["slot"], a["n_cand"], a["ptr"], a["length"], a["lo"], a["hi"], a["r_lo"], a["r_hi"], a["w"])

    try:
        open_with()
        o = [0]

        def valid(n):
            chunk = case["ref"][o[0]:o[0] + n]
            o[0] += n
            out = Outputs(1, 2)
            w = _dev(_words(chunk, 8))
            plan.append([0], [w.data_ptr()], [8], [n], 2, 5, *out.views())
            recs, states = out.read()
            reps, mstate = slot.append(chunk, 2, 5)
            _check(recs[0], states[0], reps, mstate, 2, 2, ("after refusal", o[0]))

        valid(40)
        w = _dev(_words(case["ref"][:64], 0))
        out = Outputs(2, 2)  # (room for the call that names a slot twice)
        co, so = out.views()
        bad_appends = [
            dict(slot=[0], ptr=[0]), dict(slot=[0], ptr=[w.data_ptr() + 2]), dict(slot=[0], fb=[32]), dict(slot=[0], fb=[-1]),
            dict(slot=[0], n=[-1]), dict(slot=[0], n=[261]), dict(slot=[2]), dict(slot=[-1]), dict(slot=[1]),
            dict(slot=[0, 0], ptr=[w.data_ptr()] * 2, fb=[0, 0], n=[5, 5]), dict(slot=[0], top_k=0), dict(slot=[0], top_k=9),
            dict(slot=[0], e=0), dict(slot=[0], cand=out.cand[GUARD - 7:]), dict(slot=[0], state=out.state[GUARD - 4:]),
        ]
        for bad in bad_appends:
            a = dict(dict(ptr=[w.data_ptr()], fb=[0], n=[5], top_k=2, e=5, cand=co, state=so), **bad)
            with pytest.raises(_native.NativeError) as err:
                plan.append(a["slot"], a["ptr"], a["fb"], a["n"], a["top_k"], a["e"], a["cand"], a["state"])
            assert err.value.code == -1, bad
            torch.cuda.synchronize()
            assert bool((out.cand == 0xA5).all()) and bool((out.state == 0xA5).all()), bad
            valid(7)
        nan = float("nan")
        bad_opens = [dict(slot=[2]), dict(slot=[1, 1], n_cand=[2, 2], ptr=good["ptr"] * 2, length=good["length"] * 2,
                                          lo=good["lo"] * 2, hi=good["hi"] * 2, r_lo=[0.0] * 2, r_hi=[1.0] * 2, w=[16, 16]),
                     dict(n_cand=[0]), dict(n_cand=[3]), dict(length=[[0, 33]]), dict(length=[[701, 33]]), dict(w=[0]),
                     dict(w=[17]), dict(hi=[[nan, 1.0]]), dict(r_lo=[float("inf")]), dict(ptr=[[0, cands.ptr(0, 1)]]),
                     dict(ptr=[[cands.ptr(0, 0) + 1, cands.ptr(0, 1)]])]
        for bad in bad_opens:
            with pytest.raises(_native.NativeError) as err:
                open_with(**bad)
            assert err.value.code == -1, bad
            valid(3)  # slot 0 is still the open problem it was
        for call in (lambda: plan.close_slots([1]), lambda: plan.close_slots([0, 0]), lambda: plan.reference(1),
                     lambda: plan.reference(2)):
            with pytest.raises(_native.NativeError):
                call()
        valid(0)
        plan.close_slots([0])
        with pytest.raises(_native.NativeError, match="not open"):
            plan.append([0], [w.data_ptr()], [0], [5], 2, 5, co, so)
        for dims in ((0, 1, 32, 10, 10), (1, 9, 32, 10, 10), (1, 1, 1, 10, 10), (1, 1, 262146, 10, 10), (1, 1, 32, 0, 10),
                     (1, 1, 32, 10, 0)):
            with pytest.raises(_native.NativeError):
                _native.ProgPlan(*dims)
    finally:
        plan.close()


def test_a_refusal_at_the_second_of_two_slots_leaves_the_first_untouched():
    """Every per-slot check of every named slot comes before any slot's state changes: a call that names [0, 1] with a
    good entry for slot 0 and a bad one for slot 1 is refused whole, and slot 0 has not consumed its entry."""
    import torch

    from ffsubsync_amd import _native

    case = pc.make_case(930, 300, [700, 33], 16)
    plan = _native.ProgPlan(3, 2, 32, 300, 700)
    cands = Cands([case])
    models = [pm.Slot(case["cands"], case["ref_levels"], case["W"]) for _ in range(2)]
    pos = [0, 0]

    def valid(ns):
        chunks = [case["ref"][pos[s]:pos[s] + n] for s, n in enumerate(ns)]
        keep = [_dev(_words(c, 8)) for c in chunks]
        out = Outputs(2, 2)
        plan.append([0, 1], [k.data_ptr() for k in keep], [8, 8], ns, 2, 5, *out.views())
        recs, states = out.read()
        for s, n in enumerate(ns):
            pos[s] += n
            reps, mstate = models[s].append(chunks[s], 2, 5)
            _check(recs[s], states[s], reps, mstate, 2, 2, ("slot", s, "L", pos[s]))

    try:
        _open(plan, [0, 1], [case], cands, rows=[0, 0])
        valid([40, 25])
        w = _dev(_words(case["ref"][:64], 0))
        out = Outputs(2, 2)
        co, so = out.views()
        bad_second = [dict(ptr=0), dict(ptr=w.data_ptr() + 2), dict(fb=32), dict(n=-1), dict(n=300 - 25 + 1),
                      dict(other_kind=True)]
        for bad in bad_second:
            a = dict(dict(ptr=w.data_ptr(), fb=0, n=5), **bad)
            if bad.get("other_kind"):  # slot 1 is a sampled slot for this one call
                _open_sampled_one(plan, case, cands, 1, 300)
            before = plan.reference(0)[1]
            with pytest.raises(_native.NativeError) as err:
                plan.append([0, 1], [w.data_ptr(), a["ptr"]], [0, a["fb"]], [5, a["n"]], 2, 5, co, so)
            assert err.value.code == -1, bad
            torch.cuda.synchronize()
            assert bool((out.cand == 0xA5).all()) and bool((out.state == 0xA5).all()), bad
            assert plan.reference(0)[1] == before == pos[0], bad
            if bad.get("other_kind"):  # and a fresh prefix slot again
                _open(plan, [1], [case], cands, rows=[0])
                models[1], pos[1] = pm.Slot(case["cands"], case["ref_levels"], case["W"]), 0
        valid([7, 9])
    finally:
        plan.close()


def _open_sampled_one(plan, case, cands, slot, total):
    """``slot`` reopened as a sampled slot on ``case`` with a declared length."""
    plan.open_sampled([slot], [2], [[cands.ptr(0, 0), cands.ptr(0, 1)]], [[len(s) for s, _ in case["cands"]]],
                      [[lv[0] for _, lv in case["cands"]]], [[lv[1] for _, lv in case["cands"]]], [case["ref_levels"][0]],
                      [case["ref_levels"][1]], [case["W"]], [total])
