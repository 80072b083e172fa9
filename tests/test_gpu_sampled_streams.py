"""The sampled slots of the progressive plan (``ffs_prog_open_sampled`` / ``ffs_prog_append_at``) under queued
calls, side streams, mixed slot kinds and late inputs, the way tests/test_gpu_progressive_streams.py holds the prefix
slots.  A sampled slot carries more from call to call than anything else in the library: on the device the four integer
curves per candidate, the reference bits and ``pre_r``; on the host the interval table, ``n_iv`` and L; a second
``DescStaging`` (``samp_desc``) beside the plan's ``desc``; and the ``side`` block, first allocated in the middle of a
plan's life.  A call that ran out of order, read a descriptor a later call had overwritten, read a chunk before it
arrived, or worked on a stale side curve would corrupt that append and every append after it: every call of every
sequence is held to tests/sampled_model.py (or tests/progressive_model.py for a prefix slot) at that call's K -- peaks
bit for bit, as ``test_gpu_progressive._check`` does -- with guard bytes around every output, and there is NO host
synchronisation inside a sequence.  tests/test_sampled_model_host.py asserts that every non-empty call of every
sequence changes the reports and that two adjacent calls swapped change them too.

The plug (``test_gpu_streams._plug``) keeps a stream busy, so the call that follows returns while its own descriptor
upload has not executed.  The plug's length is not a pass criterion; the event is: right after the first call behind a
plug returns, the event is still pending (asserted everywhere).  The next call on the same staging waits in
``DescStaging::wait_free`` until the pending upload has left the staging, which ends the window; sequences that need
another window plug the stream again.

What orders what.  ``append_at`` waits on ``samp_desc``, ``append`` on ``desc``, ``open`` on ``desc`` and
``open_sampled`` on both.  In the mixed sequence the prefix call and the sampled call therefore never wait for each
other on the host; on the device ``PlanCore::begin`` alone orders them.  The two calls work on the rows of different
slots, so this sequence does not need ``begin`` to pass (reasoned, and seen once: below): what it holds is that neither
kind of call disturbs the other's rows, descriptors or outputs while both are in flight.  In the sequence with the plan's first
``open_sampled`` behind pending prefix work, the allocation of ``side`` and ``samp_desc`` happens while the prefix
append is pending (asserted right before the call); ``open_sampled`` itself then waits in ``desc.wait_free`` for that
append's upload, as any ``open`` does, so whether the allocation alone would have waited for the device cannot be told
apart there.  It is told apart in the plugged queue and in the late-input sequence, where the plan's FIRST
``open_sampled`` is the first call behind the plug and returns with the plug pending: the allocation does not wait.

PLUG_MS.  Measured with ``measure_call_times`` on one MI355X (gfx950), one process, an idle device, two fresh plans of
three slots one after the other, four calls of each entry on each: the slowest single call on the host took 14.8 ms --
the first ``ProgPlan.open_sampled``, the process's first call into the library, which loads its code object and
allocates ``side`` and ``samp_desc``; the first ``open_sampled`` of the second fresh plan, which only allocates, took
5.4 ms, and no later ``open_sampled`` more than 0.12 ms; the first ``append_at`` took 0.16 ms (0.06 ms on the second
plan) and no later one more than 0.03 ms.  Twenty times 14.8 ms is 296 ms, above the cap of 250 ms that keeps a test at
a few seconds: PLUG_MS = 250, seventeen times the slowest call seen and 46 times the slowest that is not the process's
first.  A plug asked for 250 ms was over 253.2 ms after it was queued, and a plan's first ``open_sampled`` queued behind
it returned after 5.3 ms with the plug's event pending.

Run once against deliberately wrong builds (not kept): with ``plan->begin`` taken out of ``ffs_prog_append_at`` the
two-stream sequence failed with stream B plugged and passed with stream A plugged (there the next call's
``wait_free`` on the one ``samp_desc`` holds the host until the plugged upload has run, which leaves a race the
earlier call usually wins), the mixed sequences passed, as reasoned above, and every test of
tests/test_gpu_sampled.py passed; with the ``ov`` share of ``k_samp_counts`` off by one at every lag above e = 4097 the
2W = 8192, limit and three-window cases of tests/test_gpu_sampled.py failed and its earlier cases passed.
Needs a real MI355X.
"""
import time

import numpy as np
import pytest

import progressive_model as pm
import sampled_cases as sc
import sampled_model as sm
from test_gpu_progressive import Cands, Outputs, _check, _dev, _open, _words
from test_gpu_sampled import _open_sampled
from test_gpu_streams import _cycles_per_ms, _plug

pytestmark = pytest.mark.gpu

SLOWEST_CALL_MS = 14.8  # measured, see the module docstring
PLUG_MS = min(20 * SLOWEST_CALL_MS, 250.0)
TOP_K, E = 3, 40


def _torch():
    import torch

    return torch


def _ready():
    """Before a sequence: everything uploaded, the outputs filled, nothing pending."""
    _cycles_per_ms()
    _torch().cuda.synchronize()


def _pending(event, what):
    assert not event.query(), ("%s returned after the plug of %.0f ms had finished: it waited for the stream, or its upload "
                               "was not pending when the next call started" % (what, PLUG_MS))


class Feed:
    """The chunk words of one call, one buffer per slot, every bit outside the chunk set.  ``late``: the buffers the call
    reads hold 0xFF until ``arrive`` copies the staged words in."""

    def __init__(self, chunks, first_bit, late=False):
        torch = _torch()
        self.chunks, self.first_bit = chunks, int(first_bit)
        self.staged = [_dev(_words(ch, self.first_bit)) for ch in chunks]
        self.real = [torch.full_like(t, -1) for t in self.staged] if late else self.staged

    def arrive(self):
        """(on the current stream)"""
        for dst, src in zip(self.real, self.staged):
            dst.copy_(src, non_blocking=True)

    def poison(self):
        """(on the current stream, right behind the call that reads the words)"""
        for t in self.real:
            t.fill_(0x55555555)


class AppendAt:
    """One ``append_at`` call of a sequence: its slots, its segments, its words and its own guarded outputs."""

    def __init__(self, slots, segs, chunks, first_bit, max_cand, late=False):
        self.slots, self.segs, self.feed = [int(s) for s in slots], [(int(a), int(n)) for a, n in segs], Feed(chunks, first_bit, late)
        self.out = Outputs(len(self.slots), max_cand)

    def issue(self, plan):
        """(on the current stream)"""
        plan.append_at(self.slots, [t.data_ptr() for t in self.feed.real], [self.feed.first_bit] * len(self.slots),
                       [a for a, _ in self.segs], [n for _, n in self.segs], TOP_K, E, *self.out.views())

    def check(self, models, n_cands, where):
        """After the sequence's one synchronisation, in call order: ``models[slot]`` is at this call's K."""
        recs, states = self.out.read()  # (asserts the guard bytes)
        for i, s in enumerate(self.slots):
            reps, mstate = models[s].append_at(self.segs[i][0], self.feed.chunks[i], TOP_K, E)
            _check(recs[i], states[i], reps, mstate, n_cands[s], TOP_K, (where, "slot", s, self.segs[i]))


class Append:
    """One prefix ``append`` call of a sequence (tests/test_gpu_progressive_streams.py's, one slot)."""

    def __init__(self, slot, chunk, first_bit, max_cand):
        self.slot, self.feed, self.out = int(slot), Feed([chunk], first_bit), Outputs(1, max_cand)

    def issue(self, plan):
        plan.append([self.slot], [self.feed.real[0].data_ptr()], [self.feed.first_bit], [self.feed.chunks[0].size], TOP_K, E,
                    *self.out.views())

    def check(self, model, n_cand, where):
        recs, states = self.out.read()
        reps, mstate = model.append(self.feed.chunks[0], TOP_K, E)
        _check(recs[0], states[0], reps, mstate, n_cand, TOP_K, where)


def _sequence(case_of_slot, calls, max_cand, late=False):
    """AppendAt objects for ``calls`` = [(slots, (a, n) per slot, first_bit)]: slot s is fed from ``case_of_slot[s]``."""
    out = []
    for slots, segs, fb in calls:
        chunks = [case_of_slot[s]["ref"][a:a + n] for s, (a, n) in zip(slots, segs)]
        assert all(ch.size == n for ch, (_, n) in zip(chunks, segs))
        out.append(AppendAt(slots, segs, chunks, fb, max_cand, late))
    return out


def _one_slot(case, segs, max_cand, late=False, slot=0):
    return _sequence({slot: case}, [([slot], [seg], (5 * k + 1) % 32) for k, seg in enumerate(segs)], max_cand, late)


def _prefix_sequence(case, lengths, max_cand, slot=0):
    out, o = [], 0
    for k, n in enumerate(lengths):
        out.append(Append(slot, case["ref"][o:o + n], (7 * k + 3) % 32, max_cand))
        o += n
    return out


def _model(case):
    return sm.Slot(case["cands"], case["ref_levels"], case["W"], case["T"])


def _prefix_model(case):
    return pm.Slot(case["cands"], case["ref_levels"], case["W"])


def _plan(cases, n_slots=None):
    from ffsubsync_amd import _native

    return _native.ProgPlan(n_slots or len(cases), max(len(k["cands"]) for k in cases), 2 * max(k["W"] for k in cases),
                            max(k.get("T", k["ref"].size) for k in cases), max(len(s) for k in cases for s, _ in k["cands"]))


def _known(plan, slot):
    return [tuple(int(v) for v in x) for x in plan.known(slot)]


# ---- 1: a plugged queue, known() beside it and reference() behind it ---------------------------------------------------
@pytest.fixture(scope="module")
def queued():
    """The plan's first ``open_sampled`` (three slots) and the eight calls of ``sc.QUEUE_CALLS`` queued on one plugged
    stream, every chunk overwritten right behind its call and the candidates right behind the open; a second plug in
    front of the fifth call opens the window between two appends.  ``known`` of every slot is read after every call,
    and the words at ``reference(slot)`` are cloned on that same stream behind the last call."""
    torch = _torch()
    from ffsubsync_amd.progressive import _DeviceWords

    cases = sc.queue_cases()
    plan = _plan(cases)
    cands = Cands(cases)
    calls = _sequence(dict(enumerate(cases)), sc.QUEUE_CALLS, plan.max_cand)
    s = torch.cuda.Stream()
    pending, refs, known = [], [], []
    try:
        _ready()
        event = _plug(s, PLUG_MS)
        with torch.cuda.stream(s):
            _open_sampled(plan, [2, 0, 1], cases, cands, rows=[2, 0, 1])
            pending.append(("open_sampled", event.query()))
            known.append([_known(plan, i) for i in range(3)])
            cands.data.fill_(-1)
            for k, call in enumerate(calls):
                if k == 4:
                    event = _plug(s, PLUG_MS)
                call.issue(plan)
                if k == 4:
                    pending.append(("the fifth append_at", event.query()))
                known.append([_known(plan, i) for i in range(3)])
                call.feed.poison()
            for slot in range(3):
                ptr, n = plan.reference(slot)
                refs.append((n, torch.as_tensor(_DeviceWords(ptr, n // 32 + 2), device="cuda").clone()))
        torch.cuda.synchronize()
    finally:
        plan.close()
    return dict(cases=cases, calls=calls, pending=pending, known=known,
                refs=[(n, t.cpu().numpy().view(np.uint32)) for n, t in refs])


def test_open_sampled_and_eight_calls_queued_on_a_plugged_stream(queued):
    for what, done in queued["pending"]:
        assert not done, "%s returned after its plug had finished: the hazard window was not open" % what
    models = [_model(k) for k in queued["cases"]]
    assert queued["known"][0] == [[], [], []]
    for k, call in enumerate(queued["calls"]):
        call.check(models, [len(c["cands"]) for c in queued["cases"]], ("queued call", k))
        assert queued["known"][k + 1] == [m.intervals for m in models], ("known() after call", k)  # host state, in call order


def test_reference_behind_the_queued_calls(queued):
    """A read of ``reference(slot)`` ordered behind the last call's stream sees the known bits, and zeros elsewhere --
    beyond T included."""
    for slot, (n, words) in enumerate(queued["refs"]):
        case = queued["cases"][slot]
        bits = np.zeros(32 * words.size, bool)
        for call in queued["calls"]:
            for s, (a, m), ch in zip(call.slots, call.segs, call.feed.chunks):
                if s == slot:
                    bits[a:a + m] = ch
        assert n == case["T"] and bits.any() and 32 * words.size > n
        assert np.array_equal(words, _words(bits, fill=False)), (slot, n)


# ---- 2: two streams, one sampled slot ----------------------------------------------------------------------------------
@pytest.mark.parametrize("plugged", ["A", "B"])
def test_two_streams_feed_one_sampled_slot_in_call_order(plugged):
    """Ten segments of one slot, alternating between two streams with nothing but the plan's ``done`` event between
    them; one of the streams is plugged.  Record k must be the model's after k calls in call order."""
    torch = _torch()
    case = sc.two_stream_case()
    plan = _plan([case])
    cands = Cands([case])
    calls = _one_slot(case, sc.TWO_STREAM_SEGMENTS, plan.max_cand)
    streams = dict(A=torch.cuda.Stream(), B=torch.cuda.Stream())
    first = 0 if plugged == "A" else 1  # the first call behind the plug
    try:
        with torch.cuda.stream(streams["A"]):
            _open_sampled(plan, [0], [case], cands)
        _ready()
        event = _plug(streams[plugged], PLUG_MS)
        for k, call in enumerate(calls):
            with torch.cuda.stream(streams["AB"[k % 2]]):
                call.issue(plan)
                if k == first:
                    _pending(event, "append_at %d" % k)
                call.feed.poison()
        torch.cuda.synchronize()
        model = [_model(case)]
        for k, call in enumerate(calls):
            call.check(model, [2], ("plugged", plugged, "append_at", k))
        assert _known(plan, 0) == model[0].intervals
    finally:
        plan.close()


# ---- 3: a prefix slot and a sampled slot of one plan at work at the same time ------------------------------------------
@pytest.mark.parametrize("plugged", ["A", "B"])
def test_a_prefix_slot_and_a_sampled_slot_alternate_on_two_streams(plugged):
    """Slot 0 a prefix slot fed by ``append`` on stream A, slot 1 a sampled slot fed by ``append_at`` on stream B, six
    calls each in turn.  The two calls wait on different stagings, so neither waits for the other on the host; both
    slots are held to their models at every call."""
    torch = _torch()
    prefix, sampled = sc.mixed_case()
    plan = _plan([prefix, sampled])
    cands = Cands([prefix, sampled])
    a_calls = _prefix_sequence(prefix, sc.MIXED_LENGTHS, plan.max_cand, slot=0)
    b_calls = _one_slot(sampled, sc.MIXED_SEGMENTS, plan.max_cand, slot=1)
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        with torch.cuda.stream(A):
            _open(plan, [0], [prefix, sampled], cands, rows=[0])
            _open_sampled(plan, [1], [prefix, sampled], cands, rows=[1])
        _ready()
        event = _plug(A if plugged == "A" else B, PLUG_MS)
        for k, (pa, sb) in enumerate(zip(a_calls, b_calls)):
            with torch.cuda.stream(A):
                pa.issue(plan)
                if k == 0 and plugged == "A":
                    _pending(event, "append")
                pa.feed.poison()
            with torch.cuda.stream(B):
                sb.issue(plan)
                if k == 0:  # (A plugged: the sampled call waited for nothing either -- the append's staging is not its own)
                    _pending(event, "append_at")
                sb.feed.poison()
        torch.cuda.synchronize()
        pmodel, smodel = _prefix_model(prefix), {1: _model(sampled)}
        for k, (pa, sb) in enumerate(zip(a_calls, b_calls)):
            pa.check(pmodel, 2, ("plugged", plugged, "append", k))
            sb.check(smodel, {1: 2}, ("plugged", plugged, "append_at", k))
    finally:
        plan.close()


# ---- 4: the plan's first open_sampled with prefix work pending ---------------------------------------------------------
def test_the_first_open_sampled_of_a_plan_with_prefix_appends_pending():
    """A fresh plan: prefix appends on slot 0 behind a plug, then the plan's first ``open_sampled`` (slot 1), which
    allocates ``side`` and ``samp_desc`` while they are pending, and ``append_at`` calls behind a second plug, the prefix
    slot going on beside them."""
    torch = _torch()
    prefix, sampled = sc.mixed_case()
    plan = _plan([prefix, sampled])
    cands = Cands([prefix, sampled])
    a_calls = _prefix_sequence(prefix, sc.MIXED_LENGTHS, plan.max_cand, slot=0)
    b_calls = _one_slot(sampled, sc.MIXED_SEGMENTS, plan.max_cand, slot=1)
    s = torch.cuda.Stream()
    try:
        assert plan.sampled_bytes() == 0
        with torch.cuda.stream(s):
            _open(plan, [0], [prefix, sampled], cands, rows=[0])
        _ready()
        event = _plug(s, PLUG_MS)
        with torch.cuda.stream(s):
            a_calls[0].issue(plan)
            _pending(event, "append")
            a_calls[0].feed.poison()
            _open_sampled(plan, [1], [prefix, sampled], cands, rows=[1])  # (allocates; then waits for the append's upload)
            assert plan.sampled_bytes() > 0 and _known(plan, 1) == []
            a_calls[1].issue(plan)
            a_calls[1].feed.poison()
            event = _plug(s, PLUG_MS)
            b_calls[0].issue(plan)
            _pending(event, "the first append_at")
            b_calls[0].feed.poison()
            for pa, sb in zip(a_calls[2:], b_calls[1:]):
                pa.issue(plan)
                pa.feed.poison()
                sb.issue(plan)
                sb.feed.poison()
            b_calls[5].issue(plan)
            b_calls[5].feed.poison()
        torch.cuda.synchronize()
        pmodel, smodel = _prefix_model(prefix), {1: _model(sampled)}
        for k, pa in enumerate(a_calls):
            pa.check(pmodel, 2, ("append", k))
        for k, sb in enumerate(b_calls):
            sb.check(smodel, {1: 2}, ("append_at", k))
    finally:
        plan.close()


# ---- 5: close_slots and reopen with an append_at pending ---------------------------------------------------------------
def test_a_slot_reopened_along_the_chain_while_its_last_call_is_pending():
    """Slot 0 goes sampled -> prefix -> sampled -> sampled (a shorter T, a smaller W, fewer candidates); every reopen is
    queued behind a plugged call of the old problem.  Stale ``side`` rows, interval entries, reference bits or curves
    of the old problem would show in the first records after the reopen; ``known`` is empty right after each."""
    torch = _torch()
    chain = sc.reopen_chain()
    cases = [case for _, case, _ in chain]
    plan = _plan(cases, n_slots=1)
    cands = Cands(cases)
    mc = plan.max_cand
    stages = []
    for row, (kind, case, appends) in enumerate(chain):
        calls = _one_slot(case, appends, mc) if kind == "sampled" else _prefix_sequence(case, appends, mc)
        stages.append((row, kind, case, calls))
    s = torch.cuda.Stream()
    try:
        _ready()
        with torch.cuda.stream(s):
            for row, kind, case, calls in stages:
                if row:
                    plan.close_slots([0])
                    _pending(event, "close_slots")  # (host state only: it does not wait)
                if kind == "sampled":
                    _open_sampled(plan, [0], cases, cands, rows=[row])
                    assert _known(plan, 0) == [], row
                else:
                    _open(plan, [0], cases, cands, rows=[row])
                for call in calls[:-1]:
                    call.issue(plan)
                    call.feed.poison()
                event = _plug(s, PLUG_MS)  # this problem's last call stays pending behind it
                calls[-1].issue(plan)
                _pending(event, "the last %s call of problem %d" % (kind, row))
                calls[-1].feed.poison()
        torch.cuda.synchronize()
        for row, kind, case, calls in stages:
            model = {0: _model(case)} if kind == "sampled" else _prefix_model(case)
            for k, call in enumerate(calls):
                if kind == "sampled":
                    call.check(model, {0: len(case["cands"])}, ("problem", row, "call", k))
                else:
                    call.check(model, len(case["cands"]), ("problem", row, "call", k))
        assert _known(plan, 0) == model[0].intervals
    finally:
        plan.close()


# ---- 6: destroy waits --------------------------------------------------------------------------------------------------
def test_destroy_waits_for_the_pending_append_at():
    """open_sampled and a call behind a plug on one stream, a second call behind a plug on another (it returns while
    that plug is pending), then the destroy at once: it returns only after both plugs, and the outputs equal the model."""
    torch = _torch()
    case = sc.two_stream_case()
    plan = _plan([case])
    cands = Cands([case])
    calls = _one_slot(case, sc.TWO_STREAM_SEGMENTS[:2], plan.max_cand)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        _ready()
        event_a = _plug(a, PLUG_MS)
        with torch.cuda.stream(a):
            _open_sampled(plan, [0], [case], cands)
            _pending(event_a, "open_sampled")
            calls[0].issue(plan)
        event_b = _plug(b, PLUG_MS)
        with torch.cuda.stream(b):
            calls[1].issue(plan)
            _pending(event_b, "the last append_at")
    finally:
        plan.close()
    assert plan.handle is None and event_a.query() and event_b.query(), "the destroy returned while a call was pending"
    torch.cuda.synchronize()
    model = [_model(case)]
    for k, call in enumerate(calls):
        call.check(model, [2], ("destroyed behind append_at", k))  # (asserts the guard bytes)


# ---- 7: late inputs ----------------------------------------------------------------------------------------------------
def test_late_candidates_and_chunks():
    """The candidate words and every chunk hold 0xFF until a copy queued ahead of the call brings the real bytes: on
    the call's own stream behind the plug, and for one call on a second plugged stream with an event between the copy
    and the call.  A kernel or copy sent to any other stream, or a host read of the inputs, would see the poison."""
    torch = _torch()
    case, segs = sc.late_case()
    plan = _plan([case])
    cands = Cands([case])
    cands.data.fill_(-1)
    calls = _one_slot(case, segs, plan.max_cand, late=True)
    s, other = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        _ready()
        event = _plug(s, PLUG_MS)
        with torch.cuda.stream(s):
            cands.data.copy_(cands.clone, non_blocking=True)
            _open_sampled(plan, [0], [case], cands)
            _pending(event, "open_sampled")
            for k, call in enumerate(calls):
                if k == 2:  # the copy on another stream, behind a plug of its own; an event orders the call behind it
                    arrived = torch.cuda.Event()
                    event = _plug(other, PLUG_MS)
                    with torch.cuda.stream(other):
                        call.feed.arrive()
                        arrived.record()
                    s.wait_event(arrived)
                else:
                    call.feed.arrive()
                call.issue(plan)
                if k == 2:
                    _pending(event, "the append_at behind the other stream's copy")
        torch.cuda.synchronize()
        model = [_model(case)]
        for k, call in enumerate(calls):
            call.check(model, [3], ("late append_at", k))
            assert all(bool((r == st).all()) for r, st in zip(call.feed.real, call.feed.staged)), "the chunk was written"
        assert bool((cands.data == cands.clone).all()), "the candidates were written"
    finally:
        plan.close()


# ---- the measurement behind PLUG_MS ------------------------------------------------------------------------------------
def measure_call_times(repeats=3):
    """[{entry: (host ms of the first call on a fresh plan, of the slowest later call)}, the same for a second fresh
    plan] of ``ProgPlan.open_sampled`` and ``ProgPlan.append_at`` on an idle device: the figures SLOWEST_CALL_MS is taken
    from (run from a script; no test calls this)."""
    torch = _torch()
    cases = sc.queue_cases()
    out = []
    for _ in range(2):
        plan = _plan(cases)
        cands = Cands(cases)
        segs = [(100 * k, 33) for k in range(repeats + 1)]
        calls = _sequence(dict(enumerate(cases)), [([0, 1, 2], [seg] * 3, 1) for seg in segs], plan.max_cand)
        s = torch.cuda.Stream()
        times = dict(open_sampled=[], append_at=[])
        try:
            with torch.cuda.stream(s):
                for _ in range(repeats + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    _open_sampled(plan, [0, 1, 2], cases, cands)
                    times["open_sampled"].append(1e3 * (time.perf_counter() - t0))
                for call in calls:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call.issue(plan)
                    times["append_at"].append(1e3 * (time.perf_counter() - t0))
            torch.cuda.synchronize()
            models = [_model(k) for k in cases]
            for k, call in enumerate(calls):
                call.check(models, [len(c["cands"]) for c in cases], ("timed append_at", k))
        finally:
            plan.close()
        out.append({name: (t[0], max(t[1:])) for name, t in times.items()})
    return out
