"""The progressive plan (``ffs_prog_plan``) and ``ffs_sweep_peaks`` under queued calls, side streams and late
inputs, the way tests/test_gpu_streams.py holds the other side plans.  ``ProgPlan`` is the one plan that carries
answers from call to call: L per slot on the host; the reference bits, the prefix popcounts and the integer curves on
the device.  One ``DescStaging`` is filled as ``ProgOpenDesc[]`` by ``open`` and as ``ProgSlotDesc[]`` + ``QualDesc[]``
by ``append``, ``PlanCore::begin`` alone orders calls across streams, ``close_slots`` never touches the device and the
destroy promises to wait.  A call that ran out of order, read a descriptor a later call had overwritten, or read a chunk
before it arrived would corrupt that append and every append after it: every call of every sequence is held to
tests/progressive_model.py at that call's L (peaks bit for bit, as ``test_gpu_progressive._check`` does), with guard
bytes around every output, and there is NO host synchronisation inside a sequence.

The plug (``test_gpu_streams._plug``: ``torch.cuda._sleep`` and an event behind it) keeps a stream busy, so the call
that follows returns while its own descriptor upload has not executed.  The plug's length is not a pass criterion.
What proves the window open is the event: right after the first call behind a plug returns, the event is still pending
(asserted everywhere) -- neither ``open`` nor ``append`` waits for the stream.  The call after that one waits in
``DescStaging::wait_free`` until the pending upload has left the staging, which ends the window; sequences that need a
second window (append after append, ``close_slots`` with an append pending) plug the stream a second time.

PLUG_MS.  Measured with ``measure_call_times`` on one MI355X (gfx950), one process, an idle device, a fresh plan of
three slots, four calls each: the slowest single call on the host took 14.6 ms -- the first ``ProgPlan.open``, the
process's first call into the library, which loads its code object (5.5 ms for the first ``open`` of a second fresh
plan in the same process); no later ``open`` took more than 0.12 ms, the first ``append`` 0.15 ms and no later one more
than 0.03 ms.  Twenty times 14.6 ms is 292 ms, above the cap of 250 ms that keeps a test at a few seconds:
PLUG_MS = 250, seventeen times the slowest call seen and 1700 times the slowest that is not a plan's first ``open``.
A plug asked for 250 ms took 248.7 ms.  Needs a real MI355X.
"""
import time

import numpy as np
import pytest

import progressive_cases as pc
import progressive_model as pm
import sweep_model as sm
from test_gpu_progressive import GUARD, Cands, Outputs, _check, _dev, _open, _words
from test_gpu_streams import _cycles_per_ms, _plug

pytestmark = pytest.mark.gpu

SLOWEST_CALL_MS = 14.6  # measured, see the module docstring
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
    """The chunk words of one append call, one buffer per slot, every bit outside the chunk set.  ``late``: the buffers
    the call reads hold 0xFF until ``arrive`` copies the staged words in."""

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


class Append:
    """One append call of a sequence: its slots, its words and its own guarded outputs."""

    def __init__(self, slots, chunks, first_bit, max_cand, late=False):
        self.slots, self.feed = [int(s) for s in slots], Feed(chunks, first_bit, late)
        self.out = Outputs(len(self.slots), max_cand)

    def issue(self, plan):
        """(on the current stream)"""
        plan.append(self.slots, [t.data_ptr() for t in self.feed.real], [self.feed.first_bit] * len(self.slots),
                    [ch.size for ch in self.feed.chunks], TOP_K, E, *self.out.views())

    def check(self, models, n_cands, where):
        """After the sequence's one synchronisation, in call order: ``models[slot]`` is at this call's L."""
        recs, states = self.out.read()  # (asserts the guard bytes)
        for i, s in enumerate(self.slots):
            reps, mstate = models[s].append(self.feed.chunks[i], TOP_K, E)
            _check(recs[i], states[i], reps, mstate, n_cands[s], TOP_K, (where, "slot", s))


def _sequence(case_of_slot, calls, max_cand, late=False, pos=None):
    """Append objects for ``calls`` = [(slots, n_new per slot, first_bit)]: slot s is fed from ``case_of_slot[s]`` in
    order, from sample ``pos[s]`` on (0 where not given; ``pos`` is advanced)."""
    pos = {} if pos is None else pos
    for s in case_of_slot:
        pos.setdefault(s, 0)
    out = []
    for slots, ns, fb in calls:
        chunks = []
        for s, n in zip(slots, ns):
            ref = case_of_slot[s]["ref"]
            assert pos[s] + n <= ref.size
            chunks.append(ref[pos[s]:pos[s] + n])
            pos[s] += n
        out.append(Append(slots, chunks, fb, max_cand, late))
    return out


def _model(case):
    return pm.Slot(case["cands"], case["ref_levels"], case["W"])


# ---- 1 and 6: a plugged queue, and reference() behind it ---------------------------------------------------------------
@pytest.fixture(scope="module")
def queued():
    """open of three slots and the eight appends of ``pc.QUEUE_CALLS`` queued on one plugged stream, every chunk
    overwritten right behind its call and the candidates right behind ``open``; a second plug in front of the fifth
    append opens the window between two appends.  Then the words at ``reference(slot)`` cloned on that same stream."""
    torch = _torch()
    from ffsubsync_amd import _native
    from ffsubsync_amd.progressive import _DeviceWords

    cases = pc.queue_cases()
    plan = _native.ProgPlan(3, 3, 1200, 1000, 5000)
    cands = Cands(cases)
    calls = _sequence(dict(enumerate(cases)), pc.QUEUE_CALLS, 3)
    s = torch.cuda.Stream()
    pending, refs = [], []
    try:
        _ready()
        event = _plug(s, PLUG_MS)
        with torch.cuda.stream(s):
            _open(plan, [2, 0, 1], cases, cands, rows=[2, 0, 1])
            pending.append(("open", event.query()))
            cands.data.fill_(-1)
            for k, call in enumerate(calls):
                if k == 4:
                    event = _plug(s, PLUG_MS)
                call.issue(plan)
                if k == 4:
                    pending.append(("the fifth append", event.query()))
                call.feed.poison()
            for slot in range(3):
                ptr, n = plan.reference(slot)
                refs.append((n, torch.as_tensor(_DeviceWords(ptr, n // 32 + 2), device="cuda").clone()))
        torch.cuda.synchronize()
    finally:
        plan.close()
    return dict(cases=cases, calls=calls, pending=pending, refs=[(n, t.cpu().numpy().view(np.uint32)) for n, t in refs])


def test_open_and_eight_appends_queued_on_a_plugged_stream(queued):
    for what, done in queued["pending"]:
        assert not done, "%s returned after its plug had finished: the hazard window was not open" % what
    models = [_model(k) for k in queued["cases"]]
    for k, call in enumerate(queued["calls"]):
        call.check(models, [len(c["cands"]) for c in queued["cases"]], ("queued call", k))


def test_reference_behind_the_queued_appends(queued):
    """A read of ``reference(slot)`` ordered behind the last append's stream sees the bits fed, and zeros from L on."""
    fed = [[], [], []]
    for call in queued["calls"]:
        for s, ch in zip(call.slots, call.feed.chunks):
            fed[s].append(ch)
    for slot, (n, words) in enumerate(queued["refs"]):
        bits = np.concatenate(fed[slot])
        assert n == bits.size > 0
        want = _words(bits, fill=False)
        want = np.concatenate([want, np.zeros(words.size - want.size, np.uint32)])
        assert np.array_equal(words, want), (slot, n)


# ---- 2: two streams, one slot ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plugged", ["A", "B"])
def test_two_streams_feed_one_slot_in_call_order(plugged):
    """Ten appends to one slot, alternating between two streams with nothing but the plan's ``done`` event between
    them; one of the streams is plugged.  Record k must be the model's after k appends in call order
    (tests/test_progressive_model_host.py: every append changes the answer, and so would a swapped pair)."""
    torch = _torch()
    from ffsubsync_amd import _native

    case = pc.two_stream_case()
    plan = _native.ProgPlan(1, 2, 1200, 700, 700)
    cands = Cands([case])
    calls = _sequence({0: case}, [([0], [n], (5 * k + 1) % 32) for k, n in enumerate(pc.TWO_STREAM_LENGTHS)], 2)
    streams = dict(A=torch.cuda.Stream(), B=torch.cuda.Stream())
    first = 0 if plugged == "A" else 1  # the first call behind the plug
    try:
        with torch.cuda.stream(streams["A"]):
            _open(plan, [0], [case], cands)
        _ready()
        event = _plug(streams[plugged], PLUG_MS)
        for k, call in enumerate(calls):
            with torch.cuda.stream(streams["AB"[k % 2]]):
                call.issue(plan)
                if k == first:
                    _pending(event, "append %d" % k)
                call.feed.poison()
        torch.cuda.synchronize()
        model = [_model(case)]
        for k, call in enumerate(calls):
            call.check(model, [2], ("plugged", plugged, "append", k))
    finally:
        plan.close()


# ---- 3: close and reopen while work is pending -------------------------------------------------------------------------
def test_close_and_reopen_while_work_is_pending():
    """Slot 1 is opened on a long problem (S = 5000, W = 600), fed twice, closed and reopened on a short one (S = 33,
    W = 16) while the first problem's last append is pending, and fed three times; its neighbour slot 0 goes on appending.
    Stale curve words, prefix sums or reference bits of the first problem would show in the reopened slot's records."""
    torch = _torch()
    from ffsubsync_amd import _native

    long, short, neighbour = cases = pc.reopen_cases()
    plan = _native.ProgPlan(2, 2, 1200, 700, 5000)
    cands = Cands(cases)
    pos = {}
    before = _sequence({1: long, 0: neighbour}, [([1, 0], [200, 65], 3), ([1], [33], 31)], 2, pos=pos)
    pos[1] = 0  # slot 1 starts again; the neighbour's position runs on
    after = _sequence({1: short, 0: neighbour}, [([0], [31], 0), ([0, 1], [1, 65], 9), ([1], [32], 1), ([1, 0], [100, 200], 20),
                                                 ([0], [0], 7)], 2, pos=pos)
    s = torch.cuda.Stream()
    try:
        _ready()
        event = _plug(s, PLUG_MS)
        with torch.cuda.stream(s):
            _open(plan, [1, 0], cases, cands, rows=[0, 2])
            _pending(event, "open")
            before[0].issue(plan)
            before[0].feed.poison()
            event = _plug(s, PLUG_MS)  # the long problem's second append stays pending behind it
            before[1].issue(plan)
            _pending(event, "the second append")
            before[1].feed.poison()
            plan.close_slots([1])
            _pending(event, "close_slots")  # (host state only: it does not wait)
            _open(plan, [1], cases, cands, rows=[1])  # (waits for the pending upload to leave the staging, no longer)
            for call in after:
                call.issue(plan)
                call.feed.poison()
        torch.cuda.synchronize()
        models = {1: _model(long), 0: _model(neighbour)}
        for k, call in enumerate(before):
            call.check(models, {1: 1, 0: 2}, ("before the reopen", k))
        models[1] = _model(short)
        for k, call in enumerate(after):
            call.check(models, {1: 1, 0: 2}, ("after the reopen", k))
    finally:
        plan.close()


# ---- 4: destroy waits --------------------------------------------------------------------------------------------------
def test_destroy_waits_for_the_pending_appends():
    """open and an append behind a plug on one stream, a second append behind a plug on another (it returns while that
    plug is pending), then the destroy at once: it returns only after both plugs, and the outputs equal the model."""
    torch = _torch()
    from ffsubsync_amd import _native

    case = pc.queue_cases()[0]
    plan = _native.ProgPlan(1, 2, 1200, 700, 700)
    cands = Cands([case])
    calls = _sequence({0: case}, [([0], [200], 8), ([0], [65], 31)], 2)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        _ready()
        event_a = _plug(a, PLUG_MS)
        with torch.cuda.stream(a):
            _open(plan, [0], [case], cands)
            _pending(event_a, "open")
            calls[0].issue(plan)
        event_b = _plug(b, PLUG_MS)
        with torch.cuda.stream(b):
            calls[1].issue(plan)
            _pending(event_b, "the last append")
    finally:
        plan.close()
    assert plan.handle is None and event_a.query() and event_b.query(), "the destroy returned while an append was pending"
    torch.cuda.synchronize()
    model = [_model(case)]
    for k, call in enumerate(calls):
        call.check(model, [2], ("destroyed behind append", k))


# ---- 5: late inputs ----------------------------------------------------------------------------------------------------
def test_late_candidates_and_chunks():
    """The candidate words and every chunk hold 0xFF until a copy queued ahead of the call brings the real bytes: on
    the call's own stream behind the plug, and for one append on a second plugged stream with an event between the copy
    and the call.  A kernel or copy sent to any other stream, or a host read of the inputs, would see the poison."""
    torch = _torch()
    from ffsubsync_amd import _native

    case = pc.queue_cases()[2]
    plan = _native.ProgPlan(1, 3, 32, 1000, 700)
    cands = Cands([case])
    cands.data.fill_(-1)
    calls = _sequence({0: case}, [([0], [200], 1), ([0], [33], 31), ([0], [65], 8), ([0], [0], 2), ([0], [31], 0)], 3, late=True)
    s, other = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        _ready()
        event = _plug(s, PLUG_MS)
        with torch.cuda.stream(s):
            cands.data.copy_(cands.clone, non_blocking=True)
            _open(plan, [0], [case], cands)
            _pending(event, "open")
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
                    _pending(event, "the append behind the other stream's copy")
        torch.cuda.synchronize()
        model = [_model(case)]
        for k, call in enumerate(calls):
            call.check(model, [3], ("late append", k))
            assert all(bool((r == st).all()) for r, st in zip(call.feed.real, call.feed.staged)), "the chunk was written"
        assert bool((cands.data == cands.clone).all()), "the candidates were written"
    finally:
        plan.close()


# ---- 7: ffs_sweep_peaks queued -----------------------------------------------------------------------------------------
def _check_profile(g, rec, top_k, exclusion, where):
    """tests/test_gpu_ratio_sweep.py's comparison of one profile with ``sweep_model.report``."""
    want = sm.report(rec["score"], rec["offset"], rec["flags"], top_k, exclusion)
    n = len(want["peaks"])
    assert int(g["n_peaks"]) == n, where
    assert g["peak_score"][:n].tobytes() == np.array([p[0] for p in want["peaks"]], np.float64).tobytes(), where
    assert list(g["peak_offset"][:n]) == [p[1] for p in want["peaks"]], where
    assert list(g["peak_index"][:n]) == [p[2] for p in want["peaks"]], where
    assert not g["peak_score"][n:].any() and not g["peak_offset"][n:].any() and not g["peak_index"][n:].any(), where
    assert (int(g["n_points"]), int(g["n_skipped"]), int(g["flags"])) == (rec.size, want["n_skipped"], want["flags"]), where
    assert float(g["mean"]) == pytest.approx(want["mean"], rel=1e-9, abs=0), where
    assert float(g["std"]) == pytest.approx(want["std"], rel=1e-9, abs=0), where
    if want["flags"] & sm.FLAT:
        assert float(g["std"]) == 0.0 and float(g["mean"]) == want["mean"], where


def test_two_sweep_reductions_queued_behind_a_late_table():
    """``ffs_sweep_peaks`` has no plan: all it may rely on is the stream.  The record table and the file offsets arrive
    on the stream behind a plug (until then they hold 0xFF), and two calls with different ``top_k`` and ``exclusion``
    follow back to back into their own guarded outputs."""
    torch = _torch()
    from ffsubsync_amd import _native
    from test_gpu_ratio_sweep import _tables, _upload

    files = _tables()[:4]
    table, first = _upload(files)
    first_dev = torch.from_numpy(first).cuda()
    late_table, late_first = torch.full_like(table, 0xFF), torch.full_like(first_dev, -1)
    params = [(1, 4), (8, 1)]
    nbytes = len(files) * _native.SWEEP_PROFILE_BYTES
    outs = [torch.full((2 * GUARD + nbytes,), 0xA5, dtype=torch.uint8, device="cuda") for _ in params]
    s = torch.cuda.Stream()
    _ready()
    event = _plug(s, PLUG_MS)
    with torch.cuda.stream(s):
        late_table.copy_(table, non_blocking=True)
        late_first.copy_(first_dev, non_blocking=True)
        for k, ((top_k, exclusion), out) in enumerate(zip(params, outs)):
            _native.sweep_peaks(late_table, late_first, len(files), top_k, exclusion, out=out[GUARD:GUARD + nbytes])
            if k == 0:
                _pending(event, "ffs_sweep_peaks")
    torch.cuda.synchronize()
    assert bool((late_table == table).all()) and bool((late_first == first_dev).all())  # records are read, never written
    for (top_k, exclusion), out in zip(params, outs):
        raw = out.cpu().numpy()
        assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all(), "guard bytes written"
        got = raw[GUARD:-GUARD].view(_native.SWEEP_PROFILE_DTYPE)
        for f, rec in enumerate(files):
            _check_profile(got[f], rec, top_k, exclusion, ("top_k", top_k, "exclusion", exclusion, "file", f))


# ---- the measurement behind PLUG_MS ------------------------------------------------------------------------------------
def measure_call_times(repeats=3):
    """{entry: (host ms of the first call on a fresh plan, of the slowest later call)} of ``ProgPlan.open`` and
    ``ProgPlan.append`` on an idle device, as ``test_gpu_streams.measure_call_times`` takes them: the figures
    SLOWEST_CALL_MS is taken from (run from a script; no test calls this)."""
    torch = _torch()
    from ffsubsync_amd import _native

    cases = pc.queue_cases()
    plan = _native.ProgPlan(3, 3, 1200, 1000, 5000)
    cands = Cands(cases)
    calls = _sequence(dict(enumerate(cases)), [([0, 1, 2], [33, 33, 33], 1)] * (repeats + 1), 3)
    s = torch.cuda.Stream()
    times = dict(open=[], append=[])
    try:
        with torch.cuda.stream(s):
            for _ in range(repeats + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _open(plan, [0, 1, 2], cases, cands)
                times["open"].append(1e3 * (time.perf_counter() - t0))
            for call in calls:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call.issue(plan)
                times["append"].append(1e3 * (time.perf_counter() - t0))
        torch.cuda.synchronize()
        models = [_model(k) for k in cases]
        for k, call in enumerate(calls):
            call.check(models, [len(c["cands"]) for c in cases], ("timed append", k))
    finally:
        plan.close()
    return {name: (t[0], max(t[1:])) for name, t in times.items()}
