"""The side plans under queued calls, side streams and late inputs: the 16 batch entry points of ``ffs_split_plan``,
``ffs_quality_plan``, ``ffs_match_plan``, ``ffs_split_range_plan``, ``ffs_drift_plan`` and ``ffs_drift_range_plan``
(tests/stream_cases.py) issued through the ``_native`` plan methods into outputs the test owns, WITHOUT a host
synchronisation between the calls of a sequence.  The host code behind them reuses one pinned descriptor staging per
plan (guarded by ``DescStaging::wait_free``), shares the workspace, the device descriptors and the scratch between all
calls of a plan whatever their stream (guarded by ``PlanCore::begin`` waiting on ``done``), creates the refine, cue,
retime and report blocks on the first call that needs them, regrows the retime workspace, and must send every kernel
and copy to the caller's stream.  If one of these rules broke, a call would return another call's answers: every call
of every sequence is held to its own numpy model (set A and set B of an entry have equal shapes and, by
tests/test_stream_cases_host.py, different answers for every pair), and the sentinel bytes around every output must
be intact.

The plug.  ``_plug`` queues ``torch.cuda._sleep`` for PLUG_MS milliseconds on a stream and records an event behind
it, so a call that follows returns while its own descriptor upload has not executed.  Right after the first call of
a plugged sequence returns the event is checked: still pending for an entry that only queues (the hazard window is
provably open when the next call starts to fill the staging), complete for an entry whose host code waits for the
stream (``Op.host_waits``; if that wait is ever removed, flip the flag and the window check applies).

PLUG_MS.  Measured with ``measure_call_times`` on one MI355X (gfx950), one process, an idle device, every entry on a
fresh plan at set A, four calls each: the slowest single call on the host took 13.7 ms -- ``SplitPlan.align``, the
process's first call into the library, which loads its code object; no later call took more than 0.92 ms (the first
``DriftRangePlan.report``, which also waits for its own ``align``), and no repeated call more than 0.58 ms.  Twenty
times 13.7 ms is 274 ms, above the cap of 250 ms that keeps a test at a few seconds: PLUG_MS = 250, eighteen times the
slowest call seen and 270 times the slowest that is not the process's first.  ``torch.cuda._sleep`` counts clock ticks;
their rate is measured once per session (a plug asked for 250 ms took 247.4 ms).  Needs a real MI355X.
"""
import time

import numpy as np
import pytest

import layout_cases as lc
import stream_cases as sc

pytestmark = pytest.mark.gpu

SLOWEST_CALL_MS = 13.7  # measured, see the module docstring
PLUG_MS = min(20 * SLOWEST_CALL_MS, 250.0)
FILL, SENTINEL, INPUT_POISON = 0xEE, 0xA5, 0xFF
GUARD = 64 * 1024  # sentinel bytes behind every output: more than one pair's row of the largest records
_memo = {}


def _once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def _torch():
    import torch

    return torch


# ---- the plug ----------------------------------------------------------------------------------------------------------
def _cycles_per_ms():
    """The rate of ``torch.cuda._sleep``'s clock, from one timed sleep on an idle device."""
    def make():
        torch = _torch()
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000)  # (the first launch loads the kernel)
        rates = []
        for cycles in (2_000_000, 4_000_000):
            start.record()
            torch.cuda._sleep(cycles)
            end.record()
            end.synchronize()
            rates.append(cycles / start.elapsed_time(end))
        return min(rates)  # the slower clock reading: the plug is never shorter than asked for

    return _once("rate", make)


def _plug(stream, ms=PLUG_MS):
    """Bounded device work on ``stream`` and the event behind it."""
    torch = _torch()
    cycles = int(_cycles_per_ms() * ms)
    event = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        event.record()
    return event


# ---- inputs, outputs, calls --------------------------------------------------------------------------------------------
class Inputs:
    """The device inputs of one problem set of an entry: the vectors in one clean image, and the extras."""

    def __init__(self, op, which, n, late=False):
        torch = _torch()
        self.probs = op.problems(which, n)
        self.img = _once(("image", op.name, which, n), lambda: lc.build(op.vectors(self.probs), op.kind, "clean"))
        self.extra_host = {k: np.ascontiguousarray(v).copy() for k, v in op.extras(self.probs).items()}
        host = [self.img.host] + list(self.extra_host.values())
        self.staged = [torch.from_numpy(h).cuda() for h in host]
        # late inputs: the buffers the call reads hold 0xFF until ``arrive`` copies the staged bytes in
        self.real = [torch.full_like(t, INPUT_POISON) for t in self.staged] if late else self.staged
        self.ptrs = np.uint64(self.real[0].data_ptr()) + self.img.offs.astype(np.uint64)
        self.extra = dict(zip(self.extra_host, self.real[1:]))
        assert all(t.data_ptr() % 64 == 0 for t in self.real)

    def arrive(self):
        """(on the current stream)"""
        for dst, src in zip(self.real, self.staged):
            dst.copy_(src, non_blocking=True)

    def assert_untouched(self, what):
        for t, h in zip(self.staged, [self.img.host] + list(self.extra_host.values())):
            assert np.array_equal(t.cpu().numpy(), h), "%s: the call changed its inputs" % what


def _inputs(op, which, n):
    return _once(("inputs", op.name, which, n), lambda: Inputs(op, which, n))


class Arena:
    """The outputs of one call in one buffer: every output 64-byte aligned and filled with 0xEE, GUARD sentinel bytes
    in front of the first and behind each."""

    def __init__(self, specs):
        torch = _torch()
        self.slots, cursor = {}, GUARD
        for name, nbytes in specs:
            self.slots[name] = (cursor, int(nbytes))
            cursor += -(-int(nbytes) // 64) * 64 + GUARD
        self.buf = torch.full((cursor,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 64 == 0
        self.out = {name: self.buf[o:o + nb] for name, (o, nb) in self.slots.items()}
        self.refill()

    def refill(self):
        for t in self.out.values():
            t.fill_(FILL)

    def host(self, buf=None):
        raw = (self.buf if buf is None else buf).cpu().numpy()
        outside = np.ones(raw.size, bool)
        for o, nb in self.slots.values():
            outside[o:o + nb] = False
        return {name: raw[o:o + nb] for name, (o, nb) in self.slots.items()}, raw[outside]


class Call:
    """One call of a sequence: an entry, a problem set, its own outputs."""

    def __init__(self, op, which, n=sc.N_SET, inputs=None, **params):
        self.op, self.which, self.n, self.params = op, which, n, params
        self.inputs = _inputs(op, which, n) if inputs is None else inputs
        self.arena = Arena(op.outputs(self.inputs.probs))
        self.what = "%s(%s%s)" % (op.name, which, "".join(", %s %s" % kv for kv in sorted(params.items())))

    def issue(self, plan, stream):
        self.op.issue(plan, self.inputs.ptrs, self.inputs.extra, self.arena.out, self.inputs.probs, int(stream.cuda_stream),
                      **self.params)

    def want(self, i):
        if not self.params:
            return self.op.want(self.which, i, self.n)
        key = (self.op.name, self.which, i, tuple(sorted(self.params.items())))
        return _once(key, lambda: self.op.model(dict(self.inputs.probs[i], **self.params)))

    def check(self, buf=None):
        """Every pair against its model, the sentinels, the inputs (after the sequence's one synchronisation)."""
        host, outside = self.arena.host(buf)
        assert (outside == SENTINEL).all(), "%s: %d bytes outside the outputs were written" % (self.what, (outside != SENTINEL).sum())
        got = self.op.decode(self.inputs.probs, host)
        bad = [i for i, pr in enumerate(self.inputs.probs)
               if not self.op.equal(got[i], self.want(i), dict(pr, **self.params))]
        assert not bad, "%s: pairs %s differ from the model" % (self.what, bad)
        if buf is None:
            self.inputs.assert_untouched(self.what)


def _plan(ops, calls_probs, pairs_in_flight):
    """A fresh plan that fits every (op, problems) of a sequence: the largest of each size limit."""
    from ffsubsync_amd import _native

    dims = [op.plan_dims(probs, pairs_in_flight) for op, probs in zip(ops, calls_probs)]
    assert len({op.plan for op in ops}) == 1
    return getattr(_native, ops[0].plan)(*[max(d) for d in zip(*dims)])


def _plan_for(calls, pairs_in_flight=sc.N_SET):
    return _plan([c.op for c in calls], [c.inputs.probs for c in calls], pairs_in_flight)


def _ready():
    """Before a sequence: the inputs uploaded and the outputs filled, nothing pending."""
    _cycles_per_ms()
    _torch().cuda.synchronize()


def _window(event, op, what="the first call"):
    """Right after the first call of a plugged sequence returned."""
    if op.host_waits:
        assert event.query(), "%s of %s returned before the stream's earlier work: host_waits is no longer true" % (what, op.name)
    else:
        assert not event.query(), ("%s of %s returned after the plug of %.0f ms had finished: its upload was not "
                                   "pending when the next call started" % (what, op.name, PLUG_MS))


def _finish(calls):
    _torch().cuda.synchronize()
    for c in calls:
        c.check()


# ---- 1: queued on one stream -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.OP_NAMES)
def test_three_calls_queued_on_one_plugged_stream(name):
    op = sc.ops()[name]
    calls = [Call(op, which) for which in "ABA"]
    plan, s = _plan_for(calls), _torch().cuda.Stream()
    try:
        _ready()
        event = _plug(s)
        calls[0].issue(plan, s)
        _window(event, op)
        calls[1].issue(plan, s)
        calls[2].issue(plan, s)
        _finish(calls)
    finally:
        plan.close()


# ---- 2: two streams, one plan ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.OP_NAMES)
def test_two_streams_share_one_plan(name):
    """A on a plugged stream, B at once on another with nothing between the streams but the plan's own ``done`` event:
    without ``begin`` B would run inside A's workspace, descriptors and scratch."""
    torch, op = _torch(), sc.ops()[name]
    calls = [Call(op, "A"), Call(op, "B")]
    plan, s1, s2 = _plan_for(calls), torch.cuda.Stream(), torch.cuda.Stream()
    try:
        _ready()
        event = _plug(s1)
        calls[0].issue(plan, s1)
        _window(event, op)
        calls[1].issue(plan, s2)
        _finish(calls)
    finally:
        plan.close()


# ---- 3: sub-batches ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.OP_NAMES)
def test_sub_batches_refill_the_staging_inside_a_call(name):
    """Five pairs at pairs_in_flight 2: three sub-batches, the staging refilled twice inside the call, then the other set
    at once.  The second sub-batch's ``wait_free`` holds the host until the first upload has left the staging, which is
    behind the plug: when the call returns the plug has finished, whatever the entry."""
    op = sc.ops()[name]
    calls = [Call(op, "A", sc.N_SUB_BATCHES), Call(op, "B", sc.N_SUB_BATCHES)]
    plan, s = _plan_for(calls, pairs_in_flight=2), _torch().cuda.Stream()
    try:
        _ready()
        event = _plug(s)
        calls[0].issue(plan, s)
        assert event.query(), "a call of three sub-batches returned while its first upload was pending"
        calls[1].issue(plan, s)
        _finish(calls)
    finally:
        plan.close()


# ---- 4: mixed entry points on one plan, first use included -------------------------------------------------------------
MIXED = {
    # refine(A) consumes the offsets its own align wrote on the stream; the cue, retime, refine and report blocks are made
    # while earlier calls are pending; the retime workspace grows at radius 200 and is kept at radius 5
    "SplitPlan": [("align", "A", {}), ("refine", "A", {}), ("cue_report", "B", {}), ("cue_retime", "A", dict(radius=5)),
                  ("cue_retime", "B", dict(radius=200)), ("cue_retime", "A", dict(radius=5)), ("align_report", "B", {}),
                  ("drift_refine", "A", {})],
    "DriftPlan": [("align", "A", {}), ("report", "B", {}), ("smooth", "A", {}), ("align", "B", {})],
    "SplitRangePlan": [("align", "A", {}), ("report", "B", {}), ("align", "A", {})],
    "DriftRangePlan": [("align", "A", {}), ("smooth", "B", {}), ("report", "A", {}), ("align", "B", {})],
}


@pytest.mark.parametrize("plan_class", list(MIXED))
def test_mixed_entry_points_on_a_fresh_plan(plan_class):
    calls = [Call(sc.ops()["%s.%s" % (plan_class, method)], which, **params) for method, which, params in MIXED[plan_class]]
    plan, s = _plan_for(calls), _torch().cuda.Stream()
    try:
        _ready()
        event = _plug(s)
        calls[0].issue(plan, s)
        _window(event, calls[0].op)
        for c in calls[1:]:
            c.issue(plan, s)
        _finish(calls)
    finally:
        plan.close()


# ---- 5: destroy while pending ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["SplitPlan.align", "QualityPlan.report", "MatchPlan.report", "SplitRangePlan.align",
                                  "DriftPlan.align", "DriftRangePlan.align"])
def test_destroy_waits_for_the_pending_call(name):
    op = sc.ops()[name]
    call = Call(op, "A")
    plan, s = _plan_for([call]), _torch().cuda.Stream()
    try:
        _ready()
        event = _plug(s)
        call.issue(plan, s)
        _window(event, op)
    finally:
        plan.close()
    assert plan.handle is None and event.query(), "the destroy returned while the plan's last call was pending"
    _finish([call])


# ---- 6: late inputs, results consumed on the stream --------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.OP_NAMES)
def test_late_inputs_and_results_consumed_on_the_stream(name):
    """The inputs arrive on the caller's stream behind the plug (until then the buffers hold 0xFF), and the outputs are
    cloned and overwritten on that stream right behind the call: a kernel or copy sent to any other stream would read
    the poison, or write after the clone."""
    torch, op = _torch(), sc.ops()[name]
    inputs = Inputs(op, "A", sc.N_SET, late=True)
    call = Call(op, "A", inputs=inputs)
    plan, s = _plan_for([call]), torch.cuda.Stream()
    try:
        _ready()
        event = _plug(s)
        with torch.cuda.stream(s):
            inputs.arrive()
            call.issue(plan, s)
            _window(event, op)
            keep = call.arena.buf.clone()
            call.arena.refill()
        torch.cuda.synchronize()
        call.check(keep)
        host, outside = call.arena.host()
        assert (outside == SENTINEL).all() and all((v == FILL).all() for v in host.values()), "written after the clone"
        assert all(np.array_equal(r.cpu().numpy(), st.cpu().numpy()) for r, st in zip(inputs.real, inputs.staged))
    finally:
        plan.close()


# ---- the measurement behind PLUG_MS ------------------------------------------------------------------------------------
def measure_call_times(repeats=3):
    """{entry: (host ms of the first call on a fresh plan, of the slowest later call)} on an idle device: the figures
    SLOWEST_CALL_MS is taken from (run from a script; no test calls this)."""
    torch = _torch()
    out = {}
    for name, op in sc.ops().items():
        call = Call(op, "A")
        plan, s = _plan_for([call]), torch.cuda.Stream()
        try:
            times = []
            for _ in range(repeats + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call.issue(plan, s)
                times.append(1e3 * (time.perf_counter() - t0))
            torch.cuda.synchronize()
            call.check()
        finally:
            plan.close()
        out[name] = (times[0], max(times[1:]))
    return out
