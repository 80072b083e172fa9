"""Every refusal of the side plans' host code, by code, full message and order: the 16 batch entry points of
tests/stream_cases.py (``ops()``) and the six plan creates, called through the ``_native`` plan classes.

For each entry point the arguments of the table's valid call (set A, the smallest shapes ``stream_cases`` has) are taken
as the ``_native`` method would get them, exactly one is spoiled -- a scalar, a length, a lag range, a null address or
a misaligned one -- and the ``NativeError``'s code and whole message are compared with
tests/golden/side_plan_refusals.json.  A few doubly spoiled calls per family fix which of two wrong things is
reported.  Every refused call must leave ``workspace_bytes`` as it was, and the valid call that follows on the same
plan must still give the table's expected result.

Every case is one the host code refuses before it launches anything, chosen by reading the check it targets in
csrc/ffsalign.hip: no spoiled address is ever read.  (The two range reports copy the block offsets to the host before
their "outside the lag range" check: that case hands them a real tensor of offsets that no range holds.)  Not covered,
because a caller of the plan classes cannot reach them: ``n_pairs < 0``, a null per-pair host array, a null output
handle, an unknown match algorithm, the allocation failures, and the checks ``ffs_match_quality_batch`` makes on the
list headers after its first launch.

The golden file was recorded with tests/golden/make_side_plan_refusals.py from a library built from the commit before
the host code was folded onto shared helpers; the messages hold the problem sets' own lengths and ranges, which are
seeded.  Needs a real MI355X.
"""
import inspect
import json
import os

import numpy as np
import pytest

import stream_cases as sc
import test_gpu_streams as ts

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "side_plan_refusals.json")
BLOCK_PLANS = ("SplitPlan", "DriftPlan", "SplitRangePlan", "DriftRangePlan")  # (pairs_in_flight, max_blocks, max_lags, max_samples, ..)


# ---- spoiling one argument ---------------------------------------------------------------------------------------------
class At:
    """Stands in for a CUDA tensor argument: the tensor's sizes (or ``nbytes`` bytes) at another address."""

    def __init__(self, tensor, addr, nbytes=None):
        self._addr = int(addr)
        self._numel = tensor.numel() if nbytes is None else int(nbytes)
        self._size = tensor.element_size() if nbytes is None else 1

    def data_ptr(self):
        return self._addr

    def numel(self):
        return self._numel

    def element_size(self):
        return self._size


def null(t, plan):
    return At(t, 0)


def skew(n):
    return lambda t, plan: At(t, t.data_ptr() + n)


def sized(nbytes):
    """The tensor's address with a size no table has: only the size may be looked at."""
    return lambda t, plan: At(t, t.data_ptr(), nbytes)


def put(i, v):
    """Entry ``i`` of a per-pair host array set to ``v`` (or ``v(plan, array)``)."""
    def spoil(old, plan):
        a = np.array(old)
        a[i] = v(plan, a) if callable(v) else v
        return a

    return spoil


def one_more(old, plan):
    a = np.asarray(old)
    return np.append(a, a[:1])


def filled(value):
    def spoil(t, plan):
        import torch

        return torch.full_like(t, value)

    return spoil


MISALIGNED = lambda plan, a: int(a[0]) + 1
PAST_SAMPLES = lambda plan, a: plan.max_samples + 1
LAST_BLOCK = lambda plan, a: plan.max_samples  # (the plans are made for longer vectors than the set's: ``_make_plan``)
NAN, INF = float("nan"), float("inf")

# ---- the cases: (name, {parameter of the _native method: spoiled value or spoil(old, plan)}) ---------------------------
PAIRS = [("empty reference", {"ref_len": put(1, 0)}), ("empty subtitle", {"sub_len": put(0, -3)}),
         ("misaligned vector", {"ref_ptr": put(0, MISALIGNED)}), ("null vector", {"sub_ptr": put(1, 0)}),
         ("infinite level", {"sub_hi": put(0, INF)}), ("nan level", {"ref_lo": put(2, NAN)})]
BLOCK = [("block_samples small", {"block_samples": 224}), ("block_samples odd", {"block_samples": 272}),
         ("block_samples large", {"block_samples": 32800})]
WINDOW = [("window zero", {"max_offset_samples": 0}), ("window huge", {"max_offset_samples": 131073}),
          ("window past plan", {"max_offset_samples": lambda w, plan: plan.max_lags // 2 + 1})]
PENALTY = [("penalty nan", {"split_penalty": NAN}), ("penalty negative", {"split_penalty": -0.5})]
TOP_K = [("top_k zero", {"top_k": 0}), ("top_k nine", {"top_k": 9}), ("exclusion zero", {"exclusion_samples": 0})]
STEP = [("max_step negative", {"max_step": -1}), ("max_step eight", {"max_step": 8}), ("step_cost nan", {"step_cost": NAN}),
        ("step_cost infinite", {"step_cost": INF}), ("step_cost negative", {"step_cost": -1.0})]
WINDOW_LIMITS = [("subtitle past max_samples", {"sub_len": put(0, PAST_SAMPLES)}), ("blocks past max_blocks", {"sub_len": put(0, LAST_BLOCK)})]
RANGE_LIMITS = [("reference past max_samples", {"ref_len": put(0, PAST_SAMPLES)}), ("subtitle past max_samples", {"sub_len": put(1, PAST_SAMPLES)}),
                ("blocks past max_blocks", {"sub_len": put(0, LAST_BLOCK)}),
                ("lag range reversed", {"lag_lo": put(0, 5), "lag_hi": put(0, 4)}),
                ("lag_hi past int32", {"lag_hi": put(1, 2**31)}), ("lag_lo past int32", {"lag_lo": put(1, -2**31)}),
                ("lags past max_lags", {"lag_lo": put(0, 0), "lag_hi": put(0, lambda plan, a: plan.max_lags)})]
SOLVE_OUT = [("null offsets", {"offsets_out": null}), ("null scores", {"scores_out": null}), ("null totals", {"totals_out": null})]
RANGE_OUT = SOLVE_OUT + [("misaligned offsets", {"offsets_out": skew(2)}), ("misaligned scores", {"scores_out": skew(4)}),
                         ("misaligned totals", {"totals_out": skew(4)})]
SMOOTH = [("knot_blocks zero", {"knot_blocks": 0}), ("knot_blocks large", {"knot_blocks": 257}), ("radius negative", {"radius": -1}),
          ("radius large", {"radius": 17}), ("bend_cost nan", {"bend_cost": NAN}), ("bend_cost infinite", {"bend_cost": INF}),
          ("null smooth offsets", {"smooth_out": null}), ("null knots", {"knot_out": null}), ("null segments", {"segments_out": null}),
          ("null segment counts", {"n_segments_out": null}), ("misaligned smooth offsets", {"smooth_out": skew(2)}),
          ("misaligned segments", {"segments_out": skew(4)}), ("misaligned segment counts", {"n_segments_out": skew(2)}),
          ("order: knot_blocks before bend_cost", {"knot_blocks": 0, "bend_cost": NAN}),
          ("order: step_cost before radius", {"step_cost": NAN, "radius": -1}),
          ("order: smooth outputs before pairs", {"smooth_out": skew(2), "ref_len": put(0, 0)})]
REFINE = PAIRS + BLOCK + [
    ("null offsets", {"offsets": null}), ("null records", {"refine_out": null}), ("misaligned offsets", {"offsets": skew(2)}),
    ("misaligned records", {"refine_out": skew(4)}), ("radius zero", {"radius_samples": 0}), ("radius large", {"radius_samples": 131073}),
    ("margin negative", {"unmatched_margin": -1.0}), ("margin infinite", {"unmatched_margin": INF}),
    ("reference past 2^30", {"ref_len": put(0, 2**30)}), ("subtitle past 2^30", {"sub_len": put(1, 2**30)}),
    ("order: misaligned before block_samples", {"offsets": skew(2), "block_samples": 224}),
    ("order: block_samples before radius", {"block_samples": 224, "radius_samples": 0}),
    ("order: radius before margin", {"radius_samples": 0, "unmatched_margin": -1.0}),
    ("order: margin before pairs", {"unmatched_margin": -1.0, "ref_len": put(0, 0)}),
    ("order: pair 0 length before pair 1 vector", {"ref_len": put(0, 2**30), "sub_ptr": put(1, 0)})]
CUES = PAIRS + [
    ("radius negative", {"radius_samples": -1}), ("context negative", {"context_samples": -1}), ("context large", {"context_samples": 65537}),
    ("reference past 2^30", {"ref_len": put(0, 2**30)}), ("cue_count negative", {"cue_count": put(1, -1)}),
    ("cue_first negative", {"cue_first": put(0, -1)}), ("cue_first past table", {"cue_first": put(0, 10**6)}),
    ("cue_count past table", {"cue_count": put(1, 10**6)}), ("null cue table", {"cues": null}), ("misaligned cue table", {"cues": skew(4)}),
    ("order: radius before context", {"radius_samples": -1, "context_samples": -1}),
    ("order: cue_count before cue table", {"cue_count": put(1, -1), "cues": skew(4)}),
    ("order: pair 0 cues before pair 1 length", {"cue_first": put(0, -1), "ref_len": put(1, 0)})]
MANY_CUES = 2**30 + 1
SPLIT = PAIRS + BLOCK + WINDOW + PENALTY + WINDOW_LIMITS + SOLVE_OUT + [
    ("order: null before block_samples", {"totals_out": null, "block_samples": 224}),
    ("order: block_samples before window", {"block_samples": 224, "max_offset_samples": 0}),
    ("order: window before penalty", {"max_offset_samples": lambda w, plan: plan.max_lags // 2 + 1, "split_penalty": NAN}),
    ("order: penalty before pairs", {"split_penalty": NAN, "ref_len": put(0, 0)})]
REPORT_OUT = [("null report", {"report_out": null}), ("misaligned report", {"report_out": skew(4)})]
DRIFT = SPLIT + STEP + [("null jumps", {"jumps_out": null}), ("order: penalty before max_step", {"split_penalty": NAN, "max_step": -1}),
                        ("order: max_step before step_cost", {"max_step": 8, "step_cost": NAN}),
                        ("order: step_cost before pairs", {"step_cost": NAN, "sub_ptr": put(0, 0)})]
RANGE = PAIRS + BLOCK + PENALTY + RANGE_LIMITS + RANGE_OUT + [
    ("order: null before misaligned", {"offsets_out": null, "scores_out": skew(4)}),
    ("order: misaligned before block_samples", {"scores_out": skew(4), "block_samples": 224}),
    ("order: block_samples before penalty", {"block_samples": 224, "split_penalty": NAN}),
    ("order: penalty before pairs", {"split_penalty": NAN, "ref_len": put(0, 0)}),
    ("order: lengths before lag range", {"ref_len": put(0, PAST_SAMPLES), "lag_hi": put(0, 2**31)}),
    ("order: blocks before lag range", {"sub_len": put(0, LAST_BLOCK), "lag_hi": put(0, 2**31)}),
    ("order: pair 0 lag range before pair 1 vector", {"lag_hi": put(0, 2**31), "ref_ptr": put(1, 0)})]
RANGE_REPORT = PAIRS + BLOCK + TOP_K + RANGE_LIMITS + REPORT_OUT + [
    ("null offsets", {"offsets": null}), ("misaligned offsets", {"offsets": skew(2)}),
    ("offsets outside the lag range", {"offsets": filled(2**30)}),
    ("order: misaligned before block_samples", {"offsets": skew(2), "block_samples": 224}),
    ("order: block_samples before top_k", {"block_samples": 224, "top_k": 0}),
    ("order: top_k before exclusion", {"top_k": 0, "exclusion_samples": 0}),
    ("order: exclusion before pairs", {"exclusion_samples": 0, "ref_len": put(0, 0)}),
    ("order: lag range before offsets", {"lag_hi": put(0, 2**31), "offsets": filled(2**30)})]
QUALITY = [("window below -1", {"max_offset_samples": -2}), ("lags past max_lags", {"max_offset_samples": None, "ref_len": put(0, LAST_BLOCK)}), ("null records", {"out": null}),
           ("misaligned records", {"out": skew(4)}), ("order: window before top_k", {"max_offset_samples": -2, "top_k": 0}),
           ("order: exclusion before misaligned", {"exclusion_samples": 0, "out": skew(4)})] + TOP_K
CASES = {
    "SplitPlan.align": SPLIT,
    "SplitPlan.align_report": SPLIT + TOP_K + REPORT_OUT + [
        ("null piece counts", {"n_pieces_out": null}), ("misaligned piece counts", {"n_pieces_out": skew(2)}),
        ("order: penalty before top_k", {"split_penalty": NAN, "top_k": 0}), ("order: top_k before exclusion", {"top_k": 9, "exclusion_samples": 0}),
        ("order: exclusion before report", {"exclusion_samples": 0, "report_out": null}),
        ("order: report before pairs", {"report_out": skew(4), "ref_len": put(0, 0)})],
    "SplitPlan.refine": REFINE + [("null break counts", {"n_breaks_out": null}), ("misaligned break counts", {"n_breaks_out": skew(2)})],
    "SplitPlan.drift_refine": REFINE + [("null jumps", {"jumps": null}), ("null jump counts", {"n_jumps_out": null})],
    "SplitPlan.cue_report": CUES + [
        ("radius large", {"radius_samples": 4097}), ("null report", {"report_out": null}), ("misaligned report", {"report_out": skew(4)}),
        ("cue table past 2^30", {"cues": sized(24 * MANY_CUES), "report_out": sized(120 * MANY_CUES)}),
        ("order: context before table size", {"context_samples": -1, "cues": sized(24 * MANY_CUES), "report_out": sized(120 * MANY_CUES)})],
    "SplitPlan.cue_retime": CUES + [
        ("radius large", {"radius_samples": 1025}), ("penalty_q negative", {"penalty_q": -1}), ("penalty_q large", {"penalty_q": 2**20 + 1}),
        ("jump_q below -1", {"jump_q": -2}), ("jump_q large", {"jump_q": 2**40 + 1}), ("unknown flag", {"flags": 2}),
        ("cue table past 2^30", {"cues": sized(24 * MANY_CUES), "retime_out": sized(64 * MANY_CUES)}),
        ("cues past the workspace cap", {"cues": sized(24 * 30000), "retime_out": sized(64 * 30000), "cue_first": put(0, 0),
                                         "cue_count": put(0, 30000), "radius_samples": 1024}),
        ("null summary", {"summary_out": null}), ("misaligned summary", {"summary_out": skew(4)}), ("null records", {"retime_out": null}),
        ("misaligned records", {"retime_out": skew(4)}),
        ("order: context before penalty_q", {"context_samples": -1, "penalty_q": -1}), ("order: penalty_q before jump_q", {"penalty_q": -1, "jump_q": -2}),
        ("order: jump_q before flags", {"jump_q": -2, "flags": 2}),
        ("order: flags before table size", {"flags": 2, "cues": sized(24 * MANY_CUES), "retime_out": sized(64 * MANY_CUES)}),
        ("order: cues before summary", {"cue_count": put(1, -1), "summary_out": null}),
        ("order: summary before cue table", {"summary_out": skew(4), "cues": skew(4)})],
    "QualityPlan.report": PAIRS + QUALITY + [("reference past max_samples", {"ref_len": put(0, PAST_SAMPLES)}),
                                             ("subtitle past max_samples", {"sub_len": put(1, PAST_SAMPLES)}),
                                             ("order: misaligned before pairs", {"out": skew(4), "ref_len": put(0, 0)})],
    "MatchPlan.report": QUALITY + [
        ("too many vectors", {"ref_list": one_more, "ref_len": one_more, "ref_lo": one_more, "ref_hi": one_more}),
        ("empty reference", {"ref_len": put(1, 0)}), ("empty subtitle", {"sub_len": put(0, -3)}),
        ("misaligned list", {"ref_list": put(0, lambda plan, a: int(a[0]) + 4)}), ("null list", {"sub_list": put(1, 0)}),
        ("reference past max_samples", {"ref_len": put(0, PAST_SAMPLES)}), ("infinite level", {"sub_hi": put(0, INF)}),
        ("nan level", {"ref_lo": put(2, NAN)}), ("reference index past table", {"pair_ref": put(0, sc.N_SET)}),
        ("subtitle index negative", {"pair_sub": put(1, -1)}),
        ("order: misaligned before vectors", {"out": skew(4), "ref_len": put(0, 0)}),
        ("order: reference before subtitle", {"ref_hi": put(3, INF), "sub_len": put(0, 0)}),
        ("order: vectors before pairs", {"sub_list": put(3, 0), "pair_ref": put(0, -1)})],
    "SplitRangePlan.align": RANGE,
    "SplitRangePlan.report": RANGE_REPORT + [("null piece counts", {"n_pieces_out": null}), ("misaligned piece counts", {"n_pieces_out": skew(2)})],
    "DriftPlan.align": DRIFT,
    "DriftPlan.report": DRIFT + TOP_K + REPORT_OUT + [
        ("null segment counts", {"n_segments_out": null}), ("misaligned segment counts", {"n_segments_out": skew(2)}),
        ("order: step_cost before top_k", {"step_cost": NAN, "top_k": 0}), ("order: exclusion before report", {"exclusion_samples": 0, "report_out": null})],
    "DriftPlan.smooth": DRIFT + SMOOTH,
    "DriftRangePlan.align": RANGE + STEP + [("null jumps", {"jumps_out": null}),
                                            ("max_step past the plan's cap", {"max_step": lambda s, plan: plan.max_step_cap + 1}),
                                            ("order: penalty before max_step", {"split_penalty": NAN, "max_step": -1}),
                                            ("order: step_cost before pairs", {"step_cost": NAN, "ref_len": put(0, 0)})],
    "DriftRangePlan.smooth": RANGE + STEP + SMOOTH + [("null jumps", {"jumps_out": null})],
    "DriftRangePlan.report": RANGE_REPORT + [("null jumps", {"jumps": null}), ("null segment counts", {"n_segments_out": null}),
                                             ("misaligned segment counts", {"n_segments_out": skew(2)})],
}
CREATES = {
    "SplitPlan": [(0, 1, 2, 1), (1, 0, 2, 1), (1, 1, 1, 1), (1, 1, 262145, 1), (1, 1, 2, 0)],
    "DriftPlan": [(0, 1, 2, 1), (1, 0, 2, 1), (1, 1, 1, 1), (1, 1, 262145, 1), (1, 1, 2, 0)],
    "SplitRangePlan": [(0, 1, 1, 1), (65536, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 2**31, 1), (1, 1, 1, 0), (1, 1, 1, 2**30)],
    "DriftRangePlan": [(0, 1, 1, 1, 0), (65536, 1, 1, 1, 0), (1, 0, 1, 1, 0), (1, 1, 0, 1, 0), (1, 1, 2**31, 1, 0), (1, 1, 1, 0, 0),
                       (1, 1, 1, 2**30, 0), (1, 1, 1, 1, -1), (1, 1, 1, 1, 8)],
    "QualityPlan": [(0, 1, 1), (1, 0, 1), (1, 2**31 + 1, 1), (1, 1, 0), (1, 1, 2**30)],
    "MatchPlan": [(0, 1, 1, 2), (1, 0, 1, 2), (1, 2**31 + 1, 1, 2), (1, 1, 0, 2), (1, 1, 2**29, 2), (1, 1, 1, 1), (1, 1, 1, 2**24 + 1)],
}


# ---- running them ------------------------------------------------------------------------------------------------------
class _Recorder:
    """In place of a plan: keeps the calls ``Op.issue`` makes instead of making them."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args, **kwargs: self.calls.append((name, args, kwargs))


def _refusal(call):
    """(code, message) of the ``NativeError`` that ``call()`` raises; None if it returns."""
    from ffsubsync_amd import _native

    try:
        call()
    except _native.NativeError as e:
        return [e.code, str(e).split(": ", 1)[1]]
    return None


def _make_plan(op, probs):
    from ffsubsync_amd import _native

    dims = list(op.plan_dims(probs, sc.N_SET))
    if op.plan in BLOCK_PLANS:
        dims[3] += sc.K  # one block more than the longest vector: "blocks past max_blocks" needs a length the plan takes
    else:
        dims[2] *= 4  # (pairs_in_flight, max_lags, max_samples, ..): "lags past max_lags" needs a length the plan takes
    return getattr(_native, op.plan)(*dims)


def op_refusals(name):
    """{case: (code, message) or None} of an entry point's cases, after which the valid call is made and checked."""
    torch = ts._torch()
    op = sc.ops()[name]
    valid = ts.Call(op, "A")
    plan = _make_plan(op, valid.inputs.probs)
    stream = torch.cuda.current_stream()
    rec = _Recorder()
    op.issue(rec, valid.inputs.ptrs, valid.inputs.extra, valid.arena.out, valid.inputs.probs, int(stream.cuda_stream))
    method, args, kwargs = rec.calls[-1]
    assert method == op.method
    target = getattr(plan, method)
    good = dict(inspect.signature(target).bind(*args, **kwargs).arguments)
    got = {}
    closed = _make_plan(op, valid.inputs.probs)
    closed.close()
    got["closed plan"] = _refusal(lambda: getattr(closed, method)(**good))
    for case, spoils in CASES[name]:
        assert case not in got and set(spoils) <= set(good), (name, case)
        bad = dict(good)
        for key, spoil in spoils.items():
            bad[key] = spoil(good[key], plan) if callable(spoil) else spoil
        before = plan.workspace_bytes
        got[case] = _refusal(lambda: target(**bad))
        assert plan.workspace_bytes == before, "%s, %s: a refused call changed workspace_bytes" % (name, case)
    torch.cuda.synchronize()
    valid.issue(plan, stream)
    torch.cuda.synchronize()
    valid.check()
    plan.close()
    return got


def create_refusals(name):
    from ffsubsync_amd import _native

    return {repr(dims): _refusal(lambda: getattr(_native, name)(*dims)) for dims in CREATES[name]}


def record(path=GOLDEN):
    """Write the golden file from the library in use (tests/golden/make_side_plan_refusals.py)."""
    out = {name: op_refusals(name) for name in sc.OP_NAMES}
    out.update({name + " create": create_refusals(name) for name in sc.PLAN_CLASSES})
    silent = [(name, case) for name, cases in out.items() for case, r in cases.items() if r is None]
    assert not silent, "not refused: %s" % silent
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return out


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _differences(got, want):
    assert sorted(got) == sorted(want), "the cases and the golden file differ: %s" % sorted(set(got) ^ set(want))
    return ["%s: got %s, want %s" % (case, got[case], want[case]) for case in sorted(got) if got[case] != want[case]]


@pytest.mark.parametrize("name", sc.OP_NAMES)
def test_refusals(name):
    bad = _differences(op_refusals(name), _golden()[name])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", sc.PLAN_CLASSES)
def test_create_refusals(name):
    bad = _differences(create_refusals(name), _golden()[name + " create"])
    assert not bad, "\n".join(bad)
