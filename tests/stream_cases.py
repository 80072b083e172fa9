"""TEST INFRASTRUCTURE ONLY -- the table of the side plans' batch entry points for tests/test_gpu_streams.py, checked on
the host by tests/test_stream_cases_host.py.  Host data only: imports without a GPU.

One ``Op`` per export of include/ffsubsync_amd.h that takes a side plan (``ffs_split_plan``, ``ffs_quality_plan``,
``ffs_match_plan``, ``ffs_split_range_plan``, ``ffs_drift_plan``, ``ffs_drift_range_plan``) and ends in ``_batch``.  An
``Op`` says which ``_native`` plan class it runs on and how to size it, which device inputs it reads beside the vectors,
which outputs it writes (bytes each, so a caller can lay them out in one arena), how to issue the call asynchronously
through the ``_native`` plan method on a given stream, how to turn the raw output bytes into what the family's comparison
takes (the decoding the wrapper module performs after its own call), and the family's numpy model and comparison --
the ``model`` / ``same`` pairs tests/test_gpu_layout.py assembles (``FAMILY_MODELS``), tests/cue_model.py,
tests/retime_model.py and tests/drift_refine_model.py through the helpers of their own GPU tests, and for the segment
report over a lag range tests/report_reference.py as tests/test_gpu_drift_range_report.py uses it.  No expected value
comes from a device run and no tolerance is added.

Problem sets.  Set "A" of an op is the first problems of the family's small set as ``test_gpu_layout._family_problems``
picks them (K = 256, short vectors); the parameters that a call takes once (window, penalties, top_k, ...) are those
of the first problem, and a lag range without any overlap is moved around lag 0 (``_overlapping``).  Set "B" is A with every vector reversed and 3 % of its samples flipped (seeded): the same pair
count, lengths, cue tables, paths and parameters, other contents.  Equal shapes are a safety rule: if two calls'
descriptors were ever mixed, the result is wrong numbers inside the same buffers, never an access outside them.

Three entry points need offsets that another call makes.  ``refine`` and the two range reports are issued as their
wrappers issue them: the plan's ``align`` first, into outputs of the same call, then the entry point on those offsets on
the same stream (no host synchronisation between them).  ``drift_refine`` runs on a split plan, which has no drift
solve: its path is part of the problem (tests/test_gpu_drift_refine.py's seeded walks) and is uploaded as an input.

``host_waits``: whether the host code waits for the caller's stream inside the call, read from ffsalign.hip --
``ffs_split_range_report_batch`` and ``ffs_drift_range_report_batch`` read the block offsets (and jump flags) back
before they make their work items, ``ffs_align_drift_report_batch`` reads each sub-batch's segment counts back, and
``ffs_match_quality_batch`` reads the list headers back; every other entry point only queues.
"""
import re

import numpy as np

import layout_cases as lc
from ffsubsync_amd import _native

K = 256
N_SET = 4  # pairs of a problem set
N_SUB_BATCHES = 5  # pairs of the sets of the sub-batch sequence (pairs_in_flight 2: three sub-batches)
CALL_KEYS = ("w", "p", "s", "q", "m", "r", "lam", "top_k", "e", "excl", "radius", "beta", "context", "pq", "jq", "keep")
SIDE_PLANS = ("ffs_split_plan", "ffs_quality_plan", "ffs_match_plan", "ffs_split_range_plan", "ffs_drift_plan",
              "ffs_drift_range_plan")
_memo = {}


def _once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def header_exports(text):
    """{export: plan type} of every declaration ``int ffs_..._batch(<side plan>* ...`` in the header's text."""
    found = re.findall(r"\bint\s+(ffs_\w+_batch)\s*\(\s*(ffs_\w+_plan)\s*\*", text)
    return {name: plan for name, plan in found if plan in SIDE_PLANS}


# ---- problem sets ------------------------------------------------------------------------------------------------------
def _tgl():
    import test_gpu_layout as tgl

    _once("families", tgl._families)
    return tgl


def _with_call_parameters(probs, **more):
    """The problems with the parameters a call takes once set to those of the first (and ``more``)."""
    first = dict(probs[0], **more)
    shared = {k: first[k] for k in CALL_KEYS if k in first}
    return [dict(pr, **shared) for pr in probs]


def _overlapping(pr):
    """A lag range in which the two vectors never overlap has one answer whatever they hold, so nothing would tell two
    calls apart: such a range is moved, at its width, around lag 0."""
    if "lo" not in pr or (pr["lo"] <= pr["rb"].size - 1 and pr["hi"] >= -(pr["sb"].size - 1)):
        return pr
    width = pr["hi"] - pr["lo"]
    return dict(pr, lo=-(width // 2), hi=width - width // 2)


def _family_set(family, n, **more):
    return _with_call_parameters([_overlapping(pr) for pr in _tgl()._family_problems(family)[:n]], **more)


def _cue_set(module, n, **params):
    """``n`` pairs of the edge problems of a cue test (tests/test_gpu_cue_report.py, tests/test_gpu_cue_retime.py) that
    hold cues, with their cue tables."""
    import importlib

    probs, cues = importlib.import_module(module).EDGE
    pick = [1, 3, 4, 5, 0][:n]
    return [dict(probs[i], cues=tuple(np.asarray(c, np.int64) for c in cues[i]), **params) for i in pick]


def _drift_refine_set(n):
    """The first ``n`` seeded walks of tests/test_gpu_drift_refine.py at radius 100 that hold a jump (a pair without
    one has no record: nothing would tell two calls apart)."""
    import test_gpu_drift_refine as t

    pick = [pr for pr in t.FUZZ if pr["radius"] == 100 and pr["jf"][1:].any()][:n]
    assert len(pick) == n
    return _with_call_parameters([dict(pr, rb=pr["rb"].astype(np.uint8), sb=pr["sb"].astype(np.uint8)) for pr in pick])


def rewrite(pr, seed):
    """Set B's version of a problem: both vectors reversed, then 3 % of their samples flipped (at least one)."""
    rng = np.random.RandomState(seed)
    out = dict(pr)
    for key in ("rb", "sb"):
        v = np.asarray(pr[key]).astype(np.uint8)[::-1].copy()
        flip = rng.rand(v.size) < 0.03
        flip[rng.randint(v.size)] = True
        out[key] = v ^ flip.astype(np.uint8)
    return out


# ---- shapes ------------------------------------------------------------------------------------------------------------
def _lens(probs):
    return (np.array([pr["rb"].size for pr in probs], np.int64), np.array([pr["sb"].size for pr in probs], np.int64))


def _blocks(probs):
    n_blocks = (_lens(probs)[1] + K - 1) // K
    return n_blocks, int(n_blocks.max())


def _lags(probs):
    return np.array([pr["lo"] for pr in probs], np.int64), np.array([pr["hi"] for pr in probs], np.int64)


def _cue_table(probs):
    from ffsubsync_amd import cue_report as cr

    return cr.flat_cue_table([pr["cues"] for pr in probs], len(probs))


def _padded_path(probs):
    n_blocks, max_b = _blocks(probs)
    offs, jumps = np.zeros((len(probs), max_b), np.int32), np.zeros((len(probs), max_b), np.uint8)
    for p, pr in enumerate(probs):
        offs[p, :n_blocks[p]], jumps[p, :n_blocks[p]] = pr["o"], pr["jf"]
    return offs, jumps


SOLVE = (("offs", 4), ("scores", 8), ("totals", None))  # bytes per (pair, block); None: 8 bytes per pair
DRIFT = SOLVE + (("jumps", 1),)


def _solve_bytes(probs, names):
    n, max_b = len(probs), _blocks(probs)[1]
    return [(name, n * 8 if per is None else n * max_b * per) for name, per in names]


def _view(host, name, dtype, shape=None):
    a = np.ascontiguousarray(host[name]).view(dtype)
    return a if shape is None else a.reshape(shape)


def _tensors(host, names):
    """Host copies of the solve outputs as CPU tensors: what the wrappers' decoders take."""
    import torch

    kinds = dict(offs=np.int32, scores=np.float64, totals=np.float64, jumps=np.uint8)
    return [torch.from_numpy(_view(host, name, kinds[name]).copy()) for name in names]


def _split_results(probs, host):
    from ffsubsync_amd import split_align as sa

    return sa.split_results(_tensors(host, ("offs", "scores", "totals")), _blocks(probs)[0], K, _lens(probs)[1])


def _drift_results(probs, host):
    from ffsubsync_amd import drift_align as da

    offs, scores, totals, jumps = _tensors(host, ("offs", "scores", "totals", "jumps"))
    return da.drift_results(offs, scores, jumps, totals, _blocks(probs)[0], K, _lens(probs)[1])


def _rows(host, name, dtype, probs):
    return _view(host, name, dtype, (len(probs), _blocks(probs)[1]))


def _counts(host, name="counts"):
    return _view(host, name, np.int32)


# ---- the table ---------------------------------------------------------------------------------------------------------
class Op:
    """One entry point.  ``problems(which, n)``: set "A" or "B"; ``plan_dims(probs, pairs_in_flight)``: the arguments of
    ``getattr(_native, plan)``; ``extras(probs)``: {name: host array} of the device inputs beside the vectors;
    ``outputs(probs)``: [(name, bytes)]; ``issue(plan, ptrs, extra, out, probs, stream)``: the asynchronous call
    (``ptrs``: the vectors' device addresses, ``extra`` / ``out``: {name: uint8 CUDA tensor}, ``stream``: the raw
    stream); ``decode(probs, host)``: per pair, what ``same(got, want, pr)`` takes from {name: host bytes};
    ``model(pr)``: the family's numpy model."""

    kind = lc.U1

    def __init__(self, name, plan, method, export, host_waits, source, **fns):
        self.name, self.plan, self.method, self.export, self.host_waits = name, plan, method, export, host_waits
        self._source = source
        self.__dict__.update(fns)
        self.extras = fns.get("extras", lambda probs: {})

    def problems(self, which, n=N_SET):
        def make():
            a = self._source(n)
            return a if which == "A" else [rewrite(pr, 977 * (i + 1) + len(self.name)) for i, pr in enumerate(a)]

        assert which in ("A", "B")
        return _once((self.name, which, n), make)

    def want(self, which, i, n=N_SET):
        """The model's result of pair ``i`` of a set (pairs 0..3 of the four- and the five-pair sets are the same)."""
        return _once((self.name, "want", which, i), lambda: self.model(self.problems(which, n)[i]))

    def equal(self, got, want, pr):
        verdict = self.same(got, want, pr)  # None, true or an empty list of differences: equal
        return verdict is None or (isinstance(verdict, (bool, np.bool_)) and bool(verdict)) or verdict == []

    def vectors(self, probs):
        return [v for pr in probs for v in (pr["rb"], pr["sb"])]

    def pair_args(self, ptrs, probs):
        """The eight per-pair host arrays every call starts with, from the vectors' device addresses."""
        lv = lambda key, i: [pr[key][i] for pr in probs]
        r_len, s_len = _lens(probs)
        return (ptrs[0::2], r_len, lv("r_lv", 0), lv("r_lv", 1), ptrs[1::2], s_len, lv("s_lv", 0), lv("s_lv", 1))


def _window_dims(probs, pif):
    return (pif, _blocks(probs)[1], 2 * int(probs[0]["w"]), int(_lens(probs)[1].max()))


def _range_dims(probs, pif):
    lo, hi = _lags(probs)
    return (pif, _blocks(probs)[1], int((hi - lo + 1).max()), int(max(l.max() for l in _lens(probs))))


def _drift_range_dims(probs, pif):
    return _range_dims(probs, pif) + (int(probs[0]["s"]),)


def _quality_lags(probs):
    from ffsubsync_amd import quality

    return max(max(quality.n_lags(pr["rb"].size, pr["sb"].size, pr["w"]) for pr in probs), 1)


def _i32(t):
    import torch

    return t.view(torch.int32)


def _solve_out(out, names=("offs", "scores", "totals")):
    import torch

    kinds = dict(offs=torch.int32, scores=torch.float64, totals=torch.float64, jumps=torch.uint8)
    return [out[name].view(kinds[name]) for name in names]


def _ops():
    tgl = _tgl()
    fam = tgl.FAMILY_MODELS
    import test_gpu_cue_report as t_cue
    import test_gpu_cue_retime as t_retime
    import test_gpu_drift_range as t_drange
    import test_gpu_drift_refine as t_drefine
    import test_gpu_match as t_match
    import test_gpu_quality as t_quality

    ops = []

    def add(name, export, host_waits, source, **fns):
        plan, method = name.split(".")
        ops.append(Op(name, plan, method, export, host_waits, source, **fns))

    def family(name, **more):
        return lambda n: _family_set(name, n, **more)

    def one_pair(raw, p):
        """The one-pair view of a wrapper's raw result: what the families' comparisons index with 0."""
        return tuple([x[p]] if isinstance(x, list) else x[p:p + 1] for x in raw)

    # -- SplitPlan
    def split_issue(plan, ptrs, extra, out, probs, stream, op=None):
        pr = probs[0]
        plan.align(*op.pair_args(ptrs, probs), K, pr["w"], pr["p"], *_solve_out(out), stream=stream)

    def srep_issue(plan, ptrs, extra, out, probs, stream, op=None):
        pr = probs[0]
        plan.align_report(*op.pair_args(ptrs, probs), K, pr["w"], pr["p"], pr["top_k"], pr["e"], *_solve_out(out), out["rep"],
                          _i32(out["counts"]), stream=stream)

    def srep_decode(probs, host):
        raw = (_split_results(probs, host), _rows(host, "rep", _native.PIECE_REPORT_DTYPE, probs), _counts(host))
        return [one_pair(raw, p) for p in range(len(probs))]

    def refine_issue(plan, ptrs, extra, out, probs, stream, op=None):
        pr = probs[0]
        args = op.pair_args(ptrs, probs)
        offs = _solve_out(out)[0]
        plan.align(*args, K, pr["w"], pr["p"], *_solve_out(out), stream=stream)
        plan.refine(*args, K, offs, pr["radius"], np.nan if pr["beta"] is None else pr["beta"], out["rec"],
                    _i32(out["counts"]), stream=stream)

    def refine_decode(probs, host):
        res, recs = _split_results(probs, host), _rows(host, "rec", _native.BREAK_REFINE_DTYPE, probs)
        return [(res[p], recs[p:p + 1], _counts(host)[p:p + 1]) for p in range(len(probs))]

    def drefine_issue(plan, ptrs, extra, out, probs, stream, op=None):
        pr = probs[0]
        plan.drift_refine(*op.pair_args(ptrs, probs), K, _i32(extra["path_offs"]), extra["path_jumps"], pr["radius"],
                          np.nan if pr["beta"] is None else pr["beta"], out["rec"], _i32(out["counts"]), stream=stream)

    def drefine_decode(probs, host):
        recs = _rows(host, "rec", _native.BREAK_REFINE_DTYPE, probs)
        return [(recs[p], int(_counts(host)[p])) for p in range(len(probs))]

    def drefine_same(got, want, pr):
        recs, n = got
        return t_drefine._diff(recs[:n], want) + (["tail"] if recs[n:].tobytes().strip(b"\0") else [])

    def refine_outputs(probs):
        n, max_b = len(probs), _blocks(probs)[1]
        return [("rec", n * max_b * _native.BREAK_REFINE_BYTES), ("counts", n * 4)]

    def cue_extras(probs):
        return {"cues": _cue_table(probs)[0].view(np.uint8).reshape(-1)}

    def cue_slices(probs):
        _, first, count = _cue_table(probs)
        return [slice(int(f), int(f + c)) for f, c in zip(first, count)]

    def cue_issue(plan, ptrs, extra, out, probs, stream, op=None):
        pr = probs[0]
        _, first, count = _cue_table(probs)
        plan.cue_report(*op.pair_args(ptrs, probs), extra["cues"], first, count, pr["radius"], pr["context"], out["rep"],
                        stream=stream)

    def cue_decode(probs, host):
        recs = _view(host, "rep", _native.CUE_REPORT_DTYPE)
        return [recs[sl] for sl in cue_slices(probs)]

    def retime_issue(plan, ptrs, extra, out, probs, stream, op=None, radius=None):
        pr = probs[0]
        _, first, count = _cue_table(probs)
        plan.cue_retime(*op.pair_args(ptrs, probs), extra["cues"], first, count, pr["radius"] if radius is None else radius,
                        pr["context"], pr["pq"], pr["jq"], int(pr["keep"]), out["rec"], out["summary"], stream=stream)

    def retime_decode(probs, host):
        recs, sums = _view(host, "rec", _native.CUE_RETIME_DTYPE), _view(host, "summary", _native.RETIME_SUMMARY_DTYPE)
        return [(recs[sl], sums[p:p + 1]) for p, sl in enumerate(cue_slices(probs))]

    def retime_model(pr):
        recs, sums = t_retime._model([pr], [pr["cues"]], pr["radius"], pr["context"], pr["pq"], pr["jq"], pr["keep"])
        return recs, sums

    split_dims = lambda probs, pif: _window_dims(probs, pif)
    bare_dims = lambda probs, pif: (pif, 1, 2, 1)  # the refine wrappers' plan: sub-batching and descriptors only
    add("SplitPlan.align", "ffs_align_split_batch", False, family("split"), plan_dims=split_dims,
        outputs=lambda probs: _solve_bytes(probs, SOLVE), issue=split_issue, decode=_split_results, model=fam["split"][0],
        same=fam["split"][1])
    add("SplitPlan.align_report", "ffs_align_split_report_batch", False, family("split_report"), plan_dims=split_dims,
        outputs=lambda probs: _solve_bytes(probs, SOLVE + (("rep", _native.PIECE_REPORT_BYTES),)) + [("counts", 4 * len(probs))],
        issue=srep_issue, decode=srep_decode, model=fam["split_report"][0], same=fam["split_report"][1])
    add("SplitPlan.refine", "ffs_split_refine_batch", False, family("split_refine"), plan_dims=split_dims,
        outputs=lambda probs: _solve_bytes(probs, SOLVE) + refine_outputs(probs), issue=refine_issue, decode=refine_decode,
        model=fam["split_refine"][0], same=fam["split_refine"][1])
    add("SplitPlan.drift_refine", "ffs_drift_refine_batch", False, _drift_refine_set, plan_dims=bare_dims,
        extras=lambda probs: dict(zip(("path_offs", "path_jumps"), (a.reshape(-1).view(np.uint8) for a in _padded_path(probs)))),
        outputs=refine_outputs, issue=drefine_issue, decode=drefine_decode, model=t_drefine._model, same=drefine_same)
    add("SplitPlan.cue_report", "ffs_cue_report_batch", False, lambda n: _cue_set("test_gpu_cue_report", n, radius=33, context=40),
        plan_dims=bare_dims, extras=cue_extras,
        outputs=lambda probs: [("rep", _cue_table(probs)[0].size * _native.CUE_REPORT_BYTES)], issue=cue_issue, decode=cue_decode,
        model=lambda pr: t_cue._model([pr], [pr["cues"]], pr["radius"], pr["context"]),
        same=lambda got, want, pr: got.tobytes() == want.tobytes())
    add("SplitPlan.cue_retime", "ffs_cue_retime_batch", False,
        lambda n: _cue_set("test_gpu_cue_retime", n, radius=33, context=9, pq=16, jq=500, keep=True), plan_dims=bare_dims,
        extras=cue_extras,
        outputs=lambda probs: [("rec", _cue_table(probs)[0].size * _native.CUE_RETIME_BYTES),
                               ("summary", len(probs) * _native.RETIME_SUMMARY_BYTES)],
        issue=retime_issue, decode=retime_decode, model=retime_model,
        same=lambda got, want, pr: got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes())

    # -- QualityPlan, MatchPlan
    import quality_model as qm

    def quality_want(pr):
        return qm.report(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["w"], pr["top_k"], pr["e"])

    def quality_issue(plan, ptrs, extra, out, probs, stream, op=None):
        pr = probs[0]
        plan.report(*op.pair_args(ptrs, probs), pr["w"], pr["top_k"], pr["e"], out["rec"], stream=stream)

    def quality_decode(probs, host):
        return list(_view(host, "rec", _native.QUALITY_RESULT_DTYPE)[:len(probs)])

    def quality_same(compare):
        def same(rec, want, pr):  # (the helper runs the model itself)
            from ffsubsync_amd import quality

            return compare(quality.from_record(rec), pr)

        return same

    def match_issue(plan, ptrs, extra, out, probs, stream, op=None):
        pr = probs[0]
        a = op.pair_args(ptrs, probs)
        index = np.arange(len(probs))
        plan.report(*a, index, index, pr["w"], pr["top_k"], pr["e"], out["rec"], "auto", stream=stream)

    quality_out = lambda probs: [("rec", len(probs) * _native.QUALITY_RESULT_BYTES)]
    add("QualityPlan.report", "ffs_align_quality_batch", False, family("quality"),
        plan_dims=lambda probs, pif: (pif, _quality_lags(probs), int(max(l.max() for l in _lens(probs)))), outputs=quality_out,
        issue=quality_issue, decode=quality_decode, model=quality_want, same=quality_same(t_quality._compare))
    add("MatchPlan.report", "ffs_match_quality_batch", True, family("match"),
        plan_dims=lambda probs, pif: (pif, _quality_lags(probs), int(max(l.max() for l in _lens(probs))), 2 * len(probs)),
        outputs=quality_out, issue=match_issue, decode=quality_decode, model=quality_want,
        same=quality_same(t_match._compare), kind=lc.RUNS)

    # -- SplitRangePlan
    def srange_issue(plan, ptrs, extra, out, probs, stream, op=None):
        plan.align(*op.pair_args(ptrs, probs), K, *_lags(probs), probs[0]["p"], *_solve_out(out), stream=stream)

    def cutrep_issue(plan, ptrs, extra, out, probs, stream, op=None):
        pr = probs[0]
        srange_issue(plan, ptrs, extra, out, probs, stream, op)
        plan.report(*op.pair_args(ptrs, probs), K, *_lags(probs), _solve_out(out)[0], pr["top_k"], pr["e"], out["rep"],
                    _i32(out["counts"]), stream=stream)

    add("SplitRangePlan.align", "ffs_align_split_range_batch", False, family("split_range"), plan_dims=_range_dims,
        outputs=lambda probs: _solve_bytes(probs, SOLVE), issue=srange_issue, decode=_split_results, model=fam["split_range"][0],
        same=fam["split_range"][1])
    add("SplitRangePlan.report", "ffs_split_range_report_batch", True, family("cut_report"), plan_dims=_range_dims,
        outputs=lambda probs: _solve_bytes(probs, SOLVE + (("rep", _native.PIECE_REPORT_BYTES),)) + [("counts", 4 * len(probs))],
        issue=cutrep_issue, decode=srep_decode, model=fam["cut_report"][0], same=fam["cut_report"][1])

    # -- DriftPlan
    def drift_args(pr):
        return (pr["w"], pr["p"], pr["s"], pr["q"])

    def drift_issue(plan, ptrs, extra, out, probs, stream, op=None):
        offs, scores, totals, jumps = _solve_out(out, ("offs", "scores", "totals", "jumps"))
        plan.align(*op.pair_args(ptrs, probs), K, *drift_args(probs[0]), offs, scores, jumps, totals, stream=stream)

    def drep_issue(plan, ptrs, extra, out, probs, stream, op=None):
        pr = probs[0]
        offs, scores, totals, jumps = _solve_out(out, ("offs", "scores", "totals", "jumps"))
        plan.report(*op.pair_args(ptrs, probs), K, *drift_args(pr), pr["top_k"], pr["excl"], offs, scores, jumps, totals,
                    out["rep"], _i32(out["counts"]), stream=stream)

    def drep_decode(probs, host):
        raw = (_drift_results(probs, host), _rows(host, "rep", _native.SEGMENT_REPORT_DTYPE, probs), _counts(host))
        return [one_pair(raw, p) for p in range(len(probs))]

    def smooth_tail(out):
        import torch

        return (out["smooth"].view(torch.int32), out["knot"], out["seg"], _i32(out["counts"]))

    def smooth_issue(plan, ptrs, extra, out, probs, stream, op=None):
        pr = probs[0]
        offs, scores, totals, jumps = _solve_out(out, ("offs", "scores", "totals", "jumps"))
        plan.smooth(*op.pair_args(ptrs, probs), K, *drift_args(pr), pr["m"], pr["r"], pr["lam"], offs, scores, jumps, totals,
                    *smooth_tail(out), stream=stream)

    def smooth_decode(probs, host):
        raw = (_drift_results(probs, host), _rows(host, "smooth", np.int32, probs), _rows(host, "knot", np.uint8, probs),
               _rows(host, "seg", _native.SMOOTH_SEGMENT_DTYPE, probs), _counts(host))
        return [one_pair(raw, p) for p in range(len(probs))]

    report_out = lambda probs: (_solve_bytes(probs, DRIFT + (("rep", _native.SEGMENT_REPORT_BYTES),))
                                + [("counts", 4 * len(probs))])
    smooth_out = lambda probs: (_solve_bytes(probs, DRIFT + (("smooth", 4), ("knot", 1), ("seg", _native.SMOOTH_SEGMENT_BYTES)))
                                + [("counts", 4 * len(probs))])
    add("DriftPlan.align", "ffs_align_drift_batch", False, family("drift"), plan_dims=_window_dims,
        outputs=lambda probs: _solve_bytes(probs, DRIFT), issue=drift_issue, decode=_drift_results, model=fam["drift"][0],
        same=fam["drift"][1])
    add("DriftPlan.report", "ffs_align_drift_report_batch", True, family("drift_report"), plan_dims=_window_dims,
        outputs=report_out, issue=drep_issue, decode=drep_decode, model=fam["drift_report"][0], same=fam["drift_report"][1])
    add("DriftPlan.smooth", "ffs_align_drift_smooth_batch", False, family("smooth"), plan_dims=_window_dims,
        outputs=smooth_out, issue=smooth_issue, decode=smooth_decode, model=fam["smooth"][0], same=fam["smooth"][1])

    # -- DriftRangePlan
    def drange_args(probs):
        pr = probs[0]
        return _lags(probs) + (pr["p"], pr["s"], pr["q"])

    def drange_issue(plan, ptrs, extra, out, probs, stream, op=None):
        offs, scores, totals, jumps = _solve_out(out, ("offs", "scores", "totals", "jumps"))
        plan.align(*op.pair_args(ptrs, probs), K, *drange_args(probs), offs, scores, jumps, totals, stream=stream)

    def drange_smooth_issue(plan, ptrs, extra, out, probs, stream, op=None):
        pr = probs[0]
        offs, scores, totals, jumps = _solve_out(out, ("offs", "scores", "totals", "jumps"))
        plan.smooth(*op.pair_args(ptrs, probs), K, *drange_args(probs), pr["m"], pr["r"], pr["lam"], offs, scores, jumps,
                    totals, *smooth_tail(out), stream=stream)

    def drange_report_issue(plan, ptrs, extra, out, probs, stream, op=None):
        pr = probs[0]
        drange_issue(plan, ptrs, extra, out, probs, stream, op)
        offs, jumps = _solve_out(out, ("offs", "jumps"))
        plan.report(*op.pair_args(ptrs, probs), K, *_lags(probs), offs, jumps, pr["top_k"], pr["excl"], out["rep"],
                    _i32(out["counts"]), stream=stream)

    def drange_report_reference(pr):
        import piecewise_reference as pw

        return _once(("reference", id(pr)), lambda: (pr, pw.Reference(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], K, pr["lo"],
                                                                       pr["hi"])))[1]

    def drange_report_model(pr):
        """The drift solve's model and, on its path, the independent reference's segment records
        (tests/test_gpu_drift_range_report.py's comparison)."""
        import report_reference as rr

        solve = t_drange._model(pr)
        return solve, rr.segment_records(drange_report_reference(pr), solve[0], solve[2], pr["top_k"], pr["excl"])

    def drange_report_same(raw, want, pr):
        import report_reference as rr

        res, recs, counts = raw
        if not t_drange._same(res[0], want[0]):
            return ["drift solve"]
        return rr.compare(drange_report_reference(pr), want[1], recs[0], int(counts[0]), pr["top_k"], "segment")

    add("DriftRangePlan.align", "ffs_align_drift_range_batch", False, family("drift_range"), plan_dims=_drift_range_dims,
        outputs=lambda probs: _solve_bytes(probs, DRIFT), issue=drange_issue, decode=_drift_results,
        model=fam["drift_range"][0], same=fam["drift_range"][1])
    add("DriftRangePlan.smooth", "ffs_align_drift_range_smooth_batch", False, family("smooth_range"),
        plan_dims=_drift_range_dims, outputs=smooth_out, issue=drange_smooth_issue, decode=smooth_decode,
        model=fam["smooth_range"][0], same=fam["smooth_range"][1])
    def drange_report_set(n):
        """The drift range family's problems with reference levels whose mapped values 2 * level - 1 are integers, as
        ``piecewise_reference.Reference`` needs them."""
        return [dict(pr, r_lv=((0.0, 1.0), (-1.0, 2.0))[i % 2]) for i, pr in enumerate(_family_set("drift_range", n, top_k=3, excl=40))]

    add("DriftRangePlan.report", "ffs_drift_range_report_batch", True, drange_report_set,
        plan_dims=_drift_range_dims, outputs=report_out, issue=drange_report_issue, decode=drep_decode,
        model=drange_report_model, same=drange_report_same)
    for op in ops:  # every issue function gets its op (for ``pair_args``)
        op.issue = (lambda fn, op: lambda *a, **kw: fn(*a, op=op, **kw))(op.issue, op)
    return {op.name: op for op in ops}


OP_NAMES = (
    ["SplitPlan." + m for m in ("align", "align_report", "refine", "drift_refine", "cue_report", "cue_retime")]
    + ["QualityPlan.report", "MatchPlan.report", "SplitRangePlan.align", "SplitRangePlan.report"]
    + ["DriftPlan." + m for m in ("align", "report", "smooth")] + ["DriftRangePlan." + m for m in ("align", "smooth", "report")])
PLAN_CLASSES = ("SplitPlan", "QualityPlan", "MatchPlan", "SplitRangePlan", "DriftPlan", "DriftRangePlan")


def ops():
    """{name: Op}, in the order of ``OP_NAMES``."""
    return _once("ops", _ops)


def dump(x):
    """A model's result as bytes: two results are told apart by these."""
    return _tgl()._dump(x)
