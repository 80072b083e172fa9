"""The transform path's solve records at every plan length, pinned to the exact integer reference, with the dispatch
report of every solve (tests/transform_cases.py: 22 lengths, settings a-e, bit-packed / byte / float / mixed inputs, 1 to
12 candidates).

The raw-correlation sweeps of test_gpu_parity.py go through the raw-output mode of the last pass, which a solve never
runs, and the exact checks of test_gpu_exact.py reach the nominating instances at four plan lengths only; the A/B tests
cannot see what both of their sides share (twiddle tables, k_nominees' tile count, the m = d + N wrap, the tie rule at a
tile edge).  Here every solve (algorithm "fft") is held to
  * the exact records, candidate and pair, bit for bit (``check`` of test_gpu_exact.py without ``probs``: FFS_FLAG_AMBIGUOUS
    fails; the filter equals the window, so the pair record is the first maximal unfiltered candidate),
  * the dispatch report the case table expects (``Plan.dispatch_report``): a moved threshold cannot quietly take a case
    away from its kernel,
  * a healthy fp32 chain: |score_f32 - score| at a unique winner stays below the candidate's nominee margin
    5.96e-8 * log2 N * sqrt(R S) * |s|max * |r|max -- the condition under which nomination is safe at
    all; exact re-scoring would otherwise hide a damaged transform for as long as the true peak is still nominated.
    Each test prints its worst ratio per (mid family, last-pass family, first-pass family, input type) (-s).  Observed on
    an MI355X, worst over all lengths: single-transform path 0.14 (k_pass_c3), 0.26 (pruned), 0.22 (full k_pass_c) -- but
    0.83 for the silent far-end candidate (levels (0.5, 1)) at 2^24 windowless, bit-packed; block-segmented path 0.20
    (k_mid_seg_one, one and four accumulator rows), 0.21 (k_mid_seg_pipe).  The bound asserted is the margin itself (1.0).
Wall time is the CPU reference (8.7 s per windowless candidate at 2^24).  One plan at a time, closed before the next.
Need a real MI355X.
"""
import time

import numpy as np
import pytest

import transform_cases as tc
from test_gpu_exact import check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available()
    return t


def _pack(torch, probs, dtype):
    """DeviceBatch of host problems: bit-packed, 0/1 bytes, 0.0/1.0 float32, or a float64 reference with bit-packed
    candidates ("mixed")."""
    from ffsubsync_amd import _native
    from ffsubsync_amd.batch import DeviceBatch, _layout

    n_cand = len(probs[0][2])
    vecs = [v for p in probs for v in [p[1]] + list(p[2])]
    lens = np.array([v.size for v in vecs], np.int64).reshape(len(probs), 1 + n_cand)
    kinds = np.empty(lens.shape, object)
    kinds[:] = {"u1": "u1", "u8": "u8", "f32": "f32", "mixed": "u1"}[dtype]
    if dtype == "mixed":
        kinds[:, 0] = "f64"
    size = {"u1": lambda n: (n + 31) // 32 * 4, "u8": lambda n: n, "f32": lambda n: 4 * n, "f64": lambda n: 8 * n}
    nbytes = np.array([size[k](int(n)) for k, n in zip(kinds.ravel(), lens.ravel())], np.int64).reshape(lens.shape)
    offs, total = _layout(lens, nbytes)
    host = np.zeros(total, np.uint8)
    for v, o, k in zip(vecs, offs.ravel(), kinds.ravel()):
        b = (np.asarray(v) != 0).astype(np.uint8)
        raw = {"u1": lambda: np.packbits(b, bitorder="little"), "u8": lambda: b, "f32": lambda: b.astype(np.float32).view(np.uint8),
               "f64": lambda: b.astype(np.float64).view(np.uint8)}[k]()
        host[o:o + raw.size] = raw
    lo = np.array([[p[3][0]] + [lv[0] for lv in p[4]] for p in probs], np.float64)
    hi = np.array([[p[3][1]] + [lv[1] for lv in p[4]] for p in probs], np.float64)
    code = {"u1": _native.FFS_DTYPE_U1, "u8": _native.FFS_DTYPE_U8, "f32": _native.FFS_DTYPE_F32, "mixed": _native.FFS_DTYPE_U1}[dtype]
    return DeviceBatch(torch.from_numpy(host).cuda(), offs, lens, lo, hi, code,
                       ref_dtype=_native.FFS_DTYPE_F64 if dtype == "mixed" else None)


def _solve(torch, n, run, probs, pairs_in_flight):
    """(records, dispatch report) of one solve on a plan of its own (created under the run's environment)."""
    from ffsubsync_amd import batch

    db = _pack(torch, probs, run.dtype)
    al = batch.BatchAligner(n, len(run.idx), tc.window(n, run.setting), pairs_in_flight=pairs_in_flight, algorithm="fft")
    try:
        out = al.solve(db)
        report = al.plan.dispatch_report()
    finally:
        al.close()
    del db
    return out, report


def _margin_ratios(n, probs, want, out):
    """|score_f32 - score| / margin of every unique, unflagged winner."""
    ratios = []
    for i, (recs, _) in enumerate(want):
        _, ref, cands, rl, cl = probs[i]
        for j, r in enumerate(recs):
            c = out[0][i, j]
            if r["n_at_max"] != 1 or int(c["flags"]) & ~4 or not np.isfinite(r["score"]):
                continue
            ratios.append(abs(float(c["score_f32"]) - r["score"]) / tc.margin(n, ref.size, cands[j].size, rl, cl[j]))
    return ratios


@pytest.mark.parametrize("n", tc.LENGTHS)
def test_solve_records_at_plan_length(torch, monkeypatch, n):
    t0 = time.time()
    worst = {}
    for k, run in enumerate(tc.runs(n)):
        probs = tc.problems(n, run)
        want = tc.expected(n, run)
        with monkeypatch.context() as m:
            for name, value in tc.env(run.setting).items():
                m.setenv(name, value)  # (read when the plan is created)
            for pif in ((1, 2) if len(probs) > 1 else (1 + k % 2,)):
                tag = (n, run.setting, run.kind, run.dtype, run.idx, run.vset, pif)
                out, report = _solve(torch, n, run, probs, pif)
                assert report == tc.expected_dispatch(n, run, sub_batches=(len(probs) + pif - 1) // pif), (tag, report)
                check(out, want, tag)
                key = (report["mid_family"], report["last_family"], report["pass_a_family"], run.dtype)
                for ratio in _margin_ratios(n, probs, want, out):
                    worst[key] = max(worst.get(key, 0.0), ratio)
    torch.cuda.empty_cache()
    print("\nN=%d: %d solves, %.1f s; worst |score_f32 - score| / margin by (mid, last, pass A, type): %s"
          % (n, len(tc.runs(n)), time.time() - t0, {k: round(v, 4) for k, v in sorted(worst.items())}))
    assert worst and max(worst.values()) < 1.0, worst
