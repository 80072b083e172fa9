"""Multi-level float references on the run path (k_levels_sample, k_levels_bits, the threshold lists,
k_runs_chunk_flags_ml, k_runs_corr_ml, k_runs_pick) held bit for bit to the exact reference (tests/exact_reference.py)
on the case table tests/level_cases.py: every level set the analysis accepts, exact ties on tile edges, flat tops,
broken ties, the zero rule, winners at partial overlap, the negative-slice window, the 16-bit histogram cell at its
guard, plane lengths at the extraction's chunk edges, every candidate form, neighbours and sub-batches, and the plan's
list stride.  tests/test_level_cases_host.py asserts what the table claims (tie counts, cell values, where winners lie).

Records follow ``exact_check.check``: offset and flags equal, the score bit-identical except for the sign of an exact
0.0, the pair record the first maximal candidate after the offset filter.  Every run-path call also asserts
``plan.runs_stats()``, so a silent fallback to the transforms cannot pass.  Records the transforms wrote (a sub-batch
with a reference the analysis refuses, a cell at the guard, candidates that are neither bits nor lists) follow
tests/test_gpu_exact.py::test_float_references' rule for amplitude levels (``level_cases.transform_rule_bad``).
Need a real MI355X.
"""
import numpy as np
import pytest

import exact_reference as er
import level_cases as lc
from exact_check import check

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available()
    return t


def _batch(torch, probs, ref_dtype=F64, form="bits"):
    """DeviceBatch of case-table problems: float references of ``ref_dtype``; candidates bit-packed ("bits"), as
    caller-owned boundary lists made from those bits ("lists"), as 0/1 bytes ("u8") or as float64 level values ("f64")."""
    from ffsubsync_amd import _native
    from ffsubsync_amd.batch import DeviceBatch, _layout

    n_cand = len(probs[0][2])
    assert all(len(p[2]) == n_cand for p in probs)
    lens = np.array([[p[1].size] + [c.size for c in p[2]] for p in probs], np.int64)
    nbytes = lens.copy()
    nbytes[:, 0] = lens[:, 0] * np.dtype(ref_dtype).itemsize
    nbytes[:, 1:] = {"u8": lens[:, 1:], "f64": lens[:, 1:] * 8}.get(form, (lens[:, 1:] + 31) // 32 * 4)
    offs, total = _layout(lens, nbytes)
    host = np.zeros(total, np.uint8)
    lo, hi = np.zeros(lens.shape), np.ones(lens.shape)
    for p, (name, ref, cands, levels) in enumerate(probs):
        r = np.ascontiguousarray(ref, dtype=ref_dtype)
        assert np.array_equal(r.astype(F64), np.asarray(ref, F64)), name  # the type holds the levels exactly
        host[offs[p, 0]: offs[p, 0] + r.nbytes] = r.view(np.uint8)
        lo[p, 0], hi[p, 0] = float(r.min()), float(r.max())  # (a float vector's lo / hi bound its samples)
        for j, (c, lv) in enumerate(zip(cands, levels)):
            if form == "u8":
                raw = (np.asarray(c) != 0).astype(np.uint8)
            elif form == "f64":
                raw = np.where(np.asarray(c) != 0, lv[1], lv[0]).astype(F64).view(np.uint8)
            else:
                raw = np.packbits((np.asarray(c) != 0).astype(np.uint8), bitorder="little")
            host[offs[p, 1 + j]: offs[p, 1 + j] + raw.size] = raw
            lo[p, 1 + j], hi[p, 1 + j] = (min(lv), max(lv)) if form == "f64" else lv
    data = torch.from_numpy(host).cuda()
    rd = _native.FFS_DTYPE_F64 if ref_dtype == F64 else _native.FFS_DTYPE_F32
    if form in ("bits", "u8", "f64"):
        cd = {"bits": _native.FFS_DTYPE_U1, "u8": _native.FFS_DTYPE_U8, "f64": _native.FFS_DTYPE_F64}[form]
        return DeviceBatch(data, offs, lens, lo, hi, cd, ref_dtype=rd)
    # caller-owned lists of the candidates (ffs_runs_from_bits_batch), the float references stay where they are
    cap = 32768
    block = (_native.runs_list_bytes(cap) + 63) // 64 * 64
    n_list = len(probs) * n_cand
    lists = torch.empty(n_list * block, dtype=torch.uint8, device=data.device)
    l_offs = (np.arange(n_list, dtype=np.int64) * block).reshape(len(probs), n_cand)
    _native.runs_from_bits_batch(data.data_ptr() + offs[:, 1:].ravel().astype(np.uint64), lens[:, 1:].ravel(),
                                 lists.data_ptr() + l_offs.ravel().astype(np.uint64), np.full(n_list, cap, dtype=np.int64))
    base = (data.numel() + 63) // 64 * 64
    both = torch.cat([data, torch.zeros(base - data.numel(), dtype=torch.uint8, device=data.device), lists])
    offs2 = np.concatenate([offs[:, :1], l_offs + base], axis=1)
    return DeviceBatch(both, offs2, lens, lo, hi, _native.FFS_DTYPE_RUNS, ref_dtype=rd)


def _aligner(db, max_off, algorithm="runs", pairs_in_flight=4, n_fft=None):
    from ffsubsync_amd import batch

    n_fft = db.required_fft_length(max_off) if n_fft is None else n_fft
    assert n_fft >= 4096, n_fft  # (shorter plans solve every lag in k_direct)
    return batch.BatchAligner(n_fft, db.n_cand, max_off, pairs_in_flight=pairs_in_flight, algorithm=algorithm)


def _solve(db, max_off, algorithm="runs", pairs_in_flight=4, n_fft=None):
    """(records, runs_stats) of one call on a fresh plan."""
    al = _aligner(db, max_off, algorithm, pairs_in_flight, n_fft)
    try:
        out = al.solve(db)
        return out, al.plan.runs_stats()
    finally:
        al.close()


def _want(probs, max_off):
    return [er.solve(np.asarray(p[1], F64), p[2], None, p[3], max_off, max_off) for p in probs]


def _on_the_run_path(st):
    assert st[0] == 1 and st[2] == 0, st  # the run-boundary path, no sub-batch through the transforms


def _run_exact(torch, probs, max_off, tag, ref_dtype=F64, form="bits", pairs_in_flight=4, want=None):
    out, st = _solve(_batch(torch, probs, ref_dtype, form), max_off, "runs", pairs_in_flight)
    _on_the_run_path(st)
    return check(out, _want(probs, max_off) if want is None else want, tag)


def _transform_rule(out, probs, max_off, rows, tag):
    """Records the transforms wrote: each offset in the lag set, its exact score within the fp64 summation bound of the
    maximum; the pair record is the first maximal candidate of the device's own records after the filter."""
    cres, pres = out
    bad = []
    for i in rows:
        name, ref, cands, levels = probs[i]
        for j, (c, lv) in enumerate(zip(cands, levels)):
            why = lc.transform_rule_bad(ref, c, lv, max_off, int(cres[i, j]["offset"]))
            if why:
                bad.append((tag, name, j, why))
        dev = [dict(score=float(c["score"]), offset=int(c["offset"]), flags=0) for c in cres[i]]
        win = er.pair(dev, max_off)
        if int(pres[i]["best_cand"]) != win["best_cand"] or (win["best_cand"] >= 0 and int(pres[i]["offset"]) != win["offset"]):
            bad.append((tag, name, "pair", int(pres[i]["best_cand"]), win))
    assert not bad, (len(bad), bad[:6])


SET_CASES = [(ls, F64) for ls in lc.ACCEPTED] + [(ls, F32) for ls in lc.ACCEPTED if ls.dtype == F32]


@pytest.mark.parametrize("max_off", [None, 6000, 3])
@pytest.mark.parametrize("ls,ref_dtype", SET_CASES, ids=lambda x: x.name if isinstance(x, lc.LevelSet) else np.dtype(x).name)
def test_level_sets_and_windows(torch, ls, ref_dtype, max_off):
    """Every accepted level set (divisors 1 .. 4, multiplicities up to 8, sum m up to 19, a vanishing base, levels
    outside [0, 1], float32 where the type holds the levels) on the periodic-tie and flat-top families: windowless (three
    tiles and more: k_runs_pick), one tile, seven lags."""
    probs = lc.periodic_ties(ls, max_off) + lc.flat_tops(ls)
    ties = _run_exact(torch, probs, max_off, (ls.name, max_off), ref_dtype)
    assert ties >= lc.min_tie_records(ls, max_off), ties


@pytest.mark.parametrize("max_off", [None, 6000])
def test_broken_ties(torch, max_off):
    """One reference sample of the plane with the smallest m_k lifts the SMALLEST tied lag by m_k counts: the record
    must move there from the largest tied lag -- every level set in one call, beside its unbroken twin."""
    probs = []
    for ls in lc.ACCEPTED:
        broken, unbroken, _ = lc.broken_tie(ls, max_off)
        probs += [broken, unbroken]
    ties = _run_exact(torch, probs, max_off, ("broken", max_off), pairs_in_flight=8)
    assert ties >= 2 * len(lc.ACCEPTED), ties  # the unbroken twins


@pytest.mark.parametrize("max_off", [None, 6000, 3])
def test_zero_rule_relatives(torch, max_off):
    """2 lam0 - 1 = 0 with a candidate whose lower level maps to 0: the score is M11 k11 alone; an all-zero candidate
    scores exactly 0.0 at every lag (the window's largest lag wins); equal best scores across candidates."""
    _run_exact(torch, lc.zero_rule(), max_off, ("zero", max_off))


@pytest.mark.parametrize("name", ["weighted_label_0", "steps_8_1_8", "base_zero"])
def test_negative_slice_window(torch, name):
    """max_offset_samples past N - 1 - S: the few lags Python's negative slice leaves, at the far negative end (on a plan
    of the reference's own transform length: the shortest plan for such a window would be the direct kernel's)."""
    probs, windows = lc.negative_slice(lc.BY_NAME[name])
    for w in windows:
        out, st = _solve(_batch(torch, probs), w, "runs", n_fft=er.orc.fft_length(lc.NEG_R, lc.NEG_S))
        _on_the_run_path(st)
        check(out, _want(probs, w), (name, w))


@pytest.mark.parametrize("name", lc.PARTIAL_SETS)
def test_partial_overlap_winners(torch, name):
    """64 windowless problems whose winners hang over the reference's start or end (R < S and R > S, candidate levels
    (0, 1), (0, 1/1.001) and (-.5, 1.25)): Mx1 moves by up to sum m_k per lag there and the prefilter's edge term is
    refreshed every four lags only -- the margin must carry sum m_k (estep_w, count_max)."""
    _run_exact(torch, lc.partial_overlap(lc.BY_NAME[name]), None, name, pairs_in_flight=16)


def test_cell_guard(torch):
    """sum_k m_k min(n_p, n_q) = 32760: the run path, with cells at +9n and -9(n-1), the extreme 16-bit values of the
    packed halves.  32778: k_runs_chunk_flags_ml sends the sub-batch through the transforms."""
    below, at = lc.cell_guard(3640), lc.cell_guard(3642)
    _run_exact(torch, [below], None, "below the guard")
    out, st = _solve(_batch(torch, [at]), None, "runs")
    assert st == (1, 1, 1), st
    _transform_rule(out, [at], None, [0], "at the guard")


@pytest.mark.parametrize("max_off", [None, 6000])
def test_candidate_forms(torch, max_off):
    """The same problems with bit-packed candidates and with caller-owned boundary lists (one alternating every sample:
    its edge windows meet more than RUNS_EDGE entries): equal, exact records.  Candidates as bytes or float64 values
    take the transforms (the run path reads bits and lists only): the transform rule."""
    ls = lc.BY_NAME["weighted_label_0"]
    probs = lc.periodic_ties(ls, max_off) + [lc.alternating_list_candidate(ls), lc.small_problem(ls, 1)]
    want = _want(probs, max_off)
    got = {}
    for form in ("bits", "lists"):
        got[form], st = _solve(_batch(torch, probs, F64, form), max_off, "runs")
        _on_the_run_path(st)
        check(got[form], want, (form, max_off))
    for f in ("score", "offset", "flags"):
        assert np.array_equal(got["bits"][0][f], got["lists"][0][f]), f
    for form in ("u8", "f64"):
        out, st = _solve(_batch(torch, probs, F64, form), max_off, "runs")
        assert st[0] == 0, (form, st)
        _transform_rule(out, probs, max_off, range(len(probs)), (form, max_off))


def test_neighbours_and_sub_batches(torch):
    """One problem of every level set in one call, permuted, with a five-level pair and a float32-rounded `weighted`
    pair among them, under "auto" at pairs_in_flight 1, 2 and 64: every run-path pair is exact at every setting, and
    only the sub-batches that hold an odd pair go through the transforms (runs_stats)."""
    max_off = 3000
    probs = [lc.small_problem(ls, k) for k, ls in enumerate(lc.ACCEPTED)]
    probs += [lc.odd_pair(lc.BY_NAME["five_levels"], 0), lc.odd_pair(lc.BY_NAME["weighted_rounded_f32"], 1)]
    order = np.random.RandomState(31).permutation(len(probs))
    probs = [probs[i] for i in order]
    odd = [i for i, p in enumerate(probs) if p[0].startswith("odd_")]
    want = [er.solve(np.asarray(p[1], F64), p[2], None, p[3], max_off, max_off) if i not in odd else None
            for i, p in enumerate(probs)]
    n_fft = None
    # (bit-packed candidates at every setting; caller-owned lists at 2: a sub-batch that takes the transforms after all
    # expands its list candidates there)
    for form, pif in (("bits", 1), ("bits", 2), ("bits", 64), ("lists", 2)):
        db = _batch(torch, probs, F64, form)
        n_fft = db.required_fft_length(max_off) if n_fft is None else n_fft
        out, st = _solve(db, max_off, "auto", pif, n_fft)
        through = sorted({i // pif for i in odd})
        assert st == (1, (len(probs) + pif - 1) // pif, len(through)), (form, pif, st)
        fft_rows = [i for i in range(len(probs)) if i // pif in through]
        run_rows = [i for i in range(len(probs)) if i // pif not in through]
        check((out[0][run_rows], out[1][run_rows]), [want[i] for i in run_rows], ("neighbours", form, pif))
        _transform_rule(out, probs, max_off, fft_rows, ("neighbours", form, pif))


@pytest.mark.parametrize("name,ref_dtype", [("weighted_label_0", F64), ("dyadic_f32_1_1_2", F32)])
def test_plane_tails(torch, name, ref_dtype):
    """Reference lengths around k_levels_bits' 16 384 / 1024 / 128-sample steps, the last samples (top, lam0, top)
    deciding lags of the far end: the `w < pw` stores, the l0 padding past n, the chunk edges."""
    _run_exact(torch, lc.plane_tails(lc.BY_NAME[name]), None, name, ref_dtype, pairs_in_flight=8)


def _one_candidate(p, j=1):
    return (p[0], p[1], [p[2][j]], [p[3][j]])


def test_dense_threshold_planes_grow_the_stride_once(torch):
    """Planes that alternate every sample (about 9000 boundaries a list against the initial stride of 4096): the call
    is solved again at the longer stride, exact; a repeat of it and of the small call before it leave the workspace
    unchanged."""
    ls = lc.BY_NAME["weighted_label_0"]
    small = [_one_candidate(lc.small_problem(ls, k)) for k in range(8)]
    dense = lc.dense_planes()
    db_small, db_dense = _batch(torch, small), _batch(torch, dense)
    want_small, want_dense = _want(small, None), _want(dense, None)
    al = _aligner(db_dense, None, "runs", pairs_in_flight=64, n_fft=max(db_small.required_fft_length(None), db_dense.required_fft_length(None)))
    try:
        check(al.solve(db_small), want_small, "small")
        before = al.plan.workspace_bytes
        check(al.solve(db_dense), want_dense, "dense")
        after = al.plan.workspace_bytes
        assert after > before, (before, after)
        check(al.solve(db_dense), want_dense, "dense again")
        check(al.solve(db_small), want_small, "small again")
        assert al.plan.workspace_bytes == after
        assert al.plan.runs_stats() == (4, 4, 0)
    finally:
        al.close()


def test_long_caller_owned_lists_leave_the_stride_alone(torch):
    """A sparse multi-level reference against caller-owned candidate lists of more than 4096 entries: no plan-owned list
    is near its stride, so the call is solved once and the workspace stays what a small call of the same shape left
    (k_runs_chunk_flags_ml counted every candidate's entries into `longest`: the host discarded the solve, grew the
    stride four-fold and solved again, twice, keeping the larger workspace)."""
    long_probs = lc.long_candidate_lists()
    ls = lc.BY_NAME["weighted_label_0"]
    R, S = long_probs[0][1].size, long_probs[0][2][0].size
    small = [lc.small_problem(ls, 40 + k, R, S) for k in range(len(long_probs))]
    small = [(p[0], p[1], p[2][:2], p[3][:2]) for p in small]
    db_small, db_long = _batch(torch, small, form="lists"), _batch(torch, long_probs, form="lists")
    al = _aligner(db_long, None, "runs", pairs_in_flight=4)
    try:
        check(al.solve(db_small), _want(small, None), "small lists")
        before = al.plan.workspace_bytes
        check(al.solve(db_long), _want(long_probs, None), "long lists")
        assert al.plan.workspace_bytes == before, (before, al.plan.workspace_bytes)
        assert al.plan.runs_stats() == (2, 2, 0)
    finally:
        al.close()
