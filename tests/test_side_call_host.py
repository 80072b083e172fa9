"""Host tests of ``ffsubsync_amd.side_call``, the helper every side entry point is built on, and of what the fold of
the sixteen side modules onto it must not move: the plan dims of every ``_get_plan``, the order and text of every
refusal, and the host derivation of psr, margin and the gains.

Every literal table below (``PLAN_DIMS``, ``BATCH_CHECK``, ``REFUSALS``, ``PIECES``, ``SEGMENTS``) was recorded by
running the functions of the commit before the fold -- each module's own ``_get_plan``, ``_check_batch``, entry point
and ``from_record`` -- on the inputs this file builds.  The ``BlockCall`` arithmetic is computed by hand.  No GPU."""
import dataclasses
import math
from types import SimpleNamespace

import numpy as np
import pytest

from ffsubsync_amd import (_native, cue_report, cue_retime, cut_align, cut_report, drift_align, drift_range,
                           drift_range_report, drift_range_smooth, drift_refine, drift_report, drift_smooth, match, quality,
                           side_call, split_align, split_refine, split_report)

NAN, INF = math.nan, math.inf

# ---------------------------------------------------------------------------------------------------------------------
# pairs_for_budget, through every _get_plan

SHAPES = {
    "smallest": dict(max_blocks=1, max_lags=2, max_samples=256, n_pairs=1),
    "two_hours": dict(max_blocks=704, max_lags=120000, max_samples=720000, n_pairs=300),
    "cap_binds": dict(max_blocks=1, max_lags=2, max_samples=256, n_pairs=10000),
    "full_range": dict(max_blocks=704, max_lags=1440000, max_samples=720000, n_pairs=300),  # the budget binds everywhere
}
MAX_STEP = 2
_block = lambda mod, s, *more: mod._get_plan(s["n_pairs"], s["max_blocks"], s["max_lags"], s["max_samples"], *more, None)
GET_PLANS = {
    "split_align": (split_align, _block),
    "split_align/report": (split_align, lambda mod, s: mod._get_plan(s["n_pairs"], s["max_blocks"], s["max_lags"],
                                                                     s["max_samples"], None, True)),
    "cut_align": (cut_align, _block),
    "cut_report": (cut_report, _block),
    "drift_align": (drift_align, _block),
    "drift_report": (drift_report, _block),
    "drift_smooth": (drift_smooth, _block),
    "drift_range": (drift_range, lambda mod, s: _block(mod, s, MAX_STEP)),
    "drift_range_smooth": (drift_range_smooth, lambda mod, s: _block(mod, s, MAX_STEP)),
    "drift_range_report": (drift_range_report, lambda mod, s: _block(mod, s, MAX_STEP)),
    "quality": (quality, lambda mod, s: mod._get_plan(s["n_pairs"], s["max_lags"], s["max_samples"], None)),
    "match": (match, lambda mod, s: mod._get_plan(s["n_pairs"], s["max_lags"], s["max_samples"], s["n_pairs"] + 1, None)),
    "split_refine": (split_refine, lambda mod, s: mod._get_plan(s["n_pairs"])),
    "drift_refine": (drift_refine, lambda mod, s: mod._get_plan(s["n_pairs"])),
    "cue_report": (cue_report, lambda mod, s: mod._get_plan(s["n_pairs"])),
}
# (dims handed to the module's plan cache, role) per _get_plan and shape
PLAN_DIMS = {
    ("cue_report", "cap_binds"): ((256, 1, 2, 1), None),
    ("cue_report", "full_range"): ((256, 1, 2, 1), None),
    ("cue_report", "smallest"): ((1, 1, 2, 1), None),
    ("cue_report", "two_hours"): ((256, 1, 2, 1), None),
    ("cut_align", "cap_binds"): ((256, 1, 2, 256), None),
    ("cut_align", "full_range"): ((93, 704, 1440000, 720000), None),
    ("cut_align", "smallest"): ((1, 1, 2, 256), None),
    ("cut_align", "two_hours"): ((256, 704, 120000, 720000), None),
    ("cut_report", "cap_binds"): ((256, 1, 2, 256), "report"),
    ("cut_report", "full_range"): ((69, 704, 1440000, 720000), "report"),
    ("cut_report", "smallest"): ((1, 1, 2, 256), "report"),
    ("cut_report", "two_hours"): ((256, 704, 120000, 720000), "report"),
    ("drift_align", "cap_binds"): ((256, 1, 2, 256), None),
    ("drift_align", "full_range"): ((4, 704, 1440000, 720000), None),
    ("drift_align", "smallest"): ((1, 1, 2, 256), None),
    ("drift_align", "two_hours"): ((56, 704, 120000, 720000), None),
    ("drift_range", "cap_binds"): ((256, 1, 2, 256, 2), None),
    ("drift_range", "full_range"): ((31, 704, 1440000, 720000, 2), None),
    ("drift_range", "smallest"): ((1, 1, 2, 256, 2), None),
    ("drift_range", "two_hours"): ((256, 704, 120000, 720000, 2), None),
    ("drift_range_report", "cap_binds"): ((256, 1, 2, 256, 2), None),
    ("drift_range_report", "full_range"): ((23, 704, 1440000, 720000, 2), None),
    ("drift_range_report", "smallest"): ((1, 1, 2, 256, 2), None),
    ("drift_range_report", "two_hours"): ((256, 704, 120000, 720000, 2), None),
    ("drift_range_smooth", "cap_binds"): ((256, 1, 2, 256, 2), None),
    ("drift_range_smooth", "full_range"): ((31, 704, 1440000, 720000, 2), None),
    ("drift_range_smooth", "smallest"): ((1, 1, 2, 256, 2), None),
    ("drift_range_smooth", "two_hours"): ((256, 704, 120000, 720000, 2), None),
    ("drift_refine", "cap_binds"): ((256, 1, 2, 1), None),
    ("drift_refine", "full_range"): ((256, 1, 2, 1), None),
    ("drift_refine", "smallest"): ((1, 1, 2, 1), None),
    ("drift_refine", "two_hours"): ((256, 1, 2, 1), None),
    ("drift_report", "cap_binds"): ((256, 1, 2, 256), None),
    ("drift_report", "full_range"): ((4, 704, 1440000, 720000), None),
    ("drift_report", "smallest"): ((1, 1, 2, 256), None),
    ("drift_report", "two_hours"): ((54, 704, 120000, 720000), None),
    ("drift_smooth", "cap_binds"): ((256, 1, 2, 256), None),
    ("drift_smooth", "full_range"): ((4, 704, 1440000, 720000), None),
    ("drift_smooth", "smallest"): ((1, 1, 2, 256), None),
    ("drift_smooth", "two_hours"): ((54, 704, 120000, 720000), None),
    ("match", "cap_binds"): ((1024, 2, 256, 10001), None),
    ("match", "full_range"): ((124, 1440000, 720000, 301), None),
    ("match", "smallest"): ((1, 2, 256, 2), None),
    ("match", "two_hours"): ((300, 120000, 720000, 301), None),
    ("quality", "cap_binds"): ((1024, 2, 256), None),
    ("quality", "full_range"): ((124, 1440000, 720000), None),
    ("quality", "smallest"): ((1, 2, 256), None),
    ("quality", "two_hours"): ((300, 120000, 720000), None),
    ("split_align", "cap_binds"): ((256, 1, 2, 256), None),
    ("split_align", "full_range"): ((5, 704, 1440000, 720000), None),
    ("split_align", "smallest"): ((1, 1, 2, 256), None),
    ("split_align", "two_hours"): ((69, 704, 120000, 720000), None),
    ("split_align/report", "cap_binds"): ((256, 1, 2, 256), "report"),
    ("split_align/report", "full_range"): ((2, 704, 1440000, 720000), "report"),
    ("split_align/report", "smallest"): ((1, 1, 2, 256), "report"),
    ("split_align/report", "two_hours"): ((24, 704, 120000, 720000), "report"),
    ("split_refine", "cap_binds"): ((256, 1, 2, 1), None),
    ("split_refine", "full_range"): ((256, 1, 2, 1), None),
    ("split_refine", "smallest"): ((1, 1, 2, 1), None),
    ("split_refine", "two_hours"): ((256, 1, 2, 1), None),
}


def requested_dims(name, shape, monkeypatch):
    """What ``name``'s ``_get_plan`` asks its own plan cache for at ``shape``."""
    mod, call = GET_PLANS[name]
    seen = []
    monkeypatch.setattr(mod._plans, "get", lambda *dims, role=None: seen.append((dims, role)))
    call(mod, SHAPES[shape])
    assert len(seen) == 1
    dims, role = seen[0]
    assert all(type(d) is int for d in dims), dims
    return dims, role


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("name", sorted(GET_PLANS))
def test_every_get_plan_asks_for_the_dims_it_asked_for_before_the_fold(name, shape, monkeypatch):
    assert requested_dims(name, shape, monkeypatch) == PLAN_DIMS[name, shape]


def test_pairs_for_budget_is_the_one_expression():
    assert side_call.pairs_for_budget(300, 704 * (120000 + 64) * 2.2 + 1) == int((12 << 30) // (704 * (120000 + 64) * 2.2 + 1))
    assert side_call.pairs_for_budget(5, 1.0) == 5
    assert side_call.pairs_for_budget(10 ** 6, 1.0) == 256
    assert side_call.pairs_for_budget(10 ** 6, 25, cap=1024, budget=2 << 30) == 1024
    assert side_call.pairs_for_budget(0, 1.0) == 1
    assert side_call.pairs_for_budget(300, float(1 << 40)) == 1  # one pair even when one pair is over the budget
    assert type(side_call.pairs_for_budget(300, 1e9)) is int


def test_the_three_no_workspace_plans_stay_separate(monkeypatch):
    caches = [split_refine._plans, drift_refine._plans, cue_report._plans]
    assert len({id(c) for c in caches}) == 3
    assert all(c.plan_class is _native.SplitPlan for c in caches)


# ---------------------------------------------------------------------------------------------------------------------
# BlockCall arithmetic (hand-computed)

LENS = (1, 255, 256, 257, 32768 + 1)


def fake_batch(n=2, dtype=None, ref_dtype=None, n_cand=1, hi=1.0, lens=None):
    """A stand-in for ``batch.DeviceBatch`` with what the host checks read (``tests/test_cue_report_host.py``)."""
    dtype = _native.FFS_DTYPE_U1 if dtype is None else dtype
    return SimpleNamespace(n_pairs=n, n_cand=n_cand, dtype=dtype, ref_dtype=ref_dtype,
                           lens=np.full((n, 2), 100, np.int64) if lens is None else np.asarray(lens, np.int64),
                           lo=np.zeros((n, 2)), hi=np.full((n, 2), hi))


@pytest.fixture
def block_call(monkeypatch):
    """A ``BlockCall`` over subtitle lengths ``LENS`` (references 1000 samples longer) at 256 samples per block, with a
    stand-in for torch that keeps 'device' tensors as the numpy arrays they were made from."""
    fake_torch = SimpleNamespace(from_numpy=lambda a: SimpleNamespace(to=lambda dev: (a, dev)))
    monkeypatch.setattr(_native, "require_gpu", lambda: fake_torch)
    lens = np.array([[s + 1000, s] for s in LENS])
    batch = fake_batch(n=len(LENS), lens=lens)
    batch.data = SimpleNamespace(device="dev0")
    batch.pair_arrays = lambda: ("pair", "arrays")
    return side_call.BlockCall(batch, 256)


def test_block_call_counts_blocks_by_hand(block_call):
    c = block_call
    assert (c.k, c.n, c.max_b, c.dev) == (256, 5, 129, "dev0")
    assert c.n_blocks.tolist() == [1, 1, 1, 2, 129]
    assert c.sub_len.tolist() == list(LENS) and c.ref_len.tolist() == [s + 1000 for s in LENS]
    assert c.sub_len.dtype == c.ref_len.dtype == c.n_blocks.dtype == np.int64
    assert c.pair_arrays() == ("pair", "arrays")


def test_block_call_reads_0_1_bytes_through_to_bits(monkeypatch):
    monkeypatch.setattr(_native, "require_gpu", lambda: None)
    bits = fake_batch()
    bits.data = SimpleNamespace(device="dev1")
    raw = fake_batch(dtype=_native.FFS_DTYPE_U8)
    raw.to_bits = lambda: bits
    assert side_call.BlockCall(raw, 256).batch is bits
    assert side_call.BlockCall(bits, 256).batch is bits


def test_lag_dims_by_hand(block_call):
    lo = np.array([-5, 0, 7, -300, -32768], np.int64)
    hi = np.array([5, 0, 9, 1256, 33767], np.int64)
    # lags: 11, 1, 3, 1557, 66536; samples: the longest vector of either side, the reference of 32769 + 1000
    assert block_call.lag_dims(lo, hi) == (66536, 33769)
    assert all(type(x) is int for x in block_call.lag_dims(lo, hi))


def test_place_pads_exact_rows_and_refuses_short_and_long_ones(block_call):
    what = lambda p, size, blocks: "pair %d: %d block offsets, %d blocks" % (p, size, blocks)
    rows = [[7], [8], [9], [10, 11], list(range(129))]
    flags = [[True] * len(row) for row in rows]
    (flat, dev), (flat_flags, _) = block_call.place(what, (rows, np.int32), (flags, np.uint8))
    assert dev == "dev0" and flat.dtype == np.int32 and flat.shape == (5 * 129,)
    grid = flat.reshape(5, 129)
    assert grid[:4, :3].tolist() == [[7, 0, 0], [8, 0, 0], [9, 0, 0], [10, 11, 0]]
    assert not grid[:4, 3:].any() and grid[4].tolist() == list(range(129))
    assert flat_flags.dtype == np.uint8 and flat_flags.reshape(5, 129)[:4, :3].tolist() == [[1, 0, 0]] * 3 + [[1, 1, 0]]
    assert flat_flags.reshape(5, 129)[4].all() and int(flat_flags.sum()) == 5 + 129
    short = rows[:3] + [[10]] + rows[4:]
    with pytest.raises(ValueError) as e:
        block_call.place(what, (short, np.int32))
    assert str(e.value) == "pair 3: 1 block offsets, 2 blocks"
    long = rows[:4] + [list(range(130))]
    with pytest.raises(ValueError) as e:
        block_call.place(what, (long, np.int32))
    assert str(e.value) == "pair 4: 130 block offsets, 129 blocks"
    # rows are checked pair by pair: a wrong second row of pair 3 is named before a wrong first row of pair 4
    with pytest.raises(ValueError) as e:
        block_call.place(what, (long, np.int32), (short, np.uint8))
    assert str(e.value) == "pair 3: 1 block offsets, 2 blocks"
    # a caller that takes [n_pairs, >= max_b] arrays has the rows clipped first: long rows pass, short ones do not
    (flat, _), = block_call.place(what, (long, np.uint8), clip=True)
    assert flat.dtype == np.uint8 and flat.reshape(5, 129)[4].tolist() == list(range(129))
    with pytest.raises(ValueError) as e:
        block_call.place(what, (short, np.uint8), clip=True)
    assert str(e.value) == "pair 3: 1 block offsets, 2 blocks"


# ---------------------------------------------------------------------------------------------------------------------
# the batch check under its three names (and quality's, which also takes boundary lists)

BATCH_FAULTS = {
    "two_candidates": dict(n_cand=2),
    "float_reference": dict(ref_dtype=_native.FFS_DTYPE_F64),
    "float32_vectors": dict(dtype=_native.FFS_DTYPE_F32),
    "mixed_types": dict(dtype=_native.FFS_DTYPE_U8, ref_dtype=_native.FFS_DTYPE_U1),
    "boundary_lists": dict(dtype=_native.FFS_DTYPE_RUNS),
    "empty": dict(lens=[[100, 100], [0, -3]]),
    "nan_level": dict(hi=NAN),
}
BATCH_CHECKS = {
    "split_align_batch": lambda b: side_call.check_two_level_batch(b, "split_align_batch"),
    "cue_report_batch": lambda b: side_call.check_two_level_batch(b, "cue_report_batch", float_ref_message=True),
    "retime_batch": lambda b: side_call.check_two_level_batch(b, "retime_batch", float_ref_message=True),
    "quality_batch": lambda b: side_call.check_two_level_batch(b, "quality_batch", float_ref_message=True, lists=True),
}
ONE_CANDIDATE = "%s needs one candidate per pair (DeviceBatch.select_candidates)"
TWO_LEVEL = "%s needs two-level vectors: bit-packed (FFS_DTYPE_U1) or 0/1 bytes (FFS_DTYPE_U8)"
ONE_TYPE = ("quality_batch needs two-level vectors of one type: bit-packed (FFS_DTYPE_U1), 0/1 bytes (FFS_DTYPE_U8) or "
            "boundary lists (FFS_DTYPE_RUNS)")
FLOAT_REFERENCE = "%s needs a two-level reference: a multi-level float reference (FFS_DTYPE_%s) is not supported"
NO_SPEECH = ("cannot align empty speech data (reference length=%d, subtitle length=%d); the reference or subtitles may "
             "contain no detectable speech")
FINITE_LEVELS = "two-level vectors need finite levels"
BATCH_CHECK = {
    ("cue_report_batch", "boundary_lists"): TWO_LEVEL % "cue_report_batch",
    ("cue_report_batch", "empty"): NO_SPEECH % (0, 0),
    ("cue_report_batch", "float32_vectors"): FLOAT_REFERENCE % ("cue_report_batch", "F32"),
    ("cue_report_batch", "float_reference"): FLOAT_REFERENCE % ("cue_report_batch", "F64"),
    ("cue_report_batch", "mixed_types"): TWO_LEVEL % "cue_report_batch",
    ("cue_report_batch", "nan_level"): FINITE_LEVELS,
    ("cue_report_batch", "two_candidates"): ONE_CANDIDATE % "cue_report_batch",
    ("quality_batch", "boundary_lists"): None,
    ("quality_batch", "empty"): NO_SPEECH % (0, 0),
    ("quality_batch", "float32_vectors"): FLOAT_REFERENCE % ("quality_batch", "F32"),
    ("quality_batch", "float_reference"): FLOAT_REFERENCE % ("quality_batch", "F64"),
    ("quality_batch", "mixed_types"): ONE_TYPE,
    ("quality_batch", "nan_level"): FINITE_LEVELS,
    ("quality_batch", "two_candidates"): ONE_CANDIDATE % "quality_batch",
    ("retime_batch", "boundary_lists"): TWO_LEVEL % "retime_batch",
    ("retime_batch", "empty"): NO_SPEECH % (0, 0),
    ("retime_batch", "float32_vectors"): FLOAT_REFERENCE % ("retime_batch", "F32"),
    ("retime_batch", "float_reference"): FLOAT_REFERENCE % ("retime_batch", "F64"),
    ("retime_batch", "mixed_types"): TWO_LEVEL % "retime_batch",
    ("retime_batch", "nan_level"): FINITE_LEVELS,
    ("retime_batch", "two_candidates"): ONE_CANDIDATE % "retime_batch",
    ("split_align_batch", "boundary_lists"): TWO_LEVEL % "split_align_batch",
    ("split_align_batch", "empty"): NO_SPEECH % (0, -3),
    ("split_align_batch", "float32_vectors"): TWO_LEVEL % "split_align_batch",
    ("split_align_batch", "float_reference"): TWO_LEVEL % "split_align_batch",
    ("split_align_batch", "mixed_types"): TWO_LEVEL % "split_align_batch",
    ("split_align_batch", "nan_level"): FINITE_LEVELS,
    ("split_align_batch", "two_candidates"): ONE_CANDIDATE % "split_align_batch",
}


def refusal(call):
    """The text of the ValueError ``call`` raises, or None when it passes."""
    try:
        call()
    except ValueError as e:
        return str(e)
    return None


@pytest.mark.parametrize("fault", sorted(BATCH_FAULTS))
@pytest.mark.parametrize("name", sorted(BATCH_CHECKS))
def test_the_batch_check_words_each_refusal_as_its_caller_did(name, fault):
    assert refusal(lambda: BATCH_CHECKS[name](fake_batch(**BATCH_FAULTS[fault]))) == BATCH_CHECK[name, fault]


def test_the_old_names_of_the_batch_check_still_import():
    for fault in sorted(BATCH_FAULTS):
        b = fake_batch(**BATCH_FAULTS[fault])
        assert refusal(lambda: split_align._check_batch(b)) == BATCH_CHECK["split_align_batch", fault]


# ---------------------------------------------------------------------------------------------------------------------
# refusal order of every batch entry point: doubly spoiled calls on stand-in batches (nothing reaches the device)

TWO = dict(n_cand=2)
FLOAT = dict(ref_dtype=_native.FFS_DTYPE_F32)
EMPTY = dict(lens=[[100, 100], [0, -3]])
NOT_FINITE = dict(hi=INF)
_z = np.zeros(3, np.int64)
ONE_BLOCK = SimpleNamespace(block_offsets=np.zeros(1, np.int32), block_jump=np.zeros(1, np.uint8))
NO_BLOCK = SimpleNamespace(block_offsets=np.zeros(0, np.int32), block_jump=np.zeros(2, np.uint8))
LISTS = (np.zeros(1, np.uint64), [100], [0.0], [1.0], np.zeros(1, np.uint64), [100], [0.0], [1.0], [0], [0])
ENTRY_POINTS = {
    # a bad scalar together with a bad batch: the scalar is refused
    "split_align_batch/scalar": lambda: split_align.split_align_batch(fake_batch(**TWO), 6000, block_samples=1000),
    "split_report_batch/scalar": lambda: split_report.split_report_batch(fake_batch(**TWO), 6000, top_k=0),
    "refine_breaks_batch/scalar": lambda: split_refine.refine_breaks_batch(fake_batch(**TWO), [], radius_samples=0),
    "split_align_range_batch/scalar": lambda: cut_align.split_align_range_batch(fake_batch(**TWO), (5, 1), split_penalty=-1.0),
    "report_batch/scalar": lambda: cut_report.report_batch(fake_batch(**TWO), [], (5, 1), exclusion_samples=0),
    "split_range_report_batch/scalar": lambda: cut_report.split_range_report_batch(fake_batch(**TWO), (5, 1), top_k=99),
    "drift_align_batch/scalar": lambda: drift_align.drift_align_batch(fake_batch(**TWO), 6000, max_step=9),
    "drift_report_batch/scalar": lambda: drift_report.drift_report_batch(fake_batch(**TWO), 6000, step_cost=-1.0),
    "smooth_align_batch/scalar": lambda: drift_smooth.smooth_align_batch(fake_batch(**TWO), 6000, knot_blocks=0),
    "refine_jumps_batch/scalar": lambda: drift_refine.refine_jumps_batch(fake_batch(**TWO), [], unmatched_margin=-1.0),
    "drift_align_range_batch/scalar": lambda: drift_range.drift_align_range_batch(fake_batch(**TWO), (5, 1), max_step=-1),
    "smooth_align_range_batch/scalar": lambda: drift_range_smooth.smooth_align_range_batch(fake_batch(**TWO), (5, 1),
                                                                                           bend_cost=NAN),
    "drift_range_path_report_batch/scalar": lambda: drift_range_report.drift_range_path_report_batch(
        fake_batch(**TWO), ([], []), (5, 1), top_k=0),
    "drift_range_report_batch/scalar": lambda: drift_range_report.drift_range_report_batch(fake_batch(**TWO), (5, 1),
                                                                                           block_samples=100),
    "cue_report_batch/scalar": lambda: cue_report.cue_report_batch(fake_batch(**TWO), [], radius_samples=-1),
    "retime_batch/scalar": lambda: cue_retime.retime_batch(fake_batch(**TWO), [], penalty_q=-1),
    "quality_batch/scalar": lambda: quality.quality_batch(fake_batch(**TWO), 0),
    "quality_from_lists/scalar": lambda: match.quality_from_lists(*LISTS, 6000, top_k=0, algorithm="nope"),
    "quality_from_lists/algorithm": lambda: match.quality_from_lists(*LISTS, 6000, algorithm="nope"),
    # a bad batch together with a bad lag range, path or table: the batch is refused
    "split_align_batch/batch": lambda: split_align.split_align_batch(fake_batch(**FLOAT), 6000),
    "split_report_batch/batch": lambda: split_report.split_report_batch(fake_batch(**EMPTY), 6000),
    "refine_breaks_batch/batch": lambda: split_refine.refine_breaks_batch(fake_batch(**NOT_FINITE), [ONE_BLOCK]),
    "split_align_range_batch/batch": lambda: cut_align.split_align_range_batch(fake_batch(**TWO), (5, 1)),
    "report_batch/batch": lambda: cut_report.report_batch(fake_batch(**EMPTY), [], (5, 1)),
    "split_range_report_batch/batch": lambda: cut_report.split_range_report_batch(fake_batch(**FLOAT), (1.5, 2)),
    "drift_align_batch/batch": lambda: drift_align.drift_align_batch(fake_batch(**EMPTY), 6000),
    "drift_report_batch/batch": lambda: drift_report.drift_report_batch(fake_batch(**TWO), 6000),
    "smooth_align_batch/batch": lambda: drift_smooth.smooth_align_batch(fake_batch(**NOT_FINITE), 6000),
    "refine_jumps_batch/batch": lambda: drift_refine.refine_jumps_batch(fake_batch(**TWO), [ONE_BLOCK]),
    "drift_align_range_batch/batch": lambda: drift_range.drift_align_range_batch(fake_batch(**EMPTY), "x"),
    "smooth_align_range_batch/batch": lambda: drift_range_smooth.smooth_align_range_batch(fake_batch(**TWO), [(0, 1)] * 3),
    "drift_range_path_report_batch/batch": lambda: drift_range_report.drift_range_path_report_batch(
        fake_batch(**FLOAT), ([], []), (5, 1)),
    "drift_range_report_batch/batch": lambda: drift_range_report.drift_range_report_batch(fake_batch(**NOT_FINITE), (5, 1)),
    "cue_report_batch/batch": lambda: cue_report.cue_report_batch(fake_batch(**FLOAT), [(_z, _z, _z)]),
    "retime_batch/batch": lambda: cue_retime.retime_batch(fake_batch(**EMPTY), [(_z, _z, _z)]),
    "quality_batch/batch": lambda: quality.quality_batch(fake_batch(**FLOAT), 6000),
    # a good batch: the lag range, the number of paths and their lengths are refused before a device is needed
    "split_align_range_batch/range": lambda: cut_align.split_align_range_batch(fake_batch(), (5, 1)),
    "report_batch/range": lambda: cut_report.report_batch(fake_batch(), [], (1.5, 2)),
    "split_range_report_batch/range": lambda: cut_report.split_range_report_batch(fake_batch(), [(0, 1)] * 3),
    "drift_align_range_batch/range": lambda: drift_range.drift_align_range_batch(fake_batch(), "x"),
    "smooth_align_range_batch/range": lambda: drift_range_smooth.smooth_align_range_batch(fake_batch(), (0, 2 ** 31)),
    "drift_range_path_report_batch/range": lambda: drift_range_report.drift_range_path_report_batch(
        fake_batch(), ([], []), (5, 1)),
    "drift_range_report_batch/range": lambda: drift_range_report.drift_range_report_batch(fake_batch(), (5, 1)),
    "refine_breaks_batch/count": lambda: split_refine.refine_breaks_batch(fake_batch(), [ONE_BLOCK]),
    "refine_breaks_batch/length": lambda: split_refine.refine_breaks_batch(fake_batch(), [ONE_BLOCK, NO_BLOCK]),
    "refine_jumps_batch/count": lambda: drift_refine.refine_jumps_batch(fake_batch(), [ONE_BLOCK]),
    "refine_jumps_batch/length": lambda: drift_refine.refine_jumps_batch(fake_batch(), [ONE_BLOCK, NO_BLOCK]),
    "cue_report_batch/tables": lambda: cue_report.cue_report_batch(fake_batch(), [(_z, _z, _z)]),
    "retime_batch/tables": lambda: cue_retime.retime_batch(fake_batch(), [(_z, _z, _z), (_z, _z[:2], _z)]),
}
LAG_ORDER = "lag range [%d, %d]: need -(2^31 - 1) <= lag_lo <= lag_hi <= 2^31 - 1 and at most 2^31 - 1 lags"
REFUSALS = {
    "cue_report_batch/batch": FLOAT_REFERENCE % ("cue_report_batch", "F32"),
    "cue_report_batch/scalar": "radius_samples=-1: need an integer in [0, 4096]",
    "cue_report_batch/tables": "1 cue tables for 2 pairs",
    "drift_align_batch/batch": NO_SPEECH % (0, -3),
    "drift_align_batch/scalar": "max_step=9: need an integer in [0, 7]",
    "drift_align_range_batch/batch": NO_SPEECH % (0, -3),
    "drift_align_range_batch/range": "1 lag ranges for 2 pairs",
    "drift_align_range_batch/scalar": "max_step=-1: need an integer in [0, 7]",
    "drift_range_path_report_batch/batch": TWO_LEVEL % "split_align_batch",
    "drift_range_path_report_batch/range": LAG_ORDER % (5, 1),
    "drift_range_path_report_batch/scalar": "top_k=0: need an integer in [1, 8]",
    "drift_range_report_batch/batch": FINITE_LEVELS,
    "drift_range_report_batch/range": LAG_ORDER % (5, 1),
    "drift_range_report_batch/scalar": "block_samples=100: need a multiple of 32 in [256, 32768]",
    "drift_report_batch/batch": ONE_CANDIDATE % "split_align_batch",
    "drift_report_batch/scalar": "step_cost=-1.0: need a finite number >= 0",
    "quality_batch/batch": FLOAT_REFERENCE % ("quality_batch", "F32"),
    "quality_batch/scalar": "max_offset_samples=0: need an integer W >= 1, or None",
    "quality_from_lists/algorithm": "unknown algorithm 'nope': expected one of auto, bits, runs",
    "quality_from_lists/scalar": "top_k=0: need an integer in [1, 8]",
    "refine_breaks_batch/batch": FINITE_LEVELS,
    "refine_breaks_batch/count": "1 split results for 2 pairs",
    "refine_breaks_batch/length": "pair 1: 0 block offsets, 1 blocks of 1024 samples",
    "refine_breaks_batch/scalar": "radius_samples=0: need an integer in [1, 131072]",
    "refine_jumps_batch/batch": ONE_CANDIDATE % "split_align_batch",
    "refine_jumps_batch/count": "1 drift results for 2 pairs",
    "refine_jumps_batch/length": "pair 1: 0 block offsets and 2 jump flags, 1 blocks of 1024 samples",
    "refine_jumps_batch/scalar": "unmatched_margin=-1.0: need a finite number >= 0, or None for a single cut",
    "report_batch/batch": NO_SPEECH % (0, -3),
    "report_batch/range": "lag range (1.5, 2): need integers",
    "report_batch/scalar": "exclusion_samples=0: need an integer >= 1",
    "retime_batch/batch": NO_SPEECH % (0, 0),
    "retime_batch/scalar": "penalty_q=-1: need an integer in [0, 2^20] (64ths of a sample of agreement per sample of shift)",
    "retime_batch/tables": "pair 1: 3 starts, 2 ends and 3 lags: the three cue arrays need one length",
    "smooth_align_batch/batch": FINITE_LEVELS,
    "smooth_align_batch/scalar": "knot_blocks=0: need an integer in [1, 256]",
    "smooth_align_range_batch/batch": ONE_CANDIDATE % "split_align_batch",
    "smooth_align_range_batch/range": LAG_ORDER % (0, 2147483648),
    "smooth_align_range_batch/scalar": "bend_cost=nan: need a finite number >= 0",
    "split_align_batch/batch": TWO_LEVEL % "split_align_batch",
    "split_align_batch/scalar": "block_samples=1000: need a multiple of 32 in [256, 32768]",
    "split_align_range_batch/batch": ONE_CANDIDATE % "split_align_batch",
    "split_align_range_batch/range": LAG_ORDER % (5, 1),
    "split_align_range_batch/scalar": "split_penalty=-1.0: need a number >= 0 (inf = never split)",
    "split_range_report_batch/batch": TWO_LEVEL % "split_align_batch",
    "split_range_report_batch/range": "3 lag ranges for 2 pairs",
    "split_range_report_batch/scalar": "top_k=99: need an integer in [1, 8]",
    "split_report_batch/batch": NO_SPEECH % (0, -3),
    "split_report_batch/scalar": "top_k=0: need an integer in [1, 8]",
}


@pytest.mark.parametrize("case", sorted(ENTRY_POINTS))
def test_every_entry_point_refuses_in_the_order_and_words_it_did(case):
    assert refusal(ENTRY_POINTS[case]) == REFUSALS[case]


def test_the_refusal_table_covers_every_entry_point_three_ways():
    assert sorted(REFUSALS) == sorted(ENTRY_POINTS)
    for name in {c.split("/")[0] for c in ENTRY_POINTS} - {"quality_from_lists"}:
        assert {name + "/scalar", name + "/batch"} <= set(ENTRY_POINTS), name


# ---------------------------------------------------------------------------------------------------------------------
# the shared derivation of psr, margin and the gains

RECORDS = {
    "flat": dict(std=0.0, n_peaks=2, peaks=(5.0, 5.0), mean=5.0, own=5.0, prev=4.0, nxt=NAN, flat=5.0),
    "no_peak": dict(std=2.0, n_peaks=0, peaks=(), mean=1.0, own=3.0, prev=NAN, nxt=2.0, flat=1.0),
    "one_peak": dict(std=2.0, n_peaks=1, peaks=(9.0,), mean=1.0, own=9.0, prev=3.0, nxt=5.0, flat=8.0),
    "first": dict(std=4.0, n_peaks=3, peaks=(21.0, 11.0, 7.0), mean=1.0, own=21.0, prev=NAN, nxt=5.0, flat=20.0),
    "ordinary": dict(std=8.0, n_peaks=2, peaks=(41.0, 17.0), mean=1.0, own=37.0, prev=13.0, nxt=-3.0, flat=36.0, flags=4),
}


def make_record(dtype, r):
    rec = np.zeros(1, dtype)[0]
    rec["first_block"], rec["end_block"], rec["start_sample"], rec["end_sample"] = 2, 5, 2048, 5000
    rec["mean"], rec["std"], rec["n_lags"], rec["n_peaks"], rec["flags"] = r["mean"], r["std"], 12000, r["n_peaks"], r.get("flags", 0)
    rec["own_score"], rec["prev_score"], rec["next_score"] = r["own"], r["prev"], r["nxt"]
    where = "peak_offset" if "peak_offset" in dtype.names else "peak_shift"
    for i, s in enumerate(r["peaks"]):
        rec["peak_score"][i], rec[where][i] = s, 10 * i - 7
    if "offset" in dtype.names:
        rec["offset"] = -7
    else:
        rec["first_offset"], rec["last_offset"], rec["min_offset"], rec["max_offset"] = -7, -5, -8, -5
        rec["flat_score"], rec["flat_offset"] = r["flat"], -6
    return rec


def same(a, b) -> bool:
    """Equality of two ``dataclasses.asdict`` values with NaN equal to NaN, types included."""
    if isinstance(a, float) and isinstance(b, float):
        return (math.isnan(a) and math.isnan(b)) or a == b
    if isinstance(a, (list, tuple)) and type(a) is type(b):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


COPIED = dict(first_block=2, end_block=5, start_sample=2048, end_sample=5000, n_lags=12000)
PIECE_COPIED = dict(offset=-7)
SEGMENT_COPIED = dict(first_offset=-7, last_offset=-5, min_offset=-8, max_offset=-5, flat_offset=-6)
BOTH = {
    "first": dict(own_score=21.0, prev_score=NAN, next_score=5.0, peaks=[(21.0, -7), (11.0, 3), (7.0, 13)], mean=1.0,
                  std=4.0, psr=5.0, margin=2.5, gain_prev=NAN, gain_next=4.0, flags=0),
    "flat": dict(own_score=5.0, prev_score=4.0, next_score=NAN, peaks=[(5.0, -7), (5.0, 3)], mean=5.0, std=0.0, psr=0.0,
                 margin=0.0, gain_prev=0.0, gain_next=NAN, flags=1),
    "no_peak": dict(own_score=3.0, prev_score=NAN, next_score=2.0, peaks=[], mean=1.0, std=2.0, psr=0.0, margin=0.0,
                    gain_prev=NAN, gain_next=0.0, flags=1),
    "one_peak": dict(own_score=9.0, prev_score=3.0, next_score=5.0, peaks=[(9.0, -7)], mean=1.0, std=2.0, psr=4.0,
                     margin=INF, gain_prev=3.0, gain_next=2.0, flags=0),
    "ordinary": dict(own_score=37.0, prev_score=13.0, next_score=-3.0, peaks=[(41.0, -7), (17.0, 3)], mean=1.0, std=8.0,
                     psr=5.0, margin=3.0, gain_prev=3.0, gain_next=5.0, flags=4),
}
SEGMENT_ONLY = {
    "first": dict(flat_score=20.0, drift_gain=0.25),
    "flat": dict(flat_score=5.0, drift_gain=0.0),
    "no_peak": dict(flat_score=1.0, drift_gain=0.0),
    "one_peak": dict(flat_score=8.0, drift_gain=0.5),
    "ordinary": dict(flat_score=36.0, drift_gain=0.125),
}
PIECES = {c: {**COPIED, **PIECE_COPIED, **BOTH[c]} for c in BOTH}
SEGMENTS = {c: {**COPIED, **SEGMENT_COPIED, **BOTH[c], **SEGMENT_ONLY[c]} for c in BOTH}


@pytest.mark.parametrize("case", sorted(RECORDS))
def test_piece_and_segment_records_derive_what_they_derived(case):
    piece = dataclasses.asdict(split_report.from_record(make_record(_native.PIECE_REPORT_DTYPE, RECORDS[case])))
    segment = dataclasses.asdict(drift_report.from_record(make_record(_native.SEGMENT_REPORT_DTYPE, RECORDS[case])))
    for got, want in ((piece, PIECES[case]), (segment, SEGMENTS[case])):
        assert sorted(got) == sorted(want)
        for field in want:
            assert same(got[field], want[field]), (field, got[field], want[field])
    for field in ("psr", "margin", "gain_prev", "gain_next", "flags", "peaks", "mean", "std"):
        assert same(piece[field], segment[field]), field  # one derivation: the two agree wherever both have the field
