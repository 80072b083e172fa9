"""tests/stream_cases.py on the host: the table holds every side-plan batch entry point of the header, the two problem
sets of every entry have equal shapes, and the model tells every pair of set A from its pair of set B -- without that a
call that returned another call's answers could pass tests/test_gpu_streams.py unnoticed."""
import os

import numpy as np
import pytest

import stream_cases as sc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ffsubsync_amd.h")


def test_the_table_holds_every_side_plan_batch_export_of_the_header():
    with open(HEADER) as f:
        exports = sc.header_exports(f.read())
    ops = sc.ops()
    assert list(ops) == sc.OP_NAMES and len(ops) == 16
    assert sorted(op.export for op in ops.values()) == sorted(exports) and len(exports) == 16
    plan_type = dict(zip(sc.PLAN_CLASSES, sc.SIDE_PLANS))
    for op in ops.values():  # on the plan class whose handle the export takes, through a method that exists
        assert exports[op.export] == plan_type[op.plan], op.name
        from ffsubsync_amd import _native

        assert callable(getattr(getattr(_native, op.plan), op.method)), op.name
    assert {op.name for op in ops.values() if op.host_waits} == {
        "SplitRangePlan.report", "DriftPlan.report", "DriftRangePlan.report", "MatchPlan.report"}


def test_the_parser_sees_only_batch_exports_on_side_plans():
    text = """int ffs_align_batch(ffs_plan* plan, int n_pairs);
    int ffs_new_thing_batch(ffs_drift_plan* plan,
                            int n_pairs);
    int ffs_split_plan_destroy(ffs_split_plan* plan);
    int ffs_runs_from_bits_batch(const uint32_t* const* bits_dev);"""
    assert sc.header_exports(text) == {"ffs_new_thing_batch": "ffs_drift_plan"}


def _shape(op, pr):
    """Everything about a problem but the contents of its two vectors."""
    out = {k: v for k, v in pr.items() if k not in ("rb", "sb", "ref", "sub")}
    out["lens"] = (pr["rb"].size, pr["sb"].size)
    return sc.dump(out)


@pytest.mark.parametrize("name", sc.OP_NAMES)
def test_sets_a_and_b_have_equal_shapes_and_other_contents(name):
    op = sc.ops()[name]
    for n in (sc.N_SET, sc.N_SUB_BATCHES):
        a, b = op.problems("A", n), op.problems("B", n)
        assert len(a) == len(b) == n
        for pa, pb in zip(a, b):
            assert _shape(op, pa) == _shape(op, pb)
            assert not np.array_equal(pa["rb"], pb["rb"]) and not np.array_equal(pa["sb"], pb["sb"])
        assert all(pr.get("k", sc.K) == sc.K for pr in a)
        assert [sc.dump(e) for e in op.extras(a).values()] == [sc.dump(e) for e in op.extras(b).values()]
        assert op.outputs(a) == op.outputs(b) and all(nbytes > 0 for _, nbytes in op.outputs(a))
    assert [_shape(op, pr) for pr in op.problems("A", sc.N_SUB_BATCHES)[:sc.N_SET]] == [_shape(op, pr) for pr in op.problems("A")]


@pytest.mark.parametrize("name", sc.OP_NAMES)
def test_the_model_tells_every_pair_of_a_from_its_pair_of_b(name):
    op = sc.ops()[name]
    for i in range(sc.N_SUB_BATCHES):
        assert sc.dump(op.want("A", i, sc.N_SUB_BATCHES)) != sc.dump(op.want("B", i, sc.N_SUB_BATCHES)), (name, i)


def test_the_retime_radii_of_the_mixed_sequence_are_told_apart_too():
    """``cue_retime`` at radius 5 and at radius 200 (the workspace grows between them): other records per radius and set."""
    op = sc.ops()["SplitPlan.cue_retime"]
    seen = set()
    for which in "AB":
        for radius in (5, 200):
            for pr in op.problems(which):
                seen.add(sc.dump(op.model(dict(pr, radius=radius))))
    assert len(seen) == 2 * 2 * sc.N_SET
