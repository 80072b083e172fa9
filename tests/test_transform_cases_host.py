"""The claims of tests/transform_cases.py, checked without a device -- so that tests/test_gpu_transform_exact.py cannot
quietly go vacuous: the plan lengths, the inventory of kernel instances the expected dispatch covers, and the properties of
the exact reference the GPU test leans on (ties and unique winners in every case, planted offsets that win, plateaus
that fit the pool)."""
import numpy as np
import pytest

import exact_reference as er
import transform_cases as tc
from ffsubsync_amd import _native

HOST_LENGTHS = [n for n in tc.LENGTHS if n <= 1 << 20]  # the larger ones: the GPU module's own reference computation


def test_the_table_has_22_lengths_and_14_column_lengths():
    assert len(tc.LENGTHS) == 22 and len(set(tc.LENGTHS)) == 22
    assert len({tc.geometry(n)[0] for n in tc.LENGTHS}) == 14
    for n in tc.LENGTHS:
        n1, n2 = tc.geometry(n)
        assert n1 * n2 == n and n1 in tc.TILE and 256 <= n2 <= 4096


@pytest.mark.parametrize("n", tc.LENGTHS)
def test_vectors_fill_the_plan(n):
    """Windowless the plan length is exactly N; with a window at most N (the solves pass n_fft = N themselves)."""
    for vset in ("fill",) + (("long",) if n in tc.THREE_BLOCK else ()):
        R, S = tc.sizes(n, vset)
        lens = {c.size for c in tc.noise_problem(n, vset)[1]} | {c.size for p in tc.ties_problems(n, vset) for c in p[1]}
        assert max(lens) <= S and len(lens) >= 8
        if vset == "fill":
            assert R + S == n - 3 and _native.plan_length(R, S, None) == n
        for setting in "bc":
            assert all(2 < _native.plan_length(R, s, tc.window(n, setting)) <= n for s in lens)
    for run in tc.runs(n):
        assert run.vset == "fill" or run.setting == "b"
        probs = tc.problems(n, run)
        assert len(probs) == (1 if run.kind == "noise" else 2) and all(len(p[2]) == len(run.idx) for p in probs)
        if run.dtype in ("f32", "mixed"):  # float inputs are bit-exact with (0, 1) levels only
            assert all(lv == tc.UNIT for p in probs for lv in p[4])


def _union():
    seen = set()
    for n in tc.LENGTHS:
        for run in tc.runs(n):
            d = tc.expected_dispatch(n, run)
            seen.add((n, run.dtype, len(run.idx), run.setting) + tuple(d[k] for k in _native.DISPATCH_FIELDS))
    return seen


def test_inventory_of_kernel_instances():
    F = {k: 4 + i for i, k in enumerate(_native.DISPATCH_FIELDS)}
    seen = _union()
    has = lambda **kw: any(all(s[F[k]] == v if k in F else s[("n", "dtype", "n_cand", "setting").index(k)] == v for k, v in kw.items())
                           for s in seen)
    for n in tc.LENGTHS:
        # every length under a full (or radix-3), a pruned and both exhaustive last passes, bit-packed and bytes
        n1 = tc.geometry(n)[0]
        full = tc.LAST_C3 if n1 in tc.C3_N1 else tc.LAST_FULL
        for dtype in ("u1", "u8"):
            assert has(n=n, dtype=dtype, setting="a", last_family=full, sweep_family=tc.LAST_FULL, transform_length=n), (n, dtype)
            assert has(n=n, dtype=dtype, setting="b", last_family=tc.LAST_PRUNED, sweep_family=tc.LAST_PRUNED), (n, dtype)
        assert has(n=n, setting="a", n1=n1, dtype="f32") or not tc._first_of_n1(n)
        if n not in tc.BIG:
            assert has(n=n, setting="d", last_family=full, sweep_family=tc.LAST_FULL), n
            assert has(n=n, setting="c", last_family=tc.LAST_PRUNED), n
            for k in (1, 2, 3, 7):
                assert has(n=n, dtype="u1", n_cand=k), (n, k)
    for n1 in tc.C3_N1:  # k_pass_c3 with and without the half last slot, k_pass_a3 in every paired mode
        for hf in (1, 3):
            assert has(n1=n1, last_family=tc.LAST_C3, half_flags=hf), (n1, hf)
        for pm in (0, 1, 2):
            assert has(n1=n1, pass_a_family=tc.PASS_A3, pass_a_paired=pm), (n1, pm)
    for k in range(16, 25):  # k_pass_a's paired modes on the power-of-two lengths with 4096-point rows
        if tc.geometry(1 << k)[0] in tc.C3_N1:
            continue
        for pm in (0, 1, 2) if (1 << k) not in tc.BIG else (0, 2):
            assert has(transform_length=1 << k, pass_a_family=tc.PASS_A, pass_a_paired=pm), (k, pm)
    for n2 in (256, 512, 1024, 2048, 4096):
        assert has(mid_family=tc.MID, n2=n2), n2
    for n in tc.SEGMENTED:  # the three segmented mid kernels on every sub-plan length, two and three blocks
        for mid in (tc.MID_SEG_ONE_1, tc.MID_SEG_ONE_4, tc.MID_SEG_PIPE):
            assert has(n=n, transform_length=n // 3, mid_family=mid, seg_blocks=2), (n, mid)
            if n in tc.THREE_BLOCK:
                assert has(n=n, mid_family=mid, seg_blocks=3), (n, mid)
        assert has(n=n, setting="e", transform_length=n, last_family=tc.LAST_PRUNED), n
        if n not in tc.BIG:  # k_mid_seg_pipe's sweeps: odd slot count with and without the half last slot, all pairs
            for n_cand, hf in ((9, 3), (10, 1), (12, 1), (8, 1)):
                assert has(n=n, n_cand=n_cand, half_flags=hf, setting="b"), (n, n_cand)
    assert all(has(n=3 << 18, n_cand=k, setting="b", dtype="u1") for k in (1, 2, 3, 7, 8, 9, 10, 12))
    for n, setting in tc.MIXED.items():
        assert has(n=n, dtype="mixed", setting=setting, pass_a_ref_family=tc.PASS_A), n
    kinds = {(tc.geometry(n)[1] < 4096, n % 3 == 0, n in tc.SEGMENTED) for n in tc.MIXED}
    assert {(True, False, False), (False, False, False), (True, True, False), (False, True, True)} <= kinds


@pytest.mark.parametrize("n", HOST_LENGTHS)
def test_reference_properties(n):
    """Per case (length, vector set, setting): a tie record and a unique one; every planted offset inside the window is
    its candidate's exact winner; no plateau near the pool's capacity."""
    cases = {}
    for run in tc.runs(n):
        cases.setdefault((run.vset, tc.window(n, run.setting)), []).append(run)
    for (vset, max_off), rr in cases.items():
        n_at = []
        for run in rr:
            want = tc.expected(n, run)
            n_at += [r["n_at_max"] for recs, _ in want for r in recs]
            if run.kind != "noise":
                continue
            ref, cands, _, _, lags = tc.noise_problem(n, vset)
            for j, rec in zip(run.idx, want[0][0]):
                inside = lags[j] in set(er.qm.lag_set(ref.size, cands[j].size, max_off).tolist())
                if inside:
                    assert rec["offset"] == lags[j] and rec["n_at_max"] == 1, (n, vset, max_off, j, lags[j], rec)
        assert max(n_at) >= 2 and min(n_at) == 1, (n, vset, max_off, n_at)
        assert max(n_at) * 4 < tc.POOL_CAPACITY
        if max_off is None or max_off >= 705:
            assert max(n_at) > tc.KNOM  # wider than the nominee lists: the exhaustive sweep has real work
