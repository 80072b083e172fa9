"""tests/surrogate_model.py against brute force: the surrogate of a list against the statement itself on
the expanded samples, the hash against a scalar restatement, the tie rule of equal keys, the stats record against a loop,
and the verdicts the model alone gives on the end-to-end problems at the shipped ``min_z``.  No device."""
import math

import numpy as np
import pytest

import surrogate_cases as cases
import surrogate_model as sm


def test_hash_against_the_scalar_statement():
    assert sm.fmix32(0) == 0 and sm.fmix32(1) == 0x514E28B7  # murmur3's finaliser
    for seed, s in ((0, 0), (1, 0), (0xFFFFFFFF, 4095), (123456789, 63)):
        ks = sm.keys(seed, s, 300)
        assert ks.dtype == np.uint64 and [int(k) for k in ks] == [sm.key(seed, s, b) for b in range(300)]
    assert sm.file_seed(0, 0) == sm.fmix32(0) and sm.file_seed(0xFFFFFFFF, 1) == sm.fmix32(0)  # uint32 wrap-around


@pytest.mark.parametrize("block_units", [1, 2, 7, 64, 9000])
def test_surrogates_against_brute_force(block_units):
    rng = np.random.RandomState(block_units)
    for units in cases.UNITS[:12]:
        for kind in range(4):
            pos, length = cases.random_list(rng, units, kind)
            v = sm.expand(pos, length)
            assert np.array_equal(sm.boundaries(v), pos)
            for s in (0, 5):
                seed = int(rng.randint(0, 2 ** 31))
                got = sm.surrogate(pos, seed, s, block_units)
                want = cases.brute_force(v, seed, s, block_units)
                assert np.array_equal(sm.expand(got, length), want), (units, kind, s)
                assert got.size == pos.size and (np.diff(got) >= 1).all() and want.sum() == v.sum()
                if units <= 1:
                    assert np.array_equal(got, pos)
    # no run at all (m = 0) and one run (m = 1)
    assert sm.surrogate(np.zeros(0, np.int64), 1, 0, block_units).size == 0
    assert np.array_equal(sm.surrogate(np.array([3, 9]), 1, 0, block_units), [3, 9])


def test_units_keep_run_and_silence_together():
    rng = np.random.RandomState(3)
    pos, length = cases.random_list(rng, 257)
    pairs = lambda p: sorted(zip(p[1:-2:2] - p[0:-2:2], p[2::2] - p[1:-2:2]))
    for b in (1, 7):
        got = sm.surrogate(pos, 77, 2, b)
        assert pairs(got) == pairs(pos) and not np.array_equal(got, pos)
        assert got[0] == pos[0] and np.array_equal(got[-2:], pos[-2:])


def test_keys_of_one_surrogate_never_collide():
    """The contract orders blocks by (key, b), but fmix32 is a bijection of uint32: the keys of one surrogate are fmix32
    of distinct words, so no (seed, s) with two equal keys exists and the index never decides.  Shown by the inverse."""
    rng = np.random.RandomState(2)
    for h in [0, 1, 0xFFFFFFFF, 0x80000000] + [int(x) for x in rng.randint(0, 2 ** 32, 2000, dtype=np.uint64)]:
        assert cases.fmix32_inverse(sm.fmix32(h)) == h and sm.fmix32(cases.fmix32_inverse(h)) == h
    for seed in range(200):
        assert np.unique(sm.keys(seed, seed % 7, 8192)).size == 8192
    order = sm.block_order(9, 3, 8192)
    assert list(order) == sorted(range(8192), key=lambda b: (sm.key(9, 3, b), b))


def test_the_short_block_can_land_anywhere():
    for units, b in ((65, 7), (257, 64), (3, 2)):
        seed = cases.seed_placing_short_block(units, b)
        nb = (units + b - 1) // b
        assert cases.short_block_place(seed, 0, units, b) == 0 and cases.short_block_place(seed, 1, units, b) == nb - 1


def test_encode_writes_a_valid_block():
    pos, length = cases.random_list(np.random.RandomState(5), 64, kind=2)
    w = sm.encode(pos, length, 200)
    v = sm.expand(pos, length)
    assert list(w[:4]) == [pos.size, int(v.sum()), length, 200] and list(w[-2:]) == [sm.INT32_MAX, int(v.sum())]
    csum = np.concatenate([[0], np.cumsum(v)])
    assert np.array_equal(w[5:-2:2], csum[pos]) and np.array_equal(w[4:-2:2], pos) and pos[-1] == length
    assert list(sm.empty_block(77, 9)) == [0, 0, 77, 9, sm.INT32_MAX, 0]


def test_status_bits():
    assert sm.status(10, 11, 10) == 0 and sm.status(0, 1, 0) == 0
    assert sm.status(5, 9, 9) == sm.BAD_ODD
    assert sm.status(10, 10, 10) == sm.BAD_TRUNCATED and sm.status(-2, 10, 10) == sm.BAD_TRUNCATED
    assert sm.status(10, 20, 8) == sm.BAD_BOUND
    assert sm.status(2 * 8193 + 2, 1 << 20, 1 << 20) == sm.BAD_UNITS and sm.status(2 * 8192 + 2, 1 << 20, 1 << 20) == 0


def _loop_stats(scores, flags):
    real, nulls = scores[0], []
    real_ok = math.isfinite(real) and not flags[0] & 1
    for s, f in zip(scores[1:], flags[1:]):
        if math.isfinite(s) and not f & 1:
            nulls.append(float(s))
    n = len(nulls)
    mean = sum(nulls) / n if n else 0.0
    flat = n == 0 or min(nulls) == max(nulls)
    std = 0.0 if flat else math.sqrt(sum((x - mean) ** 2 for x in nulls) / n)
    fl = (1 if flat else 0) | (2 if n == 0 or not real_ok else 0) | (4 if any(f & 2 for f in flags) else 0)
    return dict(n_null=n, n_ge=sum(x >= real for x in nulls) if real_ok else 0, n_gt=sum(x > real for x in nulls) if real_ok else 0,
                mean=mean, std=std, flags=fl, mn=min(nulls) if n else 0.0, mx=max(nulls) if n else 0.0)


def test_stats_against_a_loop():
    rng = np.random.RandomState(11)
    for k in (1, 2, 63, 64, 65, 257):
        for case in range(6):
            sc = rng.randint(0, 30, k + 1) * 0.37 - 2.0
            fl = np.zeros(k + 1, np.int32)
            if case == 1:
                sc[1:] = sc[1]
            if case == 2:
                sc[rng.rand(k + 1) < 0.3] = -np.inf
                fl[rng.rand(k + 1) < 0.3] |= 1
                fl[rng.rand(k + 1) < 0.1] |= 2
            if case == 3:
                sc[1:] = np.nan
            if case == 4:
                fl[0] |= 1
            if case == 5:
                sc[1:1 + (k + 1) // 2] = sc[0]
            got, want = sm.stats(sc, fl), _loop_stats([float(x) for x in sc], [int(x) for x in fl])
            assert (got["n_null"], got["n_ge"], got["n_gt"], got["flags"]) == (want["n_null"], want["n_ge"], want["n_gt"], want["flags"])
            assert got["null_min"] == want["mn"] and got["null_max"] == want["mx"]
            assert math.isclose(got["null_mean"], want["mean"], rel_tol=1e-12, abs_tol=1e-300)
            assert math.isclose(got["null_std"], want["std"], rel_tol=1e-12, abs_tol=1e-300)
            if case == 1:
                assert got["flags"] & sm.FLAT and got["null_std"] == 0.0 and got["null_mean"] == sc[1]
            z, p = sm.z_p(got)
            assert p == (1 + got["n_ge"]) / (1 + got["n_null"]) and (z == 0.0 if got["flags"] & sm.FLAT else True)


def test_the_model_alone_gives_the_verdicts_at_the_shipped_threshold():
    """10 minutes, seeds 0-5, matched and wrong, none left out, K = 64, the hash permutation, the seven-ratio winner:
    every matched file trusted with n_ge == 0, no wrong file trusted."""
    from ffsubsync_amd import surrogate

    kinds = cases.sync_kinds()
    seen = []
    for i, kind in enumerate(kinds):
        r = cases.model_sync(i, surrogate.DEFAULT_MIN_Z)
        seen.append((kind, cases.SYNC_SEEDS[i % len(cases.SYNC_SEEDS)], round(r["z"], 2), r["record"]["n_ge"], r["trusted"]))
    print(seen)
    bad = [x for x in seen if x[4] != (x[0] == "matched") or (x[0] == "matched" and x[3] != 0)]
    assert not bad, bad
