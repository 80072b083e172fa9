"""The case tables of tests/resample_edge_cases.py hold what they name, so tests/test_gpu_resample_edges.py cannot be
vacuous: every crafted seed gives its key, every large list is valid and stays valid through the models without being
expanded, and the models' answers on the tiny files and tracks contain every situation the GPU tests are there for.
Host only (numpy models and ``exact_reference``); no device, no library call."""
import numpy as np

import resample_edge_cases as rc
import stability_model as stm
import surrogate_cases as cases
import surrogate_model as sm


# ---- crafted seeds -----------------------------------------------------------------------------------------------------
def test_seed_for_key_inverts_the_key():
    rng = np.random.RandomState(1)
    for _ in range(200):
        key, s, b = int(rng.randint(0, 2 ** 32, dtype=np.uint64)), int(rng.randint(0, 4096)), int(rng.randint(0, 8192))
        seed = rc.seed_for_key(key, s, b)
        assert 0 <= seed <= 0xFFFFFFFF and sm.key(seed, s, b) == key


def test_every_surrogate_case_puts_its_key_on_its_block():
    assert {c[4] for c in rc.SURROGATE_CASES} == {rc.PAD_KEY, rc.ZERO_KEY}
    padded = 0
    for i, case in enumerate(rc.SURROGATE_CASES):
        units, block, s, b, key = case
        seed, nb = rc.surrogate_seed(case), rc.n_blocks_of(units, block)
        assert s < rc.SURROGATE_K and b < nb
        assert sm.key(seed, s, b) == key and int(sm.keys(seed, s, nb)[b]) == key
        order = sm.block_order(seed, s, nb)
        assert int(order[nb - 1 if key == rc.PAD_KEY else 0]) == b, case  # the largest key last, the smallest first
        if b == nb - 1:
            assert cases.short_block_place(seed, s, units, block) == (nb - 1 if key == rc.PAD_KEY else 0)
        padded += nb & (nb - 1) != 0
        pos, _ = rc.crafted_list("surrogate", i)
        assert pos.size == 2 * (units + 1)
    assert padded == len(rc.SURROGATE_CASES) - 1  # one case sorts exactly 8 keys; every other sort has padding words
    shorts = [(u, bl, b) for u, bl, _, b, _ in rc.SURROGATE_CASES if u % bl and b == rc.n_blocks_of(u, bl) - 1]
    assert set(shorts) == {(65, 7, 9), (15, 7, 2)}  # the short last block carries either key, nb = 10 and nb = 3


def test_every_stability_case_sits_on_the_keep_bit():
    kept = {}
    for i, case in enumerate(rc.STABILITY_CASES):
        runs, block, s, b, key = case
        seed, nb = rc.stability_seed(case), rc.n_blocks_of(runs, block)
        assert s < rc.STABILITY_K and b < nb and sm.key(seed, s >> 1, b) == key
        pair = [bool(stm.keep_mask(seed, 2 * (s >> 1) + j, nb)[b]) for j in (0, 1)]
        assert sorted(pair) == [False, True]  # exactly one member of the pair keeps the block
        assert pair[0] == (key == rc.KEEP_BIT)  # the even member keeps it iff bit 31 is set
        kept[(runs, block, s, b, key)] = bool(stm.keep_mask(seed, s, nb)[b])
        pos, _ = rc.crafted_list("stability", i)
        assert pos.size == 2 * runs
        # the block's runs are in the output of the keeping member and of no other
        first = int(pos[2 * b * block])
        assert (first in stm.subsample(pos, seed, s, block).tolist()) == kept[(runs, block, s, b, key)]
    for (runs, block, s, b, key), k in kept.items():
        assert kept[(runs, block, s, b, key ^ 0xFFFFFFFF)] != k  # 0x7FFFFFFF <-> 0x80000000: the decision flips
    assert {(c[0], c[1]) for c in rc.STABILITY_CASES} == {(65, 7), (257, 1)} and {c[2] & 1 for c in rc.STABILITY_CASES} == {0, 1}


# ---- large lists -------------------------------------------------------------------------------------------------------
def _valid_block(words, n, ones, length, cap):
    assert words.dtype == np.int32 and words.size == 4 + 2 * (n + 1)
    assert tuple(words[:4]) == (n, ones, length, cap)
    pos, before = words[4:4 + 2 * n:2].astype(np.int64), words[5:5 + 2 * n:2].astype(np.int64)
    assert (np.diff(pos) > 0).all() and (n == 0 or (pos[0] >= 0 and pos[-1] <= length))
    runs = pos[1::2] - pos[0::2]
    assert np.array_equal(before[0::2], np.cumsum(runs) - runs) and np.array_equal(before[1::2], np.cumsum(runs))
    assert tuple(words[4 + 2 * n:]) == (rc.INT32_MAX, ones)


def test_large_lists_are_valid_and_stay_valid_through_the_models():
    lists = rc.large_lists()
    assert sorted(lists) == ["a", "a3", "b", "c", "c3"]
    for name, (pos, length) in lists.items():
        assert length == 2 ** 31 - 1 and pos.dtype == np.int64
        assert (np.diff(pos) > 0).all() and pos[0] >= 0 and int(pos[-1]) <= length
        ones = rc.ones_of(pos)
        assert 0 < ones < 2 ** 31
        for block in rc.LARGE_BLOCKS:
            for s in range(rc.LARGE_K):
                sur = sm.surrogate(pos, 12345, s, block)
                assert rc.ones_of(sur) == ones and sur.size == pos.size
                _valid_block(sm.encode(sur, length, pos.size + 1), pos.size, ones, length, pos.size + 1)
                half = stm.subsample(pos, 12345, s, block)
                _valid_block(stm.encode(half, length, pos.size + 1), half.size, rc.ones_of(half), length, pos.size + 1)
    pos_a, pos_b, pos_c = lists["a"][0], lists["b"][0], lists["c"][0]
    assert pos_a.size == 18 and (np.diff(pos_a) >= 2 ** 26).all() and pos_a[0] >= 2 ** 26
    assert pos_b.size == 24 and rc.ones_of(pos_b) > 2 ** 30
    assert pos_c.size == 4100 and int(pos_c[-1]) == 2 ** 31 - 1 and int(pos_c[0]) > 2 ** 31 - 2 ** 18
    for name in ("a3", "c3"):
        pos = lists[name][0]
        assert int(pos[0]) == 0 and int(pos[-1]) == 2 ** 31 - 1
    assert int(lists["c3"][0][2] - lists["c3"][0][0]) > 2 ** 31 - 2 ** 18  # one unit spans nearly the whole vector


# ---- tiny files --------------------------------------------------------------------------------------------------------
def test_tiny_files_are_what_the_table_says():
    assert len(rc.TINY_FILES) == 7 and sorted({f[2] for f in rc.TINY_FILES}) == [0, 1, 2, 3, 9, 40]
    assert {f[0] for f in rc.TINY_FILES} == {3000, 1777, 5003}
    assert {f[1] for f in rc.TINY_FILES} == {(0.0, 1.0), (0.25, 1.0)} and {f[4] for f in rc.TINY_FILES} == {(0.0, 1.0), (0.0, 0.5)}
    for i, (ref_len, _, runs, sub_len, _, seed, _) in enumerate(rc.TINY_FILES):
        ref, pos, sub = rc.tiny_file(i)
        assert ref.size == ref_len != sub_len == sub.size and pos.size == 2 * runs and 0 <= seed <= 0xFFFFFFFF
        assert np.array_equal(sm.boundaries(sub), pos)
        assert 80 <= sm.boundaries(ref).size < 32768  # a few hundred boundaries at the longest


def test_the_models_answers_on_the_tiny_files_contain_every_situation():
    seen = set()
    for i, (_, _, runs, sub_len, _, seed, _) in enumerate(rc.TINY_FILES):
        _, pos, _ = rc.tiny_file(i)
        silent = rc.silent_record(i)
        for block in rc.TINY_BLOCKS:
            sc, off, fl = rc.tiny_model(i, block)["half"]
            sizes = [stm.subsample(pos, seed, s, block).size for s in range(rc.TINY_K_MAX)]
            for s, size in enumerate(sizes):
                if size == 0:  # a half-sample that keeps nothing is the silent subtitle: every lag ties, the tie rule decides
                    assert (sc[1 + s], off[1 + s], fl[1 + s]) == (silent["score"], silent["offset"], silent["flags"])
                    seen.add("silent half-sample")
                    if runs:
                        seen.add("silent half-sample of a list with runs")
            if block == 64 and runs:
                assert sorted(sizes[:2]) == [0, pos.size]
                seen.add("everything beside nothing")
            for k in rc.TINY_K:
                half, null = rc.tiny_half_record(i, block, k), rc.tiny_null_record(i, block, k)
                if k == 1:
                    assert half["flags"] & stm.NO_PAIRS and half["n_pairs"] == 0
                    seen.add("NO_PAIRS")
                if k == 5:
                    assert half["n_sub"] == 5 and half["n_pairs"] == 2
                    seen.add("odd K")
                if runs <= 2:
                    assert null["flags"] == sm.FLAT and null["n_ge"] == k and null["null_std"] == 0.0
                    seen.add("FLAT")
                if not null["flags"] & sm.FLAT:
                    seen.add("non-flat")
                    if null["n_ge"] > 0:
                        seen.add("non-flat with n_ge > 0")
                    if null["n_ge"] == 0:
                        seen.add("non-flat with n_ge == 0")
                if half["max_dev"] > rc.TINY_TOL:
                    seen.add("a half-sample outside tol")
                if half["n_within"] == k:
                    seen.add("every half-sample within tol")
                assert not half["flags"] & stm.EMPTY and not null["flags"] & sm.EMPTY
    assert seen == {"silent half-sample", "silent half-sample of a list with runs", "everything beside nothing", "NO_PAIRS", "odd K",
                    "FLAT", "non-flat", "non-flat with n_ge > 0", "non-flat with n_ge == 0", "a half-sample outside tol",
                    "every half-sample within tol"}, seen


def test_the_models_answers_on_the_tiny_tracks_warn_about_too_few_blocks():
    few_null = few_stable = 0
    for i, (cues, meta) in enumerate(rc.TRACK_CUES):
        null, stable = rc.track_null_model(i), rc.track_stable_model(i)
        assert (null["ratio"], null["offset"], null["score"]) == (stable["ratio"], stable["offset"], stable["score"])
        assert null["blocks"] <= max(cues - meta - 1, 0) and stable["blocks"] <= cues - meta
        few_null += any(r.startswith("too few cues to shuffle (%d blocks < 8)" % null["blocks"]) for r in null["reasons"])
        few_stable += any(r.startswith("too few cues to resample (%d blocks < 8)" % stable["blocks"]) for r in stable["reasons"])
        if cues - meta <= 2:
            assert null["record"]["flags"] & sm.FLAT and "flat null (std 0)" in null["reasons"] and not null["trusted"]
    assert few_null >= 4 and few_stable >= 3
    assert {rc.track_null_model(i)["blocks"] for i in range(len(rc.TRACK_CUES))} >= {0, 1}
    assert rc.track_stable_model(3)["blocks"] < 9  # nine cues, some of which merge on the sample grid
