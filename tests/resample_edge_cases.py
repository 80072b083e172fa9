"""TEST INFRASTRUCTURE ONLY -- the edge cases of the shuffled-cue and half-sample paths that no random
seed and no 10-minute file reaches, shared by tests/test_resample_edge_cases_host.py (which proves that every case holds
what it names) and tests/test_gpu_resample_edges.py.  Host data only: imports without a GPU.

  - crafted seeds: fmix32 is invertible, so a seed that gives block b of surrogate s a chosen key is written down in
    closed form (``seed_for_key``): the keys 0xFFFFFFFF (the padding word of k_surrogate_lists' sort) and 0, and the two
    sides of the keep bit of k_subsample_lists, 0x7FFFFFFF and 0x80000000
  - large lists: len = 2^31 - 1, positions and ``ones`` near the ends of int32
  - tiny files and tiny tracks for the end-to-end wrappers, with the models' answers on them (computed once per process)
"""
import functools

import numpy as np

import stability_model as stm
import surrogate_cases as cases
import surrogate_model as sm

GOLDEN = 0x9E3779B9
INT32_MAX = sm.INT32_MAX
PAD_KEY, ZERO_KEY = 0xFFFFFFFF, 0
BELOW_BIT, KEEP_BIT = 0x7FFFFFFF, 0x80000000


# ---- crafted seeds -----------------------------------------------------------------------------------------------------
def seed_for_key(key, s, b):
    """The seed with ``sm.key(seed, s, b) == key``: both finalisers undone, then the surrogate's constant taken off."""
    return (cases.fmix32_inverse(cases.fmix32_inverse(key) ^ b) - GOLDEN * (s + 1)) & 0xFFFFFFFF


def _surrogate_cases():
    """(units, block_units, s, b, key): the key on block b of surrogate s of a list of ``units`` units."""
    out = []
    for key in (PAD_KEY, ZERO_KEY):
        out += [(5, 1, 0, 0, key), (5, 1, 1, 2, key), (5, 1, 2, 4, key)]  # first, middle, last of 5 blocks
        out += [(300, 1, 3, 299, key)]  # the last of 300 blocks (a 512-key sort with 212 padding words)
        out += [(65, 7, 1, 9, key), (15, 7, 2, 2, key)]  # the short last block: 2 of 7 units, 1 of 7 units
        out += [(65, 7, 3, 4, key)]  # a full block beside a short last one
    out.append((8, 1, 2, 7, PAD_KEY))  # nb = 8: a sort without any padding word
    return out


SURROGATE_CASES = _surrogate_cases()
SURROGATE_K = 1 + max(c[2] for c in SURROGATE_CASES)


def _stability_cases():
    """(runs, block_runs, s, b, key): the key on block b of the pair s >> 1; an even and an odd member of the same pair."""
    out = []
    for runs, block in ((65, 7), (257, 1)):
        nb = (runs + block - 1) // block
        for b in (nb // 2, nb - 1):
            for key in (BELOW_BIT, KEEP_BIT):
                out += [(runs, block, 2, b, key), (runs, block, 3, b, key)]
    return out


STABILITY_CASES = _stability_cases()
STABILITY_K = 1 + max(c[2] for c in STABILITY_CASES)


def surrogate_seed(case):
    _, _, s, b, key = case
    return seed_for_key(key, s, b)


def stability_seed(case):
    _, _, s, b, key = case
    return seed_for_key(key, s >> 1, b)


def n_blocks_of(units, block):
    return (units + block - 1) // block


@functools.lru_cache(maxsize=None)
def crafted_list(kind, index):
    """(pos, len) of the list of crafted case ``index``: kind "surrogate" (units + 1 runs) or "stability" (runs)."""
    case = (SURROGATE_CASES if kind == "surrogate" else STABILITY_CASES)[index]
    rng = np.random.RandomState(7000 + 100 * (kind == "stability") + index)
    units = case[0] if kind == "surrogate" else case[0] - 1
    return cases.random_list(rng, units, kind=index % 4)


# ---- large lists -------------------------------------------------------------------------------------------------------
LARGE_LEN = INT32_MAX
LARGE_BLOCKS = (1, 2, 7)
LARGE_K = 4


def _list_from(lead, runs, gaps):
    """pos of the runs ``runs`` with ``lead`` samples in front and ``gaps[j]`` behind run j (the last gap is unused)."""
    runs, gaps = np.asarray(runs, np.int64), np.asarray(gaps, np.int64)
    pos = np.zeros(2 * runs.size, np.int64)
    pos[0::2] = lead + np.concatenate([[0], np.cumsum(runs + gaps)[:-1]])
    pos[1::2] = pos[0::2] + runs
    return pos


@functools.lru_cache(maxsize=None)
def large_lists():
    """{name: (pos int64, len)} with len = 2^31 - 1.  Nothing here is ever expanded to samples."""
    out = {}
    rng = np.random.RandomState(31)
    draw = lambda n: rng.randint(1 << 26, 1 << 27, n).astype(np.int64)
    # (a) 9 runs, runs and silences of 2^26 .. 2^27 samples: every shift of a position is a large number
    lead, runs, gaps = int(draw(1)[0]), draw(9), draw(9)
    out["a"] = (_list_from(lead, runs, gaps), LARGE_LEN)
    # (d) its kind-3 variant: no lead, and the last run moved to end at len
    pos = _list_from(0, runs, gaps)
    pos[-2:] += LARGE_LEN - pos[-1]
    out["a3"] = (pos, LARGE_LEN)
    # (b) 12 runs of about 1.2e8 samples with silences of 1 to 40: ones above 2^30
    runs = 120000000 + rng.randint(-1000000, 1000001, 12).astype(np.int64)
    out["b"] = (_list_from(int(rng.randint(1, 41)), runs, rng.randint(1, 41, 12)), LARGE_LEN)
    # (c) 2 050 short runs whose last ends at len: a lead of about 2^31 - 2^17
    pos, length = cases.random_list(rng, 2049, kind=2)
    out["c"] = (pos + (LARGE_LEN - length), LARGE_LEN)
    # (d) its kind-3 variant: run 0 at sample 0, every other run moved to the end (unit 0 spans nearly 2^31 samples)
    pos, length = cases.random_list(rng, 2049, kind=3)
    pos = pos.copy()
    pos[2:] += LARGE_LEN - length
    out["c3"] = (pos, LARGE_LEN)
    return out


def ones_of(pos):
    return int((pos[1::2] - pos[0::2]).sum())


# ---- tiny files for null_test_lists / stability_test_lists ----------------------------------------------------------------
TINY_W = 400
TINY_BLOCKS = (1, 2, 64)
TINY_K = (1, 2, 5, 6)
TINY_K_MAX = max(TINY_K)
TINY_TOL = 8
# (reference samples, reference levels, subtitle runs, subtitle samples, subtitle levels, seed, how the subtitle is made)
TINY_FILES = (
    (3000, (0.0, 1.0), 0, 2500, (0.0, 1.0), 0x00001234, "random"),
    (1777, (0.25, 1.0), 1, 2000, (0.0, 1.0), 0xFFFFFFFF, "random"),
    (5003, (0.0, 1.0), 2, 4100, (0.0, 0.5), 0, "random"),
    (3000, (0.25, 1.0), 3, 3300, (0.0, 0.5), 0x80000000, "random"),
    (1777, (0.0, 1.0), 9, 1500, (0.0, 1.0), 77, "random"),
    (5003, (0.0, 1.0), 40, 4000, (0.0, 1.0), 0xDEADBEEF, "slice"),
    (3000, (0.0, 1.0), 9, 2800, (0.0, 0.5), 5, "slice"),
)


def frames_vector(rng, length):
    """A 0/1 vector of random 10-sample frames."""
    return np.repeat(rng.rand((length + 9) // 10) < 0.5, 10)[:length].astype(np.uint8)


@functools.lru_cache(maxsize=None)
def tiny_file(i):
    """(reference 0/1 vector, subtitle pos int64, subtitle 0/1 vector) of file i.  "slice": the first runs of the
    reference from sample 150 on, so the subtitle matches its reference at offset 150; "random": runs of 5 to 60 samples."""
    ref_len, _, runs, sub_len, _, _, how = TINY_FILES[i]
    rng = np.random.RandomState(900 + i)
    ref = frames_vector(rng, ref_len)
    if how == "slice":
        pos = sm.boundaries(ref[150:150 + sub_len])[:2 * runs]
    else:
        run = rng.randint(5, 61, runs)
        gap = rng.randint(5, 101, runs)
        pos = _list_from(int(rng.randint(1, 200)), run, gap) if runs else np.zeros(0, np.int64)
    assert pos.size == 2 * runs and (pos.size == 0 or int(pos[-1]) <= sub_len)
    return ref, pos, sm.expand(pos, sub_len)


@functools.lru_cache(maxsize=None)
def tiny_model(i, block):
    """The models' K_MAX + 1 records of file i at block size ``block`` (surrogate / half-sample s does not depend on K, so
    the records of a smaller K are the first K + 1): dict(null=(scores, flags), half=(scores, offsets, flags))."""
    ref, _, sub = tiny_file(i)
    _, ref_lv, _, _, sub_lv, seed, _ = TINY_FILES[i]
    return dict(null=sm.null_scores(ref, sub, ref_lv, sub_lv, TINY_W, seed, TINY_K_MAX, block),
                half=stm.half_records(ref, sub, ref_lv, sub_lv, TINY_W, seed, TINY_K_MAX, block))


def tiny_null_record(i, block, k):
    sc, fl = tiny_model(i, block)["null"]
    return sm.stats(sc[:k + 1], fl[:k + 1])


def tiny_half_record(i, block, k):
    sc, off, fl = tiny_model(i, block)["half"]
    return stm.offset_stats(sc[:k + 1], off[:k + 1], fl[:k + 1], TINY_TOL)


def silent_record(i):
    """``exact_reference.candidate`` of file i's reference against the all-zero subtitle of the file's length."""
    import exact_reference as er

    ref, _, sub = tiny_file(i)
    _, ref_lv, _, _, sub_lv, _, _ = TINY_FILES[i]
    return er.candidate(ref, np.zeros(sub.size, np.uint8), ref_lv, sub_lv, TINY_W)


# ---- tiny tracks for null_sync / stable_sync -------------------------------------------------------------------------------
TRACK_SECONDS = 4
TRACK_W = 400
TRACK_K = 16
TRACK_SEED = 3
TRACK_MIN_Z = 6.7
TRACK_TOL, TRACK_MIN_SHARE = 8, 0.5
TRACK_CUES = ((1, 0), (2, 0), (3, 0), (9, 0), (9, 8))  # (cues, of them metadata)


@functools.lru_cache(maxsize=None)
def track_problems():
    """[(reference float64 of 3 000 samples at 100 Hz, (start_us, end_us, is_metadata))]."""
    out = []
    for i, (cues, meta) in enumerate(TRACK_CUES):
        rng = np.random.RandomState(1200 + i)
        ref = frames_vector(rng, 3000).astype(np.float64)
        start = np.sort(rng.choice(np.arange(10, 250), cues, replace=False)).astype(np.int64) * 100000  # 0.1 s grid
        end = start + rng.randint(4, 20, cues).astype(np.int64) * 100000 + 30000
        flag = np.zeros(cues, np.uint8)
        flag[rng.permutation(cues)[:meta]] = 1
        out.append((ref, (start, end, flag)))
    return out


@functools.lru_cache(maxsize=None)
def track_null_model(i):
    ref, track = track_problems()[i]
    return sm.null_sync(ref, track, TRACK_W, None, TRACK_K, 1, TRACK_SEED, i, TRACK_MIN_Z)


@functools.lru_cache(maxsize=None)
def track_stable_model(i):
    ref, track = track_problems()[i]
    return stm.stable_sync(ref, track, TRACK_W, None, TRACK_K, 1, TRACK_SEED, i, TRACK_TOL, TRACK_MIN_SHARE)
