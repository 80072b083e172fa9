"""The shuffled-cue test's problems and the model's answers on them, computed once per process and shared between
tests/test_surrogate_model_host.py, tests/test_surrogate_host.py and tests/test_gpu_surrogate.py (a model null of one
10-minute file is 7 + 65 exact solves)."""
import functools

import numpy as np

import surrogate_model as sm

W = 6000
K = 64
SEED = 0
SYNC_SEEDS = tuple(range(6))  # workloads.synth.make_pair_spec at 10 minutes: matched i, then wrong i (track i, reference i + 1)
DURATION = 600.0
INT32_MAX = sm.INT32_MAX


@functools.lru_cache(maxsize=None)
def _spec(seed):
    from workloads import synth

    return synth.make_pair_spec(seed, duration_s=DURATION)


@functools.lru_cache(maxsize=None)
def reference(seed):
    from workloads import synth

    sp = _spec(seed)
    return synth.rasterize(sp.ref_len, sp.ref_starts, sp.ref_ends).astype(np.float64)


@functools.lru_cache(maxsize=None)
def track(seed):
    """The pair's ratio-1.0 candidate in 10 ms units, as tests/progressive_cases.py builds it."""
    sp = _spec(seed)
    j = sp.ratios.index(1.0)
    start, end = sp.cand_starts[j].astype(np.int64) * 10000, sp.cand_ends[j].astype(np.int64) * 10000
    keep = end > start
    return start[keep], end[keep], np.zeros(int(keep.sum()), np.uint8)


def sync_problems():
    """[(reference, track)]: the matched files of SYNC_SEEDS, then the wrong ones; none left out."""
    return [(reference(i), track(i)) for i in SYNC_SEEDS] + [(reference(i + 1), track(i)) for i in SYNC_SEEDS]


def sync_kinds():
    return ["matched"] * len(SYNC_SEEDS) + ["wrong"] * len(SYNC_SEEDS)


@functools.lru_cache(maxsize=None)
def model_sync(index, min_z, block_units=1):
    """``surrogate_model.null_sync`` of problem ``index`` of ``sync_problems()`` as file ``index`` of a call with SEED."""
    ref, tr = sync_problems()[index]
    return sm.null_sync(ref, tr, W, None, K, block_units, SEED, index, min_z)


# ---- lists for the byte-for-byte tests ---------------------------------------------------------------------------------
UNITS = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 8191, 8192)


def random_list(rng, units, kind=0):
    """(pos int64, len) of a valid list with ``units`` + 1 runs.  Runs and silences of 1 to 40 samples, about a third of
    them of length 1; kind 1: no silence in front of run 0; kind 2: the last run ends at ``len``; kind 3: both."""
    m = units + 1
    runs = np.where(rng.rand(m) < 0.35, 1, rng.randint(1, 41, m))
    gaps = np.where(rng.rand(m) < 0.35, 1, rng.randint(1, 41, m))
    lead = 0 if kind & 1 else int(rng.randint(1, 30))
    tail = 0 if kind & 2 else int(rng.randint(1, 30))
    pos = np.zeros(2 * m, np.int64)
    pos[0::2] = lead + np.concatenate([[0], np.cumsum(runs + gaps)[:-1]])
    pos[1::2] = pos[0::2] + runs
    return pos, int(pos[-1]) + tail


def short_block_place(seed, s, units, block_units):
    """The place of the (short) last block in surrogate s."""
    nb = (units + block_units - 1) // block_units
    return int(np.flatnonzero(sm.block_order(seed, s, nb) == nb - 1)[0])


def seed_placing_short_block(units, block_units, tries=20000):
    """A seed whose surrogates 0, 1, 2 put the last block first, last and (with more than two blocks) in the middle."""
    nb = (units + block_units - 1) // block_units
    for seed in range(tries):
        places = [short_block_place(seed, s, units, block_units) for s in range(3)]
        if places[0] == 0 and places[1] == nb - 1 and (nb <= 2 or 0 < places[2] < nb - 1):
            return seed
    raise AssertionError("no seed in %d tries" % tries)


def fmix32_inverse(h):
    """The inverse of ``surrogate_model.fmix32``: every step of the finaliser is a bijection of uint32 (an xor-shift, a
    multiplication by an odd constant), so two blocks of one surrogate -- fmix32 of two different words -- never share a
    key and the (key, b) tie rule of the contract never decides an order."""
    m = 0xFFFFFFFF
    h ^= h >> 16
    h = (h * pow(0xC2B2AE35, -1, 1 << 32)) & m
    h ^= (h >> 13) ^ (h >> 26)
    h = (h * pow(0x85EBCA6B, -1, 1 << 32)) & m
    h ^= h >> 16
    return h


def brute_force(v01, seed, s, block_units):
    """The surrogate of a 0/1 vector by the statement itself: cut the samples at the unit edges, reorder the pieces,
    re-read the runs."""
    v01 = np.asarray(v01, dtype=np.uint8)
    pos = sm.boundaries(v01)
    m = pos.size // 2
    if m <= 1:
        return v01.copy()
    u = m - 1
    pieces = [v01[pos[2 * j]:pos[2 * j + 2]] for j in range(u)]
    nb = (u + block_units - 1) // block_units
    order = sorted(range(nb), key=lambda b: (sm.key(seed, s, b), b))
    moved = [pieces[j] for b in order for j in range(b * block_units, min((b + 1) * block_units, u))]
    return np.concatenate([v01[:pos[0]]] + moved + [v01[pos[2 * u]:]])
