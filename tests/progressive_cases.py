"""The shapes of the progressive kernel tests (tests/test_gpu_progressive.py), chosen on the host: the smallest at which
the kernels of csrc/ffs_progressive.h can still go wrong.  No device is involved here; tests/test_progressive_model_host.py
checks that the list covers what it claims."""
import numpy as np

TOTALS = (1, 31, 32, 33, 95, 1000, 4130)
CUTS = ("once", "ones", "cycle", "random")
FIRST_BITS = (0, 1, 8, 31)
SUB_LENGTHS = (1, 31, 33, 700, 5000)
WINDOWS = (1, 16, 33, 600, 2500)  # 2 * 2500 lags cross the 4096-lag tile of k_prog_counts
N_CANDS = (1, 3, 8)
RATIOS = (24 / 23.976, 24 / 25, 23.976 / 24, 23.976 / 25, 25 / 23.976, 25 / 24, 1.0, 1.5)  # amplitudes min(1/ratio, 1)
PIECE_SUB = 45000  # the subtitle length of the append longer than one staged piece


def cut(total, kind, seed=0):
    """The append lengths of one way to cut ``total`` samples."""
    if kind == "once":
        return [total]
    if kind == "ones":
        return [1] * total
    out, left = [], total
    if kind == "cycle":
        cyc, i = (1, 31, 32, 33, 64, 65), 0
        while left > 0:
            out.append(min(cyc[i % 6], left))
            left -= out[-1]
            i += 1
        return out
    rng = np.random.RandomState(1000 + seed)
    while left > 0:
        n = int(rng.randint(0, 201))
        out.append(0 if rng.rand() < 0.15 else min(n, left))  # lengths in [0, 200], one in seven an empty append
        left -= out[-1]
    return out


def speech(rng, n, scale=40.0, density=0.45):
    """A piecewise-constant 0/1 vector of n samples."""
    seg = np.maximum(1, rng.geometric(1.0 / scale, size=n // 4 + 16))
    v = np.repeat(rng.rand(seg.size) < density, seg)[:n]
    return np.concatenate([v, np.zeros(n - v.size, bool)])


def make_case(seed, total, S_list, W, ref_levels=(0.0, 1.0), top_k=3, exclusion=None, shifts=None):
    """dict(ref, cands=[(bits, (lo, hi))], ref_levels, W, top_k, e): candidates are noisy shifted copies of the reference
    where they can be, with amplitudes hi = 1 and min(1 / ratio, 1) in turn.  ``shifts``: the lag each candidate's copy
    is planted at, instead of a random lag of the window."""
    rng = np.random.RandomState(7000 + seed)
    ref = speech(rng, total)
    cands = []
    for c, S in enumerate(S_list):
        shift = int(rng.randint(-W + 1, W + 1))
        if shifts is not None:
            shift = int(shifts[c])
        idx = np.arange(S) + shift
        ok = (idx >= 0) & (idx < total)
        s = speech(rng, S)
        s[ok] = ref[idx[ok]]
        s ^= rng.rand(S) < 0.05
        hi = 1.0 if c % 2 == 0 else min(1.0 / RATIOS[c % len(RATIOS)], 1.0)
        cands.append((s, (0.0, hi)))
    return dict(ref=ref, cands=cands, ref_levels=tuple(ref_levels), W=int(W), top_k=top_k,
                e=int(exclusion if exclusion is not None else max(1, W // 8)))


def total_cases():
    """(name, case, cut kind, first_bit): every total cut every way it can be, cycling through the subtitle lengths, the
    windows, the candidate counts, the reference levels and the first bits so that each value of each meets several
    totals."""
    out, i = [], 0
    for total in TOTALS:
        for kind in CUTS:
            if kind == "ones" and total > 95:
                continue
            n_cand = N_CANDS[i % 3]
            S_list = [SUB_LENGTHS[(i + c) % 5] for c in range(n_cand)]
            W = WINDOWS[(i // 2 + total) % 5]
            if W == 2500 and kind in ("ones", "cycle") and total > 33:
                W = 600  # (the model's cost: the tile-crossing window meets every total in the other cuts)
            lv = (0.0, 1.0) if i % 2 == 0 else (0.1, 1.0)
            fb = FIRST_BITS[i % 4]
            case = make_case(i, total, S_list, W, lv, top_k=1 + i % 8)
            out.append(("L%d-%s-W%d-c%d-fb%d" % (total, kind, W, n_cand, fb), case, kind, fb))
            i += 1
    return out


# ---- end to end (tests/test_gpu_progressive_sync.py) ----------------------------------------------------------------
SYNC_SEEDS = tuple(range(8))
SYNC_DURATION, SYNC_CHUNK, SYNC_W, SYNC_E, SYNC_TOP_K = 600.0, 10000, 6000, 300, 3
# the shipped rule's thresholds with two stable updates (stops early enough to be seen in six chunks), and the shipped rule
SYNC_RULES = (dict(min_psr=5.0, min_margin=3.0, min_ratio_margin=0.05, stable_updates=2, offset_tolerance=2, min_samples=0),
              dict(min_psr=5.0, min_margin=3.0, min_ratio_margin=0.05, stable_updates=5, offset_tolerance=2, min_samples=0))
_sync = {}


def sync_problem(seed):
    """(reference 0/1, track, candidates [(0/1, (0, amplitude))] by the CPU rasteriser, ratios) of a synth pair at
    10 min: the track is the pair's ratio-1.0 candidate in 10 ms units, as tests/test_gpu_quality.py builds it."""
    if seed not in _sync:
        from oracle import raster_oracle
        from workloads import synth

        spec = synth.make_pair_spec(seed, duration_s=SYNC_DURATION)
        j = spec.ratios.index(1.0)
        start, end = spec.cand_starts[j].astype(np.int64) * 10000, spec.cand_ends[j].astype(np.int64) * 10000
        keep = end > start
        track = (start[keep], end[keep], np.zeros(int(keep.sum()), np.uint8))
        cands = []
        for r in spec.ratios:
            v = raster_oracle.rasterize(*track, r)
            cands.append((v > 0, (0.0, min(1.0 / r, 1.0))))
        ref = synth.rasterize(spec.ref_len, spec.ref_starts, spec.ref_ends).astype(bool)
        _sync[seed] = (ref, track, cands, list(spec.ratios))
    return _sync[seed]


_runs = {}


def sync_model_run(seed, rule_index):
    """progressive_model.run of the seed under SYNC_RULES[rule_index] (None: never settle), computed once."""
    import progressive_model as pm

    key = (seed, rule_index)
    if key not in _runs:
        ref, _, cands, _ = sync_problem(seed)
        never = dict(SYNC_RULES[0], stable_updates=None)
        if (seed, None) not in _runs:
            _runs[(seed, None)] = pm.run(ref, cands, (0.0, 1.0), SYNC_W, SYNC_CHUNK, never, SYNC_TOP_K, SYNC_E)
        if rule_index is not None:
            full = _runs[(seed, None)]["history"]
            rule = SYNC_RULES[rule_index]
            stop = next((u for u in range(1, len(full) + 1) if pm.settled(full[:u], **rule)), None)
            h = full[:stop] if stop else full
            _runs[key] = dict(updates=len(h), settled=stop is not None, state=h[-1], history=h)
    return _runs[key]


def window_cases():
    """Every window against every subtitle length at a total of 1000 (W > S, W > L and W <= S + 1 among them), one
    random cut each."""
    out = []
    for i, W in enumerate(WINDOWS):
        for j, S in enumerate(SUB_LENGTHS):
            total = 1000 if (i + j) % 3 else 95
            case = make_case(100 + 5 * i + j, total, [S], W, (0.0, 1.0) if j % 2 else (0.1, 1.0))
            out.append(("W%d-S%d-L%d" % (W, S, total), case, "random", FIRST_BITS[(i + j) % 4]))
    return out


# ---- the windows at which k_prog_counts changes shape ------------------------------------------------------------------
TILE = 4096  # PROG_TILE: the lags e = W - d of one workgroup of k_prog_counts; tile k holds e in [4096 k, 4096 k + 4096)
MAX_LAGS = 262144  # _native.PROG_MAX_LAGS: 64 tiles, lpad = max_lags
TILE_WINDOWS = (2048, 2049, 4096)  # 2W = one full tile, one full tile and two lags, two full tiles
TILE_SUB_LENGTHS = (33, 5000)
TILE_TOTALS = (1000, 4130)
LIMIT_W, LIMIT_CUTS, LIMIT_SUB_LENGTHS = MAX_LAGS // 2, (1000, 1, 1999), (5000, 200000)


def tile_of(W, lag):
    """The tile of k_prog_counts that owns lag d of a window W."""
    return (int(W) - int(lag)) // TILE


def tile_shift(W, S, total):
    """The lag a tile case plants its candidate at.  A subtitle longer than the window: the most negative lag, the last
    of the last tile, written to curve[0] (at 2W = 4098 the lag before it: the first of the two lags of tile 1).  A
    short one: the largest lag the reference reaches, W itself (the first lag of tile 0, the top of the curve) where it
    can."""
    if S > W:
        return -W + 2 if (2 * W) % TILE == 2 else -W + 1
    return min(W, total - S)


def tile_cases():
    """(name, case, append lengths, first_bit): 2W = 4096, 4098 and 8192 against a subtitle shorter and one longer than
    the window, at a total below and one above a tile, in one append and in a random cut; then the limit window
    2W = MAX_LAGS, whose long subtitle meets the reference in tiles 33 and beyond."""
    out, i = [], 0
    for W in TILE_WINDOWS:
        for S in TILE_SUB_LENGTHS:
            for total in TILE_TOTALS:
                for kind in ("once", "random"):
                    case = make_case(200 + i, total, [S], W, (0.0, 1.0) if i % 2 else (0.1, 1.0), top_k=8,
                                     shifts=[tile_shift(W, S, total)])
                    out.append(("W%d-S%d-L%d-%s" % (W, S, total, kind), case, cut(total, kind, seed=i), FIRST_BITS[i % 4]))
                    i += 1
    limit = make_case(260, sum(LIMIT_CUTS), LIMIT_SUB_LENGTHS, LIMIT_W, (0.1, 1.0), top_k=8, exclusion=LIMIT_W // 8,
                      shifts=[-4500, -100000])  # (tiles 33 and 56)
    out.append(("W%d-limit" % LIMIT_W, limit, list(LIMIT_CUTS), FIRST_BITS[i % 4]))
    return out


def tile_slot_cases():
    """(cases, append lengths per round): W = 2048, 4096 and 16 in three slots of one plan, appended in one call: n_tiles
    comes from the largest window, so the workgroups of the surplus tiles of the small slots must return."""
    cases = [make_case(270, 1000, [5000, 33], 2048, top_k=8, shifts=[-2047, 967]),
             make_case(271, 700, [5000], 4096, (0.1, 1.0), top_k=8, shifts=[-4095]),
             make_case(272, 333, [33, 700], 16, top_k=8)]
    return cases, [(200, 65, 33), (0, 1, 300), (800, 634, 0)]


def tile_e2_case():
    """(case, append lengths): W = 2048 with L = S = 2100 at the end, where the reference's own mask is the window."""
    return make_case(280, 2100, [2100], 2048, top_k=8), [1000, 1060, 39, 1]


# ---- queued and shared-stream sequences (tests/test_gpu_progressive_streams.py) ----------------------------------------
QUEUE_LENGTHS = (0, 1, 31, 32, 33, 65, 200)
# the appends of the plugged queue: (slots, n_new per slot, first_bit of the call), every slot's total within its case
QUEUE_CALLS = (([2, 0, 1], [200, 33, 65], 1), ([1], [0], 31), ([0, 2], [1, 31], 8), ([1, 2, 0], [32, 65, 200], 0),
               ([2], [33], 5), ([0, 1], [0, 200], 17), ([1, 0, 2], [1, 31, 32], 30), ([2, 1], [200, 33], 13))


def queue_cases():
    """The three slots of the plugged queue (the sizes of tests/test_gpu_progressive.py's slot cases)."""
    return [make_case(940, 700, [700, 33], 600), make_case(941, 333, [5000], 33, (0.1, 1.0)),
            make_case(942, 1000, [31, 700, 33], 16)]


TWO_STREAM_LENGTHS = (33, 65, 1, 200, 31, 32, 64, 100, 7, 150)  # no empty append: every call must change the answer


def two_stream_case():
    """One slot fed from two streams in turn (appends 0, 2, 4, ... on A; 1, 3, 5, ... on B)."""
    return make_case(950, 700, [700, 33], 600, (0.1, 1.0))


def reopen_cases():
    """(the long problem of slot 1, the short one it is reopened on, the neighbour in slot 0)."""
    return (make_case(960, 700, [5000], 600), make_case(961, 200, [33], 16, (0.1, 1.0)),
            make_case(962, 333, [700, 33], 33))
