"""The shapes of the sampled kernel tests (tests/test_gpu_sampled.py, tests/test_gpu_sampled_streams.py,
tests/test_gpu_sampled_sync.py), chosen on the host: the smallest at which the kernels of csrc/ffs_sampled.h can still
go wrong.  No device is involved here; tests/test_sampled_model_host.py checks that the lists cover what they claim.
A script is a list of appends (position, n, first_bit)."""
import numpy as np

import progressive_cases as pc

FIRST_BITS = (0, 5, 31)
LAG_COUNTS = (64, 4096, 4098)  # 2W: below a tile of k_samp_counts, one full tile, a tile and two lags
PIECE = 16384  # _native.PROG_PIECE_SAMPLES: the reference samples k_samp_counts stages at a time
MAX_INTERVALS = 256


def make_case(seed, T, S_list, W, ref_levels=(0.0, 1.0), top_k=3, exclusion=None, shifts=None, ones=(), zeros=()):
    """progressive_cases.make_case with the declared length T; ``ones`` / ``zeros``: [a, b) stretches of the reference
    forced to all speech / all silence."""
    case = pc.make_case(seed, T, S_list, W, ref_levels, top_k, exclusion, shifts)
    for a, b in ones:
        case["ref"][a:b] = True
    for a, b in zeros:
        case["ref"][a:b] = False
    case["T"] = int(T)
    return case


def with_bits(appends):
    """(a, n) pairs as a script, the first bits in turn."""
    return [(a, n, FIRST_BITS[i % 3]) for i, (a, n) in enumerate(appends)]


def edge_case():
    """2W = 64, T = 3001, candidates of three lengths.  In order: a segment beyond every subtitle's reach (alone: ov = 0
    at every lag, a flat all-0.0 curve); one sample at 0; a segment inside one word; a segment directly in front of it
    that shares its last word with it (the both-ends mask); one directly behind; 31, 32 and 33 samples; two segments
    inside one word and the one that exactly fills the hole between them; a re-report; all ones; all zeros; a segment
    ending at T."""
    case = make_case(3000, 3001, [700, 33, 1500], 32, (0.1, 1.0), top_k=4, exclusion=4, ones=[(400, 464)], zeros=[(500, 564)])
    script = with_bits([(2000, 100), (0, 1), (40, 5), (10, 30), (45, 10), (100, 31), (200, 32), (300, 33), (355, 5), (365, 5),
                        (360, 5), (600, 0), (401, 62), (500, 64), (2994, 7)])
    return case, script


def piece_case():
    """2W = 4096, T = 40 000: a segment of 16 385 samples (one more than a staged piece), then one directly in front of
    it, one directly behind, and the tail up to T."""
    case = make_case(3001, 40000, [38000, 5000], 2048, (0.0, 1.0), top_k=3, exclusion=300, shifts=[-1500, 2048])
    return case, with_bits([(5000, PIECE + 1), (4990, 10), (5000 + PIECE + 1, 33), (39000, 1000)])


def tile_case():
    """2W = 4098 (the second tile holds two lags), T = 9000, three candidate lengths: the clipping at S differs per
    candidate, one candidate is planted at the most negative lags."""
    case = make_case(3002, 9000, [9000, 33, 4000], 2049, (0.1, 1.0), top_k=8, exclusion=200, shifts=[-2047, 2049, 0])
    return case, with_bits([(3000, 200), (0, 100), (8000, 1000), (3200, 50), (100, 2900)])


def shape_cases():
    return [("edges-64", *edge_case()), ("piece-4096", *piece_case()), ("tile-4098", *tile_case())]


def slot_cases():
    """Three slots of one plan appended in the same calls, their interval counts apart: (cases, rounds of (a, n) per slot)."""
    cases = [make_case(3010, 3000, [700, 33], 32), make_case(3011, 3500, [5000], 2048, (0.1, 1.0), top_k=8, shifts=[-2000]),
             make_case(3012, 3200, [33, 700, 31], 32, top_k=8)]
    rounds = [((0, 100), (3000, 500), (50, 1)), ((200, 33), (0, 64), (52, 1)), ((100, 100), (64, 1), (54, 1)),
              ((1000, 0), (2000, 1000), (60, 1))]
    return cases, rounds


S2_SEGMENTS = ((0, 70), (70, 130), (500, 533), (533, 600), (1000, 1001), (4000, 5000), (600, 640))
S2_ORDERS = ((0, 1, 2, 3, 4, 5, 6), (6, 5, 4, 3, 2, 1, 0), (3, 0, 5, 2, 6, 1, 4))


def s2_case():
    """2W = 4098, T = 5000, and the segments [a, b) whose union is K (abutting ones among them)."""
    case = make_case(3020, 5000, [5000, 700, 33], 2049, (0.1, 1.0), top_k=4, exclusion=100)
    return case, list(S2_SEGMENTS)


def s2_scripts():
    """Six scripts that end on the same K: three orders, each with every segment in one append and cut into abutting
    appends of 1, 31, 32, 33, 64, 65, ... samples (front to back in one order, back to front in the others)."""
    _, segs = s2_case()
    out = []
    for o, order in enumerate(S2_ORDERS):
        whole, pieces = [], []
        for k in order:
            a, b = segs[k]
            whole.append((a, b - a))
            parts, at = [], a
            for n in pc.cut(b - a, "cycle"):
                parts.append((at, n))
                at += n
            pieces += parts if o == 0 else parts[::-1]
        out += [with_bits(whole), with_bits(pieces)]
    return out


def s3_case():
    """K = a prefix: 2W = 4096, the cuts of a prefix slot fed at their positions."""
    case = make_case(3030, 4130, [5000, 700], 2048, (0.1, 1.0), top_k=5, exclusion=50)
    return case, [1000, 33, 1, 0, 2000, 1096]


def s4_case():
    """The reference's lag mask is the window for every candidate at (T, S_c, W): 2W = 4096, T = 5000, reference levels
    (0, 1) so that the unread frames' 0.5 is (lo + hi) / 2.  About half of the reference is known."""
    case = make_case(3040, 5000, [5000, 4900, 5100], 2048, (0.0, 1.0), top_k=3, exclusion=300, shifts=[-700, 1200, 40])
    return case, with_bits([(1000, 600), (3000, 1000), (0, 333), (4500, 500), (1600, 64)])


def reopen_cases():
    """(a sampled problem, the prefix problem the slot is reopened on, the sampled problem it is reopened on again)."""
    return (make_case(3050, 3000, [5000], 2048, top_k=3), make_case(3051, 700, [33, 700], 32, (0.1, 1.0)),
            make_case(3052, 3100, [700], 32, (0.1, 1.0)))


def queue_case():
    """Open and six appends queued without a synchronisation: 2W = 64."""
    case = make_case(3060, 3000, [700, 5000, 33], 32, (0.1, 1.0))
    return case, with_bits([(500, 100), (0, 1), (600, 0), (100, 333), (433, 67), (2000, 1000)])


def interval_limit_case():
    """256 one-sample intervals at 0, 2, 4, ... 510; position 512 would be the 257th; position 1 joins two."""
    return make_case(3070, 3000, [700], 32, top_k=2, exclusion=8)


def refusal_case():
    return make_case(3080, 3000, [700, 33], 16)


# ---- the windows at which k_samp_counts changes shape ------------------------------------------------------------------
TILE = pc.TILE  # tile k of k_samp_counts holds the lags e = W - d in [4096 k, 4096 k + 4096)
TILE_T = 9000
TILE_SUB_LENGTHS = (33, 5000, TILE_T)  # S = 33, S = 5000 and S = T
# per window W: the lags the three candidates of case "a" and of case "b" are planted at.  Together they are the tile
# edges the window has: d = W (the first lag of tile 0) and d = -W + 1 (the last lag of the last tile); d = W - 4095
# and d = W - 4096 (the last lag of tile 0, the first of tile 1); at 2W = 8192, d = W - 8191 = -W + 1 again
# (d = W - 8192 is outside the window, as d = W - 4096 is at 2W = 4096).  The candidate of 33 samples takes the lags >= 0:
# planted below 0 it would not meet the reference at all.
TILE_PLANTS = {2048: ((2048, -2047, 2048), (2048, 2048, -2047)),
               2049: ((2049, -2048, -2047), (2049, -2047, -2046)),
               4096: ((4096, -4095, 1), (0, 1, -4095))}
TIE_SEGMENTS = ((5900, 50), (0, 50))
TIE_ISLAND = (1901, 2049)  # the lags the first segment makes reachable
LIMIT_W, LIMIT_T = pc.LIMIT_W, 3000
LIMIT_SEGMENTS = ((1001, 1999), (1000, 1), (0, 1000))  # 1999, 1 and 1000 samples, back to front


def reach(a, n, S, W):
    """(d_lo, d_hi), the lags of the window at which a subtitle of S samples meets the segment [a, a + n), or None:
    sample i in [0, S) meets reference sample i + d, so d runs over [a - S + 1, a + n - 1]."""
    lo, hi = max(a - S + 1, -W + 1), min(a + n - 1, W)
    return (lo, hi) if n > 0 and lo <= hi else None


def reach_tiles(a, n, S, W):
    """The tiles of k_samp_counts that hold a reachable lag of the segment, ascending."""
    r = reach(a, n, S, W)
    return [] if r is None else list(range(pc.tile_of(W, r[1]), pc.tile_of(W, r[0]) + 1))


def tile_script(W):
    """The appends of a tile case, T = 9000, in this order:
      1. at 2W = 8192 the one sample at 0: whatever the subtitle's length it is met at lags d <= 0 only, which is tile 1
         (every lag of tile 0 stays at ov = 0, score 0.0).  No such segment exists at 2W = 4096 (one tile) or 4098
         (a segment ending at b is met at d = b - 1 >= 0 by every subtitle long enough to reach tile 1, and d >= 0 is
         tile 0 there): these start with a segment beyond the short subtitle's reach, which leaves its curve all 0.0;
      2. [2900, 3100): for S = 5000 and S = T its lags straddle e = 4096 where the window has a second tile, and reach the
         last lag of the window; for S = 33 they stay in tile 0;
      3. a segment at 0 (at 2W = 8192, where 1. was that one: the rest of word 0 and beyond, abutting it inside the word);
      4. [3100, 3140), which abuts 2. inside word 96;
      5. the tail up to T."""
    first, at0 = ((0, 1), (1, 69)) if 2 * W == 8192 else ((7000, 100), (0, 70))
    return with_bits([first, (2900, 200), at0, (3100, 40), (TILE_T - 1000, 1000)])


def tie_case():
    """"ties-4098": one candidate of 4000 samples, the segment [5900, 5950) and then [0, 50).  After the first only the
    lags [1901, 2049] are reachable; every other lag -- e = 149 .. 4097, across the tile edge e = 4096 -- scores exactly
    0.0, and with an exclusion of 200 lags every peak after the first is picked from that run.  The second segment makes
    the island [-2048, 49] reachable, both lags of tile 1 among it."""
    case = make_case(3101, TILE_T, [4000], 2049, (0.1, 1.0), top_k=8, exclusion=200, shifts=[1950])
    return case, with_bits(TIE_SEGMENTS)


def limit_case():
    """2W = 262 144, the ABI limit (64 tiles, lpad = max_lags): T = 3000 in three segments fed back to front, S = 5000 and
    S = 200 000.  The long candidate meets the reference in tiles 31 .. 63 only."""
    case = make_case(3102, LIMIT_T, pc.LIMIT_SUB_LENGTHS, LIMIT_W, (0.1, 1.0), top_k=8, exclusion=LIMIT_W // 8,
                     shifts=[-4500, -100000])
    return case, with_bits(LIMIT_SEGMENTS)


def tile_cases():
    """(name, case, script): 2W = 4096, 4098 and 8192 with three candidates each (S = 33, 5000 and T) planted on the tile
    edges (TILE_PLANTS; two cases per window) under ``tile_script``; the tie case; the limit window on a plan of exactly
    ``max_lags`` = 262 144 (the last entry)."""
    out = []
    for i, W in enumerate(pc.TILE_WINDOWS):
        for j, plants in enumerate(TILE_PLANTS[W]):
            case = make_case(3110 + 2 * i + j, TILE_T, TILE_SUB_LENGTHS, W, (0.1, 1.0) if j else (0.0, 1.0), top_k=8,
                             exclusion=200, shifts=plants)
            out.append(("W%d-%s" % (W, "ab"[j]), case, tile_script(W)))
    out.append(("ties-4098", *tie_case()))
    out.append(("W%d-limit" % LIMIT_W, *limit_case()))
    return out


def tile_slot_cases():
    """(cases, rounds of (a, n) per slot): W = 2048, 4096 and 16 in three sampled slots appended in one call: n_tiles
    comes from the widest, so the workgroups of the surplus tiles of the narrow slots must return."""
    cases = [make_case(3120, 3000, [5000, 33], 2048, top_k=8, shifts=[-2047, 2048]),
             make_case(3121, 3000, [5000], 4096, (0.1, 1.0), top_k=8, shifts=[-4095]),
             make_case(3122, 1000, [33, 700], 16, top_k=8)]
    return cases, [((2900, 100), (0, 1), (500, 33)), ((0, 65), (1, 300), (0, 0)), ((65, 200), (2000, 1000), (533, 1))]


ROW_END_TOTALS = (3008, 3009, 3039)  # T % 32 = 0, 1, 31, and T / 32 + 2 a multiple of 16: the row has no padding words


def row_end_cases():
    """(T, [case of slot 0, case of slot 1], steps of (slot, a, n, first_bit)) for a plan of two sampled slots with
    ``max_ref_samples`` = T: slot 0 is fed a segment ending at T and then one at 0; slot 1 -- the next row of ``ref`` and
    ``pre_r`` -- is fed before and after, its later segments abutting the first inside words 0 and 1."""
    out = []
    for k, T in enumerate(ROW_END_TOTALS):
        cases = [make_case(3130 + 2 * k, T, [700, 33], 32, (0.1, 1.0), ones=[(T - 40, T)]),
                 make_case(3131 + 2 * k, T, [700, 33], 32)]
        steps = [(1, 3, 37, 5), (0, T - 40, 40, 31), (1, 0, 3, 0), (0, 0, 33, 5), (1, 40, 60, 31), (1, T - 1, 1, 0)]
        out.append((T, cases, steps))
    return out


# ---- queued and shared-stream sequences (tests/test_gpu_sampled_streams.py) --------------------------------------------
QUEUE_LENGTHS = (0, 1, 31, 32, 33, 65, 200)
# the calls of the plugged queue: (slots, (a, n) per slot, first_bit of the call).  Every slot is fed back to front, each
# segment abutting the one fed before it; slot 1 (2W = 4098) starts with the segment that ends at its T, and every
# segment of it is met in both tiles.
QUEUE_CALLS = (([2, 0, 1], [(500, 200), (600, 33), (2835, 65)], 1), ([1], [(100, 0)], 31),
               ([0, 2], [(599, 1), (469, 31)], 8), ([1, 2, 0], [(2803, 32), (404, 65), (399, 200)], 0),
               ([2], [(371, 33)], 5), ([0, 1], [(300, 0), (2603, 200)], 17),
               ([1, 0, 2], [(2602, 1), (368, 31), (339, 32)], 30), ([2, 1], [(139, 200), (2569, 33)], 13))


def queue_cases():
    """The three sampled slots of the plugged queue; every position fed is within reach of the slot's longest candidate."""
    return [make_case(3140, 3000, [700, 33], 32), make_case(3141, 2900, [5000], 2049, (0.1, 1.0), shifts=[-2047]),
            make_case(3142, 3200, [33, 700, 31], 32)]


# ten segments of one slot in scattered order, none empty: every call must change the answer
TWO_STREAM_SEGMENTS = ((900, 33), (100, 65), (899, 1), (400, 200), (165, 31), (1200, 32), (0, 64), (600, 100), (1232, 7),
                       (700, 150))


def two_stream_case():
    """One sampled slot fed from two streams in turn (calls 0, 2, 4, ... on A; 1, 3, 5, ... on B)."""
    return make_case(3150, 2000, [700, 33], 600, (0.1, 1.0))


MIXED_LENGTHS = (33, 65, 1, 200, 31, 32)  # the prefix slot's appends
MIXED_SEGMENTS = ((900, 33), (835, 65), (0, 1), (400, 200), (933, 31), (1, 32))  # the sampled slot's, in step with them


def mixed_case():
    """(the prefix problem of slot 0, the sampled problem of slot 1): one plan, about the same size."""
    return pc.make_case(3160, 700, [700, 33], 600), make_case(3161, 2000, [700, 33], 600, (0.1, 1.0))


def reopen_chain():
    """[(kind, case, appends)] of one slot reopened behind pending work: sampled -> prefix -> sampled, then sampled again
    with a shorter T, a smaller W and fewer candidates.  Appends: (a, n) of a sampled problem, n of the prefix one."""
    return [("sampled", make_case(3170, 3000, [5000, 700], 2049, shifts=[-2047, 100]), [(2000, 1000), (0, 700), (1000, 33)]),
            ("prefix", pc.make_case(3171, 700, [33, 700], 32, (0.1, 1.0)), [100, 33, 567]),
            ("sampled", make_case(3172, 3100, [700, 5000, 33], 600, (0.1, 1.0)), [(3000, 100), (50, 64), (0, 50)]),
            ("sampled", make_case(3173, 1000, [700], 16), [(600, 65), (0, 33), (665, 31)])]


def late_case():
    """One sampled slot whose candidates and chunks arrive late: (case, (a, n) per call)."""
    return make_case(3180, 3000, [31, 700, 33], 16), [(500, 200), (467, 33), (0, 65), (300, 0), (65, 31)]


# ---- end to end (tests/test_gpu_sampled_sync.py): the problems of tests/test_gpu_progressive_sync.py -----------------
SYNC_SEEDS = pc.SYNC_SEEDS
SYNC_SEGMENT, SYNC_W, SYNC_E, SYNC_TOP_K = 6000, pc.SYNC_W, pc.SYNC_E, pc.SYNC_TOP_K
SYNC_RULES = pc.SYNC_RULES
_runs = {}


def sync_model_run(seed, rule_index):
    """sampled_model.run of the seed on the spread schedule under SYNC_RULES[rule_index] (None: never settle), once."""
    import progressive_model as pm
    import sampled_model as sm

    if (seed, None) not in _runs:
        ref, _, cands, _ = pc.sync_problem(seed)
        never = dict(SYNC_RULES[0], stable_updates=None)
        _runs[(seed, None)] = sm.run(ref, cands, (0.0, 1.0), SYNC_W, sm.segment_schedule(ref.size, SYNC_SEGMENT), never,
                                     SYNC_TOP_K, SYNC_E)
    key = (seed, rule_index)
    if key not in _runs:
        full = _runs[(seed, None)]["history"]
        rule = SYNC_RULES[rule_index]
        stop = next((u for u in range(1, len(full) + 1) if pm.settled(full[:u], **rule)), None)
        h = full[:stop] if stop else full
        _runs[key] = dict(updates=len(h), settled=stop is not None, state=h[-1], history=h)
    return _runs[key]
