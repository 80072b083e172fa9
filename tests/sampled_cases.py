"""The shapes of the sampled kernel tests (tests/test_gpu_sampled.py, tests/test_gpu_sampled_sync.py), chosen on the host:
the smallest at which the kernels of csrc/ffs_sampled.h can still go wrong.  No device is involved here;
tests/test_sampled_model_host.py checks that the lists cover what they claim.  A script is a list of appends
(position, n, first_bit)."""
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
