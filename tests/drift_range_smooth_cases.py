"""TEST INFRASTRUCTURE ONLY -- the seeded small problems tests/test_drift_range_smooth_host.py and
tests/test_gpu_drift_range_smooth.py share, and the model's answers to them (computed once per process).

``small_problems``: R and S in 700..9000, K in {256, 512, 1024}, levels other than 0/1, penalties {0, 60, inf}, max_step
0..7, step costs {0, 1, 16, 128}, lag ranges of six kinds (the full overlap range, asymmetric, lag_lo > 0, past both
overlap edges, [-W+1, W], no overlap at all) plus ranges of L = 1, 5, 63, 65 and 2049 lags around the true offset,
crossed with knot_blocks {1, 2, 3, 8, 16, 256}, radius {0, 1, 5, 16} and bend_cost {0, 1, 64, 1e6}.  Three made by hand
follow them: 70 blocks fitted with a knot on every block, a path that climbs 7 samples per block under knot_blocks = 256
(the widest band row), and a short file whose last interval is longer than knot_blocks.
"""
import numpy as np

import cut_model as cm
import drift_range_smooth_model as drsm

KNOT_BLOCKS = (1, 2, 3, 8, 16, 256)
RADII = (0, 1, 5, 16)
BEND_COSTS = (0.0, 1.0, 64.0, 1e6)
EXTRA_L = (1, 5, 63, 65, 2049)
N_RANDOM = 30


def _reference(rng, R):
    seg = np.maximum(1, rng.geometric(1.0 / 50.0, size=R // 20 + 16))
    rb = np.repeat(rng.rand(seg.size) < 0.45, seg)[:R]
    return np.concatenate([rb, np.zeros(R - rb.size, bool)])


def _problem(rb, sb, r_lv, s_lv, **kw):
    rb, sb = rb.copy(), sb.copy()
    rb[0], rb[1], sb[0], sb[1] = True, False, True, False  # both levels present
    return dict(ref=np.where(rb, r_lv[1], r_lv[0]), sub=np.where(sb, s_lv[1], s_lv[0]), rb=rb, sb=sb, r_lv=r_lv, s_lv=s_lv,
                **kw)


def _random(seed):
    rng = np.random.RandomState(9300 + seed)
    R, S = int(rng.randint(700, 9001)), int(rng.randint(700, 9001))
    k = int(rng.choice([256, 512, 1024]))
    r_lv = [(0.0, 1.0), (-1.0, 2.5), (0.3, 0.8)][seed % 3]
    s_lv = [(0.0, 1.0), (0.0, 24.0 / 25.0), (-0.5, 1.25)][(seed // 3) % 3]
    rb = _reference(rng, R)
    sh0 = int(rng.randint(-S // 2, R // 2))
    every = int(rng.randint(100, 600))  # drifts away one sample every `every` samples, then a break
    cut = int(rng.randint(0, S + 1))
    i = np.arange(S)
    idx = i + sh0 + i // every + np.where(i < cut, 0, int(rng.randint(-1500, 1501)))
    sb = np.zeros(S, bool)
    ok = (idx >= 0) & (idx < R)
    sb[ok] = rb[idx[ok]]
    sb ^= rng.rand(S) < 0.08
    s = seed % 8
    kind = seed % 6
    if seed >= N_RANDOM:
        length = EXTRA_L[seed - N_RANDOM]
        lo = sh0 - int(rng.randint(0, length))  # around the true offset
        hi = lo + length - 1
    elif kind == 0:
        lo, hi = cm.full_range(R, S)
    elif kind == 1:
        lo, hi = -int(rng.randint(1, S)), int(rng.randint(0, 3 * R))
    elif kind == 2:
        lo = int(rng.randint(1, R))
        hi = lo + int(rng.randint(0, 4000))
    elif kind == 3:
        lo = -S - int(rng.randint(0, 2000))
        hi = R + int(rng.randint(1, 3000))
    elif kind == 4:
        w = int(rng.randint(1, 5000))
        lo, hi = -w + 1, w
    else:
        lo = R + int(rng.randint(0, 5000)) if seed % 2 else -S - int(rng.randint(5000, 9000))
        hi = lo + int(rng.randint(0, 5000))
    return _problem(rb, sb, r_lv, s_lv, k=k, p=[0.0, 60.0, np.inf][(seed // 2) % 3], s=s,
                    q=[0.0, 1.0, 16.0, 128.0][(seed // 8 + seed) % 4], lo=lo, hi=hi, m=KNOT_BLOCKS[seed % 6],
                    r=RADII[(seed // 6 + seed) % 4], lam=BEND_COSTS[(seed // 3) % 4])


def _ramp(seed, k, n_blocks, per_block, lag0, **kw):
    """A subtitle whose true offset climbs ``per_block`` samples per block from ``lag0``, a little noise on top."""
    rng = np.random.RandomState(seed)
    rb = rng.rand(n_blocks * k + abs(lag0) + abs(per_block) * n_blocks + 64) < 0.5
    i = np.arange(n_blocks * k - 5)
    sb = rb[i + lag0 + per_block * (i // k)]
    sb ^= rng.rand(sb.size) < 0.02
    return _problem(rb, sb, (0.0, 1.0), (0.0, 1.0), k=k, **kw)


def small_problems():
    out = [_random(seed) for seed in range(N_RANDOM + len(EXTRA_L))]
    # 70 blocks in one segment, a knot on every block: 69 intervals
    out.append(_ramp(1, 256, 70, 1, 300, p=np.inf, s=2, q=1.0, lo=-500, hi=1500, m=1, r=1, lam=1.0))
    # 7 samples per block under M = 256: one interval whose band is as wide as a band row can be asked to be
    out.append(_ramp(2, 256, 14, 7, 200, p=np.inf, s=7, q=0.0, lo=-300, hi=2100, m=256, r=16, lam=0.0))
    # 12 blocks, M = 8: n = 11 gives one interval of 11 blocks, longer than M
    out.append(_ramp(3, 256, 12, -1, 40, p=np.inf, s=1, q=1.0, lo=-64, hi=64, m=8, r=5, lam=1.0))
    return out


SMALL = small_problems()
_MODEL = {}


def model(i):
    """``drift_range_smooth_model.solve`` of SMALL[i], computed once and left unchanged."""
    if i not in _MODEL:
        pr = SMALL[i]
        _MODEL[i] = drsm.solve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], pr["lo"], pr["hi"], pr["p"], pr["s"],
                               pr["q"], pr["m"], pr["r"], pr["lam"])
    return _MODEL[i]


def coverage():
    """What the set holds, from the model's answers: the counts both test files assert on."""
    import drift_report_model as drm
    import drift_smooth_model as dsm

    c = dict(one_block=0, two_block=0, last_shorter=0, last_longer=0, most_intervals=0, most_segments=0, widest_step=0,
             knot_outside=0, moved=0)
    for i, pr in enumerate(SMALL):
        (off, _, jump, _), smooth, _, _ = model(i)
        segs = drm.segments_of(jump)
        c["most_segments"] = max(c["most_segments"], len(segs))
        c["moved"] += int((smooth != off).sum())
        n_int = 0
        for f, e in segs:
            c["one_block"] += e - f == 1
            c["two_block"] += e - f == 2
            ks = dsm.knots_of(f, e, pr["m"])
            n_int += len(ks) - 1
            if len(ks) > 1:
                last = ks[-1] - ks[-2]
                c["last_shorter"] += last < pr["m"]
                c["last_longer"] += last > pr["m"]
            steps = np.abs(np.diff(off[f:e]))
            if pr["m"] == 256 and pr["s"] == 7 and steps.size and steps.max() == 7:
                c["widest_step"] += 1
            for kb in ks:
                c["knot_outside"] += off[kb] - pr["r"] < pr["lo"] or off[kb] + pr["r"] > pr["hi"]
        c["most_intervals"] = max(c["most_intervals"], n_int)
    return c
