"""TEST INFRASTRUCTURE ONLY -- the groups added for the segment path report over a lag range, shared by
tests/test_drift_range_report_host.py (the model and the reference on the CPU) and tests/test_gpu_drift_range_report.py
(the device).  The range groups themselves are tests/test_gpu_split_optimum.py's (``report_cases.range_pairs``) and the
settings ``report_cases.SEGMENT_SETTINGS``; here are the shapes the report alone needs, all over ASYMMETRIC ranges and
built from tests/report_cases.py's constructions: more than eight segments beside a one-segment pair, more than 1024
blocks, an offset spread of more than 1024 lags with a step every block, 1024-word blocks over the full range, a shift
set of one shift and neighbour shifts outside the shift set."""
import math

import report_cases as rc

EXTRA_NAMES = ("rounds", "long", "wide", "words", "single", "edge288", "edge800")


def _at(pr, lo, hi):
    return dict(pr, lo=lo, hi=hi)


def extra_groups():
    """{name: (K, pairs, [(P, max_step, Q)])}."""
    win = rc.extra_window_groups()
    rng = rc.extra_range_groups()
    out = {}
    # more than 8 segments (24 blocks of 256, a break every second block, range [-500, 1500], P = 0.5) beside a pair of
    # one segment: reused rows, slots past the count beside full ones
    k, (many,) = rng["rounds"]
    one = win["rounds"][2][1]
    out["rounds"] = (k, [many, _at(one, -500, 1500)], [(0.5, 1, 16.0), (0.5, 0, 1.0)])
    # more than 1024 blocks, jumps at blocks 1023, 1024 and 1025
    k, _, (pr,), settings = win["long"]
    out["long"] = (k, [_at(pr, -45, 60)], settings)
    # an offset spread of at least 1024 lags with a step every block (max_step 7, Q = 0, K = 256: 8-word items); the
    # second pair is periodic, its flat maximum ties across the 1024-lag chunks
    k, _, pairs, settings = win["wide"]
    out["wide"] = (k, [_at(pr, -900, 1100) for pr in pairs], settings)
    # K = 32 768 over the full range: 1024-word blocks, more than one work item per run
    k, (pr,) = rng["words"]
    out["words"] = (k, [pr], [(60.0, 2, 1.0), (3.0, 0, 1.0)])
    # a shift set of exactly one shift: the range [0, 1], a path that visits both lags
    k, _, (pr,), settings = win["single"]
    out["single"] = (k, [_at(pr, 0, 1)], settings)
    # neighbour shifts outside the shift set (NaN inside a pair)
    for name in ("edge288", "edge800"):
        k, w, (pr,), settings = win[name]
        out[name] = (k, [_at(pr, -w + 1, w)], settings)
    return out


def conditions_hold(facts):
    """What the comparison over the range groups and the added groups must have covered (``report_reference.Facts``)."""
    return (facts.first_1024 >= 1 and facts.single_shift >= 1 and facts.nan_inside >= 1 and facts.flat_second_chunk >= 1
            and facts.no_overlap >= 2 and facts.stepping >= 10)


assert all(math.isfinite(q) for g in extra_groups().values() for _, _, q in g[2])
