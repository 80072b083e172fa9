"""The rule by which device records are compared with the exact reference (tests/exact_reference.py), shared by the GPU
suites that pin records bit for bit: offset and flags equal, the score bit-identical except for the sign of an exact
0.0, the pair record the first maximal candidate after the offset filter.  numpy only."""
import numpy as np

import exact_reference as er

FLAG_DIRECT = 8


def _same_score(got, want):
    """Bit-identical, except that an exact 0.0 may carry either sign."""
    if want == 0.0:
        return got == 0.0
    return np.float64(got).tobytes() == np.float64(want).tobytes()


def check(out, want, tag, direct=False, probs=None, filter_max=None):
    """Every candidate and pair record equals the exact reference; returns the number of tie records checked.

    ``probs`` given: FFS_FLAG_AMBIGUOUS is accepted where the call's exhaustive pool overflowed -- then the record's score
    is the exact score at its offset, at most the maximum, and the pair record is the first maximal candidate of the
    device's own candidate records (``filter_max`` the call's offset filter).  Without ``probs`` the flag fails."""
    cres, pres = out
    assert len(pres) == len(want)
    bad, ties = [], 0
    for i, (recs, win) in enumerate(want):
        ambiguous = False
        for j, r in enumerate(recs):
            c = cres[i, j]
            got = (int(c["offset"]), float(c["score"]), int(c["flags"]))
            flags = r["flags"] | (FLAG_DIRECT if direct else 0)
            if probs is not None and got[2] & 2:
                name, ref01, cands01, rl, cl = probs[i]
                at = er.score_at(ref01, cands01[j], rl, cl[j], got[0])
                if got[2] != flags | 2 or not _same_score(got[1], at) or at > r["score"]:
                    bad.append((tag, i, j, "ambiguous", got, at, r))
                ambiguous = True
                continue
            if got[0] != r["offset"] or not _same_score(got[1], r["score"]) or got[2] != flags:
                bad.append((tag, i, j, got, (r["offset"], r["score"], flags, r["n_at_max"])))
            ties += r["n_at_max"] >= 2
        p = pres[i]
        if ambiguous:
            dev = [dict(score=float(c["score"]), offset=int(c["offset"]), flags=0) for c in cres[i]]
            win = er.pair(dev, filter_max)
        if int(p["best_cand"]) != win["best_cand"] or (win["best_cand"] >= 0 and (
                int(p["offset"]) != win["offset"] or not _same_score(float(p["score"]), win["score"]))):
            bad.append((tag, i, "pair", (int(p["best_cand"]), int(p["offset"]), float(p["score"])), win))
    assert not bad, (len(bad), bad[:6])
    return ties
