"""TEST INFRASTRUCTURE ONLY -- an independent statement of the joint cue retiming for tiny cases: the
agreement A_k(delta) by per-sample loops, then the ENUMERATION OF EVERY PATH (K <= 5 live cues, radius <= 3: at most
7^5 paths).  Shares no code with tests/retime_model.py or tests/cue_model.py."""
import itertools

MAX_LAG = 1 << 31
MAX_LIVE, MAX_RADIUS = 5, 3


def live_cues(S, cues):
    """[(table index, a, e, lag)] of the cues that are neither empty nor invalid, in table order."""
    out = []
    for k, (start, end, lag) in enumerate(zip(*cues)):
        a, e = min(max(int(start), 0), S), min(max(int(end), 0), S)
        if e > a and abs(int(lag)) <= MAX_LAG:
            out.append((k, a, e, int(lag)))
    return out


def agreement(r, s, a, e, lag, delta, context):
    """Agreeing minus disagreeing samples of the window [a - m, e + m) inside s, among those whose partner is inside r."""
    total = 0
    for i in range(max(0, a - context), min(len(s), e + context)):
        j = i + lag + delta
        if 0 <= j < len(r):
            total += 1 if bool(s[i]) == bool(r[j]) else -1
    return total


def link_cost(dp, d, penalty_q, jump_q):
    w = penalty_q * abs(d - dp)
    return w if jump_q < 0 else min(w, jump_q)


def admissible(dp, d, g, keep_order):
    return not (keep_order and g >= 0 and dp > d + g)


class Reference:
    def __init__(self, r, s, cues, radius, context, penalty_q, jump_q, keep_order):
        assert radius <= MAX_RADIUS
        self.live = live_cues(len(s), cues)
        assert len(self.live) <= MAX_LIVE
        self.radius, self.penalty_q, self.jump_q, self.keep_order = radius, penalty_q, jump_q, keep_order
        self.shifts = list(range(-radius, radius + 1))
        self.A = [{d: agreement(r, s, a, e, lag, d, context) for d in self.shifts} for _, a, e, lag in self.live]
        self.gap = [0] + [(self.live[j][1] + self.live[j][3]) - (self.live[j - 1][1] + self.live[j - 1][3])
                          for j in range(1, len(self.live))]

    def value(self, path):
        """The total of a path (one shift per live cue), or None when a link is not admissible."""
        if len(path) != len(self.live) or any(abs(d) > self.radius for d in path):
            return None
        total = 0
        for j, d in enumerate(path):
            total += 64 * self.A[j][d]
            if j:
                if not admissible(path[j - 1], d, self.gap[j], self.keep_order):
                    return None
                total -= link_cost(path[j - 1], d, self.penalty_q, self.jump_q)
        return total

    def optimum(self):
        """The largest total over every admissible path (0 without a live cue)."""
        if not self.live:
            return 0
        return max(v for v in (self.value(p) for p in itertools.product(self.shifts, repeat=len(self.live))) if v is not None)
