"""TEST INFRASTRUCTURE ONLY -- the numpy / Python-integer model of the adaptive energy VAD, the second
statement of the definitions in include/ffsubsync_amd.h (ffs_vad_levels, ffs_vad_level_hist, ffs_vad_pick_threshold,
ffs_vad_level_labels).  The device must equal it bit for bit.  Reuses ingest_reference.frame_sums for the exact frame
sums; everything else is restated here.  The case builders are shared by tests/test_adaptive_vad_host.py (CPU: the
conditions on the inputs) and tests/test_gpu_adaptive_vad.py (GPU: the very same inputs).

The rule is the project's own: there is no upstream counterpart to compare against."""
from fractions import Fraction

import numpy as np

import ingest_reference as ir

MAX_EDGES, MAX_BINS, MAX_FRAMES = 255, 256, 1 << 23
OTSU, FLOOR = 0, 1
RULES = {"otsu": OTSU, "floor": FLOOR}
FALLBACK, TOO_LONG, EMPTY, FLAT, CLAMPED_LO, CLAMPED_HI = 1, 2, 4, 8, 16, 32
FIELDS = ("threshold_bin", "flags", "floor_bin", "top_bin", "n_frames", "n_counted", "n_speech", "eta")

# launch geometry of ffs_vad_level_hist (csrc/ffs_adaptive_vad.h): at most HIST_MAX_BLOCKS workgroups of 256 threads, 16
# level bytes per thread and trip; the unaligned head and the tail of the buffer go through workgroup 0
HIST_MAX_BLOCKS, HIST_BYTES_PER_TRIP = 16, 256 * 16
HIST_TWO_TRIPS = 2 * HIST_MAX_BLOCKS * HIST_BYTES_PER_TRIP + 3 * HIST_BYTES_PER_TRIP + 17   # 143 377: all 16 workgroups take >= 2 trips
HIST_IDLE = HIST_BYTES_PER_TRIP + 1   # 4097: two workgroups are launched, 256 vectors and one tail byte: the second has no work
HIST_COUNTS = (0, 1, 15, 16, 17, HIST_IDLE, HIST_TWO_TRIPS)


def default_edges():
    """10^(k / 20) for k = 1 .. 191 as the package builds it: half-dB steps of the mean square, 192 level bins."""
    return np.array([10.0 ** ((k * 0.5) / 10.0) for k in range(1, 192)], dtype=np.float64)


def levels_of_sums(sums, counts, edges):
    """level = #{k : float64(E) >= edges[k] * float64(n)}: one fp64 multiply and one compare per edge."""
    e = np.asarray(sums, np.int64).astype(np.float64)[:, None]
    n = np.asarray(counts, np.int64).astype(np.float64)[:, None]
    edges = np.asarray(edges, np.float64)[None, :]
    out = np.empty(e.shape[0], np.uint8)
    for o in range(0, e.shape[0], 65536):   # in pieces: half a million frames times 191 edges at once is too much memory
        out[o:o + 65536] = (e[o:o + 65536] >= edges * n[o:o + 65536]).sum(axis=1)
    return out


def frame_levels(pcm, frame_len, edges):
    sums, counts = ir.frame_sums(pcm, frame_len)
    return levels_of_sums(sums, counts, edges)


def edge_distance(pcm, frame_len, edges):
    """Smallest relative distance |E - edge n| / (edge n) of any frame from any edge: rounding cannot move a level when
    this is far above 2^-52.  Pairs where the comparison is exact in integers (an integer edge times n below 2^53) are
    left out -- a frame may sit exactly on those."""
    sums, counts = ir.frame_sums(pcm, frame_len)
    edges = np.asarray(edges, np.float64)
    exact = np.array([float(e).is_integer() and e * 4800 < 2.0 ** 53 for e in edges])
    if exact.all() or not sums.size:
        return np.inf
    t = edges[None, ~exact] * counts.astype(np.float64)[:, None]
    return float(np.min(np.abs(sums.astype(np.float64)[:, None] - t) / t))


def level_hist(levels, n_bins):
    return np.bincount(np.asarray(levels, np.uint8), minlength=256)[:n_bins].astype(np.uint32)


def otsu_scores(hist, lo_bin):
    """[(t, d, m)] in exact Python integers for every t in lo_bin + 1 .. B - 1 with 0 < n0 < N'."""
    h = [int(x) if b >= lo_bin else 0 for b, x in enumerate(hist)]
    N, S = sum(h), sum(b * x for b, x in enumerate(h))
    out, n0, s0 = [], 0, 0
    for t in range(1, len(h)):
        n0 += h[t - 1]
        s0 += (t - 1) * h[t - 1]
        if t > lo_bin and 0 < n0 < N:
            out.append((t, S * n0 - N * s0, n0 * (N - n0)))
    return out


def otsu_exact(hist, lo_bin):
    """(smallest t of the largest d^2 / m in exact rational arithmetic, whether a different t comes within 2^-50 of it
    relatively -- a case where fp64 rounding could decide), or (None, False)."""
    scores = [(t, Fraction(d * d, m)) for t, d, m in otsu_scores(hist, lo_bin)]
    if not scores:
        return None, False
    best = max(v for _, v in scores)
    t_best = min(t for t, v in scores if v == best)
    close = any(v != best and best - v <= best * Fraction(1, 1 << 50) for _, v in scores)
    return t_best, close


def pick(hist, rule=OTSU, lo_bin=20, t_min=21, t_max=None, fallback_bin=100, floor_ppm=50000, margin_bins=12):
    """The record of one histogram as a dict of Python numbers (FIELDS)."""
    hist = [int(x) for x in hist]
    B = len(hist)
    t_max = B - 1 if t_max is None else t_max
    assert rule in (OTSU, FLOOR) and 0 <= lo_bin < t_min <= t_max <= B - 1 and 0 <= fallback_bin <= B
    h = [x if b >= lo_bin else 0 for b, x in enumerate(hist)]
    total, N = sum(hist), sum(h)
    S, Q = sum(b * x for b, x in enumerate(h)), sum(b * b * x for b, x in enumerate(h))
    occupied = [b for b, x in enumerate(h) if x]
    rec = dict(flags=0, eta=0.0, floor_bin=-1, top_bin=occupied[-1] if occupied else -1, n_frames=total, n_counted=N)
    if N:
        need, c = max(1, (N * floor_ppm + 999999) // 1000000), 0
        for b, x in enumerate(h):
            c += x
            if c >= need:
                rec["floor_bin"] = b
                break
    thr = fallback_bin
    if total > MAX_FRAMES:
        rec["flags"] = TOO_LONG | FALLBACK
    elif N == 0:
        rec["flags"] = EMPTY | FALLBACK
    else:
        have = True
        if rule == OTSU:
            best_v, best_t = -1.0, None
            for t, d, m in otsu_scores(hist, lo_bin):
                v = (float(d) * float(d)) / float(m)   # int -> float rounds to nearest; one multiply, one divide
                if v > best_v:
                    best_v, best_t = v, t
            if best_t is None:
                rec["flags"], have = FLAT | FALLBACK, False
            else:
                thr, rec["eta"] = best_t, best_v / float(N * Q - S * S)
        else:
            thr = rec["floor_bin"] + margin_bins
            if len(occupied) == 1:
                rec["flags"] |= FLAT
        if have:
            if thr < t_min:
                thr, rec["flags"] = t_min, rec["flags"] | CLAMPED_LO
            elif thr > t_max:
                thr, rec["flags"] = t_max, rec["flags"] | CLAMPED_HI
    rec["threshold_bin"] = thr
    rec["n_speech"] = sum(hist[thr:])
    return rec


def speech(levels, threshold_bin):
    return np.asarray(levels, np.uint8).astype(np.int64) >= int(threshold_bin)


def detect(pcm, frame_len, edges=None, **pick_args):
    """(speech flags, record, levels) of a whole file."""
    edges = default_edges() if edges is None else edges
    levels = frame_levels(pcm, frame_len, edges)
    rec = pick(level_hist(levels, len(edges) + 1), **pick_args)
    return speech(levels, rec["threshold_bin"]), rec, levels


def record_tuple(rec):
    """The record's fields with eta as its bit pattern, for bit-for-bit comparison."""
    return tuple(int(rec[f]) for f in FIELDS[:-1]) + (np.float64(rec["eta"]).view(np.uint64).item(),)


def gain_files():
    """(frame_len, {gain in dB: int16 PCM}): one file at three gains by integer-exact scaling (x 32, x 8, x 1 of the same
    small integers, so every frame's sum of squares scales by exactly 1024, 64 and 1: 0, -12.04 and -30.1 dB).  Runs of
    speech (uniform in +-120: 36.8 dB at x 1, 66.9 dB at x 32) 30.8 dB above a floor (uniform in +-3: 6 dB at x 1), a
    short last frame."""
    rng = np.random.RandomState(30)
    fl, n_frames = 160, 3000
    runs = np.maximum(1, rng.geometric(1.0 / 40.0, size=n_frames))
    is_speech = np.repeat(rng.rand(runs.size) < 0.4, runs)[:n_frames]
    amp = np.repeat(np.where(is_speech, 120, 3), fl)
    base = np.rint(rng.uniform(-1.0, 1.0, size=n_frames * fl) * amp).astype(np.int64)[:-57]
    return fl, {0: (base * 32).astype(np.int16), -12: (base * 8).astype(np.int16), -30: base.astype(np.int16)}


# ---- edge tables of the level sweep -----------------------------------------------------------------------------------


def edge_tables():
    """name -> table: the default, one edge, 255 edges (every lane makes four compares), 64 and 65 edges (either side of
    the lane-stride boundary).  The non-default tables mix the exact decades in, so the frames of
    ingest_reference.energy_pool that sit exactly at, one below and one above 10^k n meet an edge there too."""
    def spaced(n):   # n ascending edges from 10^0.05 to 10^9.55, the decades 1e0 .. 1e9 exact where they fall in
        e = np.array([10.0 ** (0.05 + 9.5 * k / max(n - 1, 1)) for k in range(n)], np.float64)
        for d in range(10):
            e[int(np.argmin(np.abs(np.log10(e) - d)))] = 10.0 ** d
        assert np.all(np.diff(e) > 0)
        return e
    return {"default": default_edges(), "one": np.array([1e5]), "255": spaced(255), "64": spaced(64), "65": spaced(65)}


# ---- histograms of the pick table ----------------------------------------------------------------------------------------


def pick_cases():
    """(name, histogram, keyword arguments of pick): two spikes, the symmetric plateau (the lowest t wins), one occupied
    bin, everything below lo_bin, totals of exactly 2^23 and 2^23 + 1 split between lo_bin and bin 255, both clamps, the
    FLOOR count exactly at need and one short of it, n_bins 2 and 256, random shapes."""
    def hist(B, **bins):
        h = np.zeros(B, np.uint32)
        for b, x in bins.items():
            h[int(b[1:])] = x
        return h
    rng = np.random.RandomState(26)
    cases = [
        ("two spikes", hist(192, b40=7000, b41=900, b95=2500, b96=300), {}),
        ("two spikes, silence below lo_bin", hist(192, b0=50000, b3=9, b40=7000, b95=2500), {}),
        ("plateau", hist(4, b0=5, b3=5), dict(lo_bin=0, t_min=1, fallback_bin=2)),
        ("plateau above lo_bin", hist(192, b30=11, b33=11), {}),
        ("one bin: FLAT", hist(192, b77=1234), {}),
        ("one bin: FLAT, floor", hist(192, b77=1234), dict(rule=FLOOR)),
        ("all below lo_bin: EMPTY", hist(192, b0=999, b19=5), {}),
        ("all below lo_bin: EMPTY, floor", hist(192, b0=999, b19=5), dict(rule=FLOOR)),
        ("all zero", hist(192), {}),
        ("2^23 in lo_bin and 255", hist(256, b20=1 << 22, b255=1 << 22), {}),
        ("2^23 uneven", hist(256, b20=(1 << 23) - 3, b255=3), {}),
        ("2^23 + 1: TOO_LONG", hist(256, b20=1 << 22, b255=(1 << 22) + 1), {}),
        ("2^23 + 1 with silence: TOO_LONG", hist(256, b0=1, b20=1 << 22, b255=1 << 22), dict(rule=FLOOR)),
        ("clamp low", hist(192, b21=500, b22=400, b23=300), dict(t_min=40)),
        ("clamp high", hist(192, b100=500, b180=400), dict(t_max=120)),
        ("floor clamp high", hist(192, b150=500, b185=400), dict(rule=FLOOR, margin_bins=30, t_max=170)),
        ("floor clamp low", hist(192, b21=500, b185=400), dict(rule=FLOOR, margin_bins=0, t_min=30)),
        # need = ceil(1000 * 50000 / 10^6) = 50: bins 30 + 31 hold exactly 50, or 49
        ("floor exactly at need", hist(192, b30=20, b31=30, b60=950), dict(rule=FLOOR)),
        ("floor one short of need", hist(192, b30=20, b31=29, b60=951), dict(rule=FLOOR)),
        ("floor ppm 0: need 1", hist(192, b30=1, b60=999), dict(rule=FLOOR, floor_ppm=0)),
        ("floor ppm 10^6: need all", hist(192, b30=1, b60=998, b90=1), dict(rule=FLOOR, floor_ppm=1000000, margin_bins=0)),
        ("two bins", hist(2, b0=3, b1=4), dict(lo_bin=0, t_min=1, fallback_bin=1)),
        ("two bins, one empty", hist(2, b1=4), dict(lo_bin=0, t_min=1, fallback_bin=2)),
        ("256 bins", hist(256, b25=100, b26=300, b130=200, b255=7), dict(fallback_bin=256)),
        ("fallback B", hist(192, b50=10), dict(fallback_bin=192)),
        ("fallback 0", hist(192, b50=10), dict(fallback_bin=0)),
    ]
    for i in range(12):   # bimodal level distributions with a noise floor, random sizes
        B = (192, 256, 64, 17)[i % 4]
        lo = (20, 20, 5, 0)[i % 4]
        centres = np.sort(rng.randint(lo + 1, B, 2))
        lv = np.concatenate([rng.normal(centres[0], 3.0, rng.randint(50, 200000)), rng.normal(centres[1], 4.0, rng.randint(50, 90000)),
                             np.zeros(rng.randint(0, 5000))])
        h = np.bincount(np.clip(np.rint(lv), 0, B - 1).astype(np.int64), minlength=B).astype(np.uint32)
        cases.append(("random %d" % i, h, dict(rule=(OTSU, FLOOR)[i % 3 == 2], lo_bin=lo, t_min=lo + 1, fallback_bin=min(100, B))))
    return cases


# ---- refusals of the four exports --------------------------------------------------------------------------------------


def refusal_calls():
    """(export, arguments) the library must refuse with FFS_E_INVALID and a message that starts with the export's name,
    before anything touches a device: the pointers are small integers that are never dereferenced."""
    P, Q = 4096, 8192   # stand-ins for device pointers, 16-byte aligned
    pick = lambda **kw: tuple(dict(dict(hist=P, n_hist=1, n_bins=192, rule=0, lo_bin=20, t_min=21, t_max=191, fallback_bin=100,
                                        floor_ppm=50000, margin_bins=10, records=Q, stream=None), **kw).values())
    return [
        ("ffs_vad_levels", (P, -1, 160, Q, 191, P, None)), ("ffs_vad_levels", (P, 10, 0, Q, 191, P, None)),
        ("ffs_vad_levels", (P, 10, 160, Q, 0, P, None)), ("ffs_vad_levels", (P, 10, 160, Q, 256, P, None)),
        ("ffs_vad_levels", (None, 10, 160, Q, 191, P, None)), ("ffs_vad_levels", (P, 10, 160, None, 191, P, None)),
        ("ffs_vad_levels", (P, 10, 160, Q, 191, None, None)), ("ffs_vad_levels", (P, 10, 160, Q + 4, 191, P, None)),
        ("ffs_vad_levels", (P + 1, 10, 160, Q, 191, P, None)),
        ("ffs_vad_level_hist", (P, -1, 192, Q, None)), ("ffs_vad_level_hist", (P, 10, 1, Q, None)),
        ("ffs_vad_level_hist", (P, 10, 257, Q, None)), ("ffs_vad_level_hist", (P, 10, 192, None, None)),
        ("ffs_vad_level_hist", (None, 10, 192, Q, None)), ("ffs_vad_level_hist", (P, 10, 192, Q + 2, None)),
        ("ffs_vad_level_hist", (None, 0, 192, None, None)),
        ("ffs_vad_pick_threshold", pick(n_hist=-1)), ("ffs_vad_pick_threshold", pick(n_bins=1)),
        ("ffs_vad_pick_threshold", pick(n_bins=257)), ("ffs_vad_pick_threshold", pick(rule=2)),
        ("ffs_vad_pick_threshold", pick(rule=-1)), ("ffs_vad_pick_threshold", pick(lo_bin=-1)),
        ("ffs_vad_pick_threshold", pick(lo_bin=21)), ("ffs_vad_pick_threshold", pick(t_min=100, t_max=99)),
        ("ffs_vad_pick_threshold", pick(t_max=192)), ("ffs_vad_pick_threshold", pick(fallback_bin=-1)),
        ("ffs_vad_pick_threshold", pick(fallback_bin=193)), ("ffs_vad_pick_threshold", pick(floor_ppm=-1)),
        ("ffs_vad_pick_threshold", pick(floor_ppm=1000001)), ("ffs_vad_pick_threshold", pick(margin_bins=-1)),
        ("ffs_vad_pick_threshold", pick(margin_bins=256)), ("ffs_vad_pick_threshold", pick(hist=None)),
        ("ffs_vad_pick_threshold", pick(records=None)), ("ffs_vad_pick_threshold", pick(records=Q + 4)),
        ("ffs_vad_pick_threshold", pick(hist=P + 2)),
        ("ffs_vad_level_labels", (P, -1, None, 100, 0.0, Q, None, None)), ("ffs_vad_level_labels", (P, 10, None, -1, 0.0, Q, None, None)),
        ("ffs_vad_level_labels", (P, 10, None, 257, 0.0, Q, None, None)), ("ffs_vad_level_labels", (None, 10, None, 100, 0.0, Q, None, None)),
        ("ffs_vad_level_labels", (P, 10, None, 100, 0.0, None, None, None)), ("ffs_vad_level_labels", (P, 10, Q + 2, 0, 0.0, Q, None, None)),
        ("ffs_vad_level_labels", (P, 10, None, 100, 0.0, Q + 2, None, None)),
    ]


def accepted_empty_calls():
    """(export, arguments) of a count of 0: FFS_OK, nothing launched (null pointers are fine)."""
    return [("ffs_vad_levels", (None, 0, 160, None, 191, None, None)),
            ("ffs_vad_pick_threshold", (None, 0, 192, 0, 20, 21, 191, 100, 50000, 10, None, None)),
            ("ffs_vad_level_labels", (None, 0, None, 100, 0.0, None, None, None))]


def check_refusals(lib):
    for name, args in refusal_calls():
        assert getattr(lib, name)(*args) == -1, (name, args)
        assert lib.ffs_last_error().decode().startswith(name + ": "), (name, args, lib.ffs_last_error())
    for name, args in accepted_empty_calls():
        assert getattr(lib, name)(*args) == 0, (name, args)
