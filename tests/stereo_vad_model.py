"""TEST INFRASTRUCTURE ONLY -- the numpy / Python-integer model of the centre-channel VAD, the second
statement of the definitions in include/ffsubsync_amd.h (ffs_vad_stereo_levels, ffs_vad_centre_gate).  The device must
equal it bit for bit.  The levels go through adaptive_vad_model.levels_of_sums with counts 4 n_f; the pick, the labels
and the steady-run gate behind the centre gate are adaptive_vad_model's and steady_gate_model's, unchanged.  The case
builders are shared by tests/test_stereo_vad_host.py (CPU: the conditions on the inputs) and
tests/test_gpu_stereo_vad.py (GPU: the very same inputs).

The rule is the project's own: there is no upstream counterpart to compare against, this model is its only reference."""
import math

import numpy as np

import adaptive_vad_model as am
import steady_gate_model as gm

MONO, ALL_REJECTED = 1, 2
FIELDS = ("threshold_bin", "flags", "min_contrast_bins", "max_side", "n_frames", "n_active", "n_kept", "sum_contrast")

# launch geometry (csrc/ffs_stereo_vad.h)
MAX_FRAME_VEC = 512             # STEREO_MAX_FRAME_VEC: pairs of the longest frame on the vector path (128 16-byte vectors)
ONE_VECTOR_MORE = MAX_FRAME_VEC + 4
SWEEP_GRID_FRAMES = 16384 * 4 * 8   # frames of one trip of the sweep's capped grid: 16384 blocks x 4 waves x 8 frames
GATE_GRID_FRAMES = 256 * 256    # frames of one trip of the centre gate's capped grid: CENTRE_MAX_BLOCKS x CENTRE_THREADS


# ---- the definitions ------------------------------------------------------------------------------------------------


def stereo_sums(pcm, frame_len):
    """(M, S, n) per frame of interleaved (L, R) int16 pairs, the short last frame included: M = sum (L + R)^2 and
    S = sum (L - R)^2 as int64 (at most 2^32 per pair: exact for every frame length used here), n the pair count."""
    x = np.asarray(pcm).astype(np.int64)
    assert x.ndim == 1 and x.size % 2 == 0
    u, v = (x[0::2] + x[1::2]) ** 2, (x[0::2] - x[1::2]) ** 2
    fl = int(frame_len)
    n_pairs = u.size
    starts = np.arange(0, n_pairs, fl)
    counts = np.minimum(fl, n_pairs - starts).astype(np.int64)
    if not n_pairs:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), counts
    return np.add.reduceat(u, starts), np.add.reduceat(v, starts), counts


def stereo_levels(pcm, frame_len, edges):
    """(mid, side): level = #{k : float64(sum) >= edges[k] * float64(4 n)}."""
    m, s, n = stereo_sums(pcm, frame_len)
    return am.levels_of_sums(m, 4 * n, edges), am.levels_of_sums(s, 4 * n, edges)


def centre_gate(mid, side, t, c):
    """(out levels, record): out = mid where mid - side >= c, else 0; active = mid >= t; kept = active and passing."""
    m, s = np.asarray(mid, np.uint8).astype(np.int64), np.asarray(side, np.uint8).astype(np.int64)
    assert m.shape == s.shape and m.ndim == 1
    contrast = m - s
    passing = contrast >= int(c)
    active = m >= int(t)
    n_active, n_kept = int(active.sum()), int((active & passing).sum())
    max_side = int(s.max()) if s.size else 0
    flags = (MONO if s.size and max_side == 0 else 0) | (ALL_REJECTED if n_active > 0 and n_kept == 0 else 0)
    rec = dict(threshold_bin=int(t), flags=flags, min_contrast_bins=int(c), max_side=max_side, n_frames=int(m.size),
               n_active=n_active, n_kept=n_kept, sum_contrast=int(contrast[active].sum()))
    return np.where(passing, m, 0).astype(np.uint8), rec


def record_tuple(rec):
    return tuple(int(rec[f]) for f in FIELDS)


def detect(pcm, frame_len, c, edges=None, steady=None, **pick_args):
    """A whole file: (speech flags, threshold record, centre record, gate record or None, mid, side).  The pick runs on
    the histogram of the mid levels of all frames; ``steady`` = (dip_bins, max_run) runs the steady-run gate on the centre
    gate's output."""
    edges = am.default_edges() if edges is None else edges
    mid, side = stereo_levels(pcm, frame_len, edges)
    thr = am.pick(am.level_hist(mid, len(edges) + 1), **pick_args)
    out, centre = centre_gate(mid, side, thr["threshold_bin"], c)
    if steady is None:
        return am.speech(out, thr["threshold_bin"]), thr, centre, None, mid, side
    speech, gate = gm.gate_vectorised(out, thr["threshold_bin"], steady[0], steady[1])
    return speech, thr, centre, gate, mid, side


def edge_distance(pcm, frame_len, edges):
    """adaptive_vad_model.edge_distance for both sums: the smallest relative distance of any frame's M or S from any
    edge times 4 n, leaving out the pairs where the comparison is exact in integers."""
    m, s, n = stereo_sums(pcm, frame_len)
    edges = np.asarray(edges, np.float64)
    exact = np.array([float(e).is_integer() and e * 4 * 4800 < 2.0 ** 53 for e in edges])
    if exact.all() or not m.size:
        return np.inf
    t = edges[None, ~exact] * (4 * n).astype(np.float64)[:, None]
    return float(min(np.min(np.abs(x.astype(np.float64)[:, None] - t) / t) for x in (m, s)))


# ---- inputs of the stereo sweep --------------------------------------------------------------------------------------

FRAME_LENS = (1, 3, 4, 5, 160, 480, MAX_FRAME_VEC, ONE_VECTOR_MORE)   # pairs; the last two are 512 and 516
START_OFFSETS = (0, 1, 2, 4)            # int16 values into a 16-byte aligned allocation: 0, 2, 4 and 8 bytes
OUT_OFFSETS = (0, 1, 3)                 # bytes behind an 8-byte boundary, for each level output
WHOLE_FRAMES = (0, 1) + tuple(range(40, 48))   # no and one frame, then every residue mod 8
POOL_FRAMES = 49                        # the longest slice plus one frame to cut a tail from
GUARD_PAIRS = 32                        # loud pairs behind every pool: a read past n_pairs changes a level
TABLES = ("default", "one", "64", "65", "255")
DECADES = (1, 5, 8)                     # decade edges 10^k of every table but "one" (10^5 only)


def tails(frame_len):
    return tuple(sorted({0, 1, frame_len - 1} & set(range(frame_len))))


def _squares(target, max_terms, vmax=32767):
    """Values up to ``vmax`` whose squares sum to ``target`` exactly, at most ``max_terms`` of them, or None: greedy
    while more than four terms are left, then a search over the last four (greedy alone wastes terms in short frames)."""
    def search(rem, terms):
        if rem == 0:
            return []
        if terms == 0 or rem > terms * vmax * vmax:
            return None
        top = min(math.isqrt(rem), vmax)
        if terms == 1:
            return [top] if top * top == rem else None
        for v in range(top, max(top - 40, 0), -1):
            rest = search(rem - v * v, terms - 1)
            if rest is not None:
                return [v] + rest
        return None
    vals, rem = [], int(target)
    if rem < 0:
        return None
    while rem > 0 and max_terms - len(vals) > 4:
        v = min(math.isqrt(rem), vmax)
        vals.append(v)
        rem -= v * v
    rest = search(rem, min(4, max_terms - len(vals)))
    return None if rest is None else vals + rest


def boundary_frame(frame_len, k, delta, which):
    """[frame_len, 2] int16 pairs with M (``which`` = "mid") or S ("side") exactly 10^k * 4 frame_len + delta and the other
    sum as small as parity allows (L + R and L - R have the same parity), or None where no such frame exists."""
    vals = _squares(10 ** int(k) * 4 * int(frame_len) + int(delta), int(frame_len))
    if vals is None:
        return None
    big = np.zeros(int(frame_len), np.int64)
    big[:len(vals)] = [v if i % 2 else -v for i, v in enumerate(vals)]
    small = big % 2                      # the other signal: 0 or 1, the same parity
    u, v = (big, small) if which == "mid" else (small, big)
    frame = np.stack([(u + v) // 2, (u - v) // 2], axis=1)
    assert np.all(np.abs(frame) <= 32767)
    frame = frame.astype(np.int16)
    m, s, _ = stereo_sums(frame.ravel(), frame_len)
    assert int((m if which == "mid" else s)[0]) == 10 ** int(k) * 4 * int(frame_len) + int(delta)
    return frame


def extreme_frames(frame_len):
    """Full scale: all samples -32768 ((L + R)^2 = 2^32 and 2 L R = 2^31 in every pair), and the two mixed-sign pairs."""
    lo, hi = np.full(frame_len, -32768), np.full(frame_len, 32767)
    return [np.stack([lo, lo], 1), np.stack([lo, hi], 1), np.stack([hi, lo], 1)]


def sweep_pool(frame_len):
    """int16 [POOL_FRAMES, frame_len, 2]: frames of correlated noise at levels across the table with every
    inter-channel relation (centred, wide, anti-phase, one channel silent), the boundary frames of DECADES at -1, 0, +1
    in M and in S, and the full-scale frames, spread so that the slots of a group of four and the frames behind the last
    group meet them."""
    rng = np.random.RandomState(2800 + int(frame_len))
    amp = 10.0 ** rng.uniform(0.3, 4.3, size=(POOL_FRAMES, 1))
    common = rng.standard_normal((POOL_FRAMES, frame_len)) * amp
    own = rng.standard_normal((2, POOL_FRAMES, frame_len)) * amp
    w = rng.choice([0.0, 0.3, 0.9, 1.0], size=(POOL_FRAMES, 1))
    sign = rng.choice([1.0, 1.0, -1.0], size=(POOL_FRAMES, 1))
    left = w * common + (1 - w) * own[0]
    right = sign * (w * common + (1 - w) * own[1]) * rng.choice([1.0, 1.0, 0.0], size=(POOL_FRAMES, 1))
    frames = np.clip(np.rint(np.stack([left, right], axis=2)), -32768, 32767).astype(np.int64)
    special = [boundary_frame(frame_len, k, d, which) for which in ("mid", "side") for k in DECADES for d in (-1, 0, 1)]
    special = [f for f in special if f is not None] + extreme_frames(frame_len)
    slots = rng.permutation(POOL_FRAMES)
    for j, slot in enumerate(slots[:min(POOL_FRAMES, 2 * len(special))]):
        frames[slot] = special[j % len(special)]
    return frames.astype(np.int16)


def sweep_buffers(frame_len):
    """{start offset: int16 buffer} = offset loud values, the pool, a loud guard."""
    guard = np.where(np.arange(2 * GUARD_PAIRS) % 3 == 0, 32767, -32768).astype(np.int16)
    pool = sweep_pool(frame_len).ravel()
    return {off: np.concatenate([guard[:off], pool, guard]) for off in START_OFFSETS}


def sweep_cases(frame_len):
    """Every (start offset, whole-frame count, tail) combination for one frame length; the edge table and the two
    outputs' offsets cycle through them, so each table meets each offset, tail kind and residue.  Dicts with ``offset``
    (int16 values into the buffer), ``n_pairs``, ``table``, ``mid_off`` and ``side_off``."""
    i = 0
    for off in START_OFFSETS:
        for tail in tails(frame_len):
            for whole in WHOLE_FRAMES:
                yield dict(offset=off, n_pairs=whole * frame_len + tail, table=TABLES[i % len(TABLES)],
                           mid_off=OUT_OFFSETS[i % 3], side_off=OUT_OFFSETS[(i // 3) % 3])
                i += 1
            i += 1   # 10 counts per tail: shift, so that a table does not stay with the same residues


def case_pcm(buffers, case):
    return buffers[case["offset"]][case["offset"]: case["offset"] + 2 * case["n_pairs"]]


GRID_STRIDE_FRAME_LEN = 4
GRID_STRIDE_FRAMES = SWEEP_GRID_FRAMES + 8 * 4099 + 5


def grid_stride_pcm():
    """More than one trip of the sweep's grid at 4 pairs a frame (under 9 MB), one pair short of a whole last frame:
    centred, wide and silent stretches."""
    rng = np.random.RandomState(78)
    n_pairs = GRID_STRIDE_FRAME_LEN * GRID_STRIDE_FRAMES - 1
    kind = np.repeat(rng.randint(0, 3, size=GRID_STRIDE_FRAMES // 50 + 2), 50 * GRID_STRIDE_FRAME_LEN)[:n_pairs]
    left = rng.randint(-6000, 6001, size=n_pairs)
    right = np.where(kind == 0, left + rng.randint(-40, 41, size=n_pairs), rng.randint(-6000, 6001, size=n_pairs))
    shift = np.where(kind == 2, 7, 0)
    return np.stack([left >> shift, right >> shift], axis=1).astype(np.int16).ravel()


STREAM_FRAME_LEN, STREAM_RATES = 4, (100, 400)   # 4 pairs a frame: a buffer of the streaming entries is 10 000 frames
STREAM_FRAMES = 25003                            # two whole buffers and a part of a third, a short last frame


def stream_pcm():
    """The head of grid_stride_pcm(): more than two buffers of the streaming entries, one pair short of a whole frame."""
    return grid_stride_pcm()[:2 * (STREAM_FRAME_LEN * STREAM_FRAMES - 1)]


def dual_mono(mono):
    return np.repeat(np.asarray(mono, np.int16), 2)


# ---- cases of the centre gate ------------------------------------------------------------------------------------------

GATE_LENGTHS = (0, 1, 63, 64, 65, GATE_GRID_FRAMES + 300)
GATE_OFFSETS = (0, 1, 3)


def random_levels(rng, n):
    """(mid, side): runs of centred, wide and quiet frames, and side levels above, at and below the mid ones."""
    runs = np.maximum(1, rng.geometric(0.05, size=int(n * 0.15) + 64))
    kind = np.repeat(rng.randint(0, 4, size=runs.size), runs)[:n]
    mid = np.where(kind == 3, rng.randint(0, 60, size=n), rng.randint(90, 192, size=n))
    side = np.where(kind == 0, mid - rng.randint(0, 80, size=n), np.where(kind == 1, mid + rng.randint(-3, 4, size=n), rng.randint(0, 256, size=n)))
    return mid.astype(np.uint8), np.clip(side, 0, 255).astype(np.uint8)


def gate_cases():
    """(name, mid, side, t, c): thresholds 0, 1 and 256, limits 0, 1 and 255, contrast exactly c and c - 1, side above
    mid, files without an active frame, with every active frame rejected, dual mono, a negative sum of contrasts."""
    u8 = lambda *a: np.array(a, np.uint8)
    rng = np.random.RandomState(29)
    m, s = random_levels(rng, 700)
    cases = [
        ("t 0: everything active", m, s, 0, 12),
        ("t 1", m, s, 1, 12),
        ("t 256: nothing active", m, s, 256, 12),
        ("c 0: everything with mid >= side passes", m, s, 100, 0),
        ("c 1", m, s, 100, 1),
        ("c 255", u8(255, 255, 254, 200, 0), u8(0, 1, 0, 0, 0), 100, 255),
        ("contrast exactly c and c - 1", u8(120, 120, 119, 131, 12, 11), u8(108, 109, 107, 120, 0, 0), 100, 12),
        ("side above mid", u8(120, 100, 130, 0), u8(121, 255, 200, 255), 100, 0),
        ("no active frame", u8(10, 20, 99, 0, 50), u8(0, 30, 5, 0, 90), 100, 12),
        ("all active frames rejected", u8(120, 130, 20, 100), u8(115, 130, 0, 99), 100, 12),
        ("dual mono", u8(120, 10, 130, 0, 100), u8(0, 0, 0, 0, 0), 100, 12),
        ("dual mono, nothing active", u8(1, 10, 3), u8(0, 0, 0), 100, 200),
        ("negative sum of contrasts", u8(100, 101, 150, 99), u8(255, 250, 140, 0), 100, 5),
        ("one frame: kept", u8(150), u8(100), 100, 50),
        ("one frame: rejected", u8(150), u8(101), 100, 50),
    ]
    for n in (63, 64, 65, 300):
        mm, ss = random_levels(rng, n)
        cases.append(("random %d" % n, mm, ss, int(rng.randint(90, 140)), int(rng.randint(0, 40))))
    return cases


# ---- the whole-file test input -----------------------------------------------------------------------------------------

WIDE = (1500, 2900)     # frames of the wide noise stretch
BED_BURST = (3300, 3420)    # frames of the burst of speech over a wide bed
FILE_CONTRAST = 12          # min_contrast_bins at which the file's wide stretch is gone (the shipped default is 0)


def stereo_file(frame_len=160, seed=6):
    """int16 interleaved PCM of a synthetic file, 40 s at 100 frames a second with a short last frame: an independent
    floor in both channels, centred speech bursts of 0.3 .. 3 s with pauses, one 14 s stretch of loud noise that is
    independent in the two channels (rho = 0), and one centred burst over a bed of such noise 20 dB below it."""
    rng = np.random.RandomState(seed)
    n_frames = 4000
    amp = np.zeros(n_frames)
    f = 50
    while f < n_frames - 400:
        ln = int(rng.randint(30, 300))
        if f + ln < WIDE[0] - 100 or (f >= WIDE[1] + 100 and f + ln < BED_BURST[0] - 100):
            amp[f:f + ln] = rng.uniform(2000.0, 6000.0)
        f += ln + int(rng.randint(20, 120))
    amp[BED_BURST[0]:BED_BURST[1]] = 4000.0
    centre = rng.standard_normal((n_frames, frame_len)) * amp[:, None]
    wide = np.full(n_frames, 20.0)
    wide[WIDE[0]:WIDE[1]] = 4000.0
    wide[BED_BURST[0] - 50:BED_BURST[1] + 50] = 400.0
    own = rng.standard_normal((2, n_frames, frame_len)) * wide[None, :, None]
    x = np.stack([centre + own[0], centre + own[1]], axis=2)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16).reshape(-1)[:-2 * 57]


# ---- refusals --------------------------------------------------------------------------------------------------------


def refusal_calls():
    """(export, arguments, a fragment of the message) the library must refuse with FFS_E_INVALID and a message that
    starts with the export's name, before anything touches a device: the pointers are small integers that are never
    dereferenced."""
    P, Q, R, O = 4096, 8192, 12288, 16384   # stand-ins for device pointers, 16-byte aligned
    lv = lambda **kw: tuple(dict(dict(pcm=P, n=10, fl=160, edges=Q, ne=191, mid=R, side=O, stream=None), **kw).values())
    cg = lambda **kw: tuple(dict(dict(mid=P, side=Q, n=100, thr_dev=None, thr=100, c=12, out=R, rec=O, stream=None), **kw).values())
    A, B = "ffs_vad_stereo_levels", "ffs_vad_centre_gate"
    return [
        (A, lv(n=-1), b"bad n_pairs=-1"), (A, lv(fl=0), b"frame_len=0"), (A, lv(ne=0), b"n_edges=0 outside"),
        (A, lv(ne=256), b"n_edges=256 outside"), (A, lv(pcm=None), b"null device pointer"), (A, lv(edges=None), b"null device pointer"),
        (A, lv(mid=None), b"null device pointer"), (A, lv(side=None), b"null device pointer"), (A, lv(pcm=P + 1), b"misaligned PCM"),
        (A, lv(edges=Q + 4), b"misaligned PCM (2 bytes) or edge table"),
        (B, cg(n=-1), b"n_frames=-1 is negative"), (B, cg(thr=-1), b"threshold_host=-1 outside"), (B, cg(thr=257), b"threshold_host=257 outside"),
        (B, cg(c=-1), b"min_contrast_bins=-1 outside"), (B, cg(c=256), b"min_contrast_bins=256 outside"),
        (B, cg(mid=None), b"null mid, side or record"), (B, cg(side=None), b"null mid, side or record"),
        (B, cg(rec=None), b"null mid, side or record"), (B, cg(thr_dev=Q + 2), b"misaligned threshold"),
        (B, cg(rec=O + 4), b"misaligned threshold (4 bytes) or record"), (B, cg(out=P), b"overlaps an input"),
        (B, cg(out=Q + 99), b"overlaps an input"), (B, cg(out=P - 99), b"overlaps an input"),
    ]


def accepted_empty_calls():
    """A count of 0 without pointers: FFS_OK before any launch."""
    return [("ffs_vad_stereo_levels", (None, 0, 160, None, 191, None, None, None))]


def check_refusals(lib):
    for name, args, fragment in refusal_calls():
        assert getattr(lib, name)(*args) == -1, (name, args)
        msg = lib.ffs_last_error()
        assert msg.decode().startswith(name + ": ") and fragment in msg, (name, args, msg)
    for name, args in accepted_empty_calls():
        assert getattr(lib, name)(*args) == 0, (name, args)


def python_refusals(av, tensors):
    """(callable, a fragment of the ValueError's message) for every host-side check of the Python layer that needs no
    device.  ``tensors``: dict with a CPU int16 vector ``pcm`` and CPU uint8 vectors ``mid``, ``side`` -- the checks that
    ask for CUDA tensors refuse them before any native call."""
    pcm, mid, side = tensors["pcm"], tensors["mid"], tensors["side"]
    rec = av.CentreRecord(100, 0, 12, 5, 10, 4, 2, 30)
    return [
        (lambda: av.stereo_levels(pcm, 160), "pcm: need a contiguous int16 CUDA vector"),
        (lambda: av.stereo_levels(pcm, 0), "frame_len=0"),
        (lambda: av.stereo_levels(pcm, True), "frame_len=True"),
        (lambda: av.stereo_levels(pcm, 160, edges=[3.0, 2.0]), "edges: need positive finite values"),
        (lambda: av.stereo_levels(pcm, 160, edges=np.zeros(256)), "edges: need 1 to 255"),
        (lambda: av.centre_gate(mid, side, 100, -1), "min_contrast_bins=-1"),
        (lambda: av.centre_gate(mid, side, 100, 256), "min_contrast_bins=256"),
        (lambda: av.centre_gate(mid, side, 100, 1.5), "min_contrast_bins=1.5"),
        (lambda: av.centre_gate(mid, side, 100, True), "min_contrast_bins=True"),
        (lambda: av.centre_gate(mid, side, -1), "threshold=-1"),
        (lambda: av.centre_gate(mid, side, 257), "threshold=257"),
        (lambda: av.centre_gate(mid, side, 1.0), "threshold=1.0"),
        (lambda: av.centre_gate(mid, side, side), "threshold: a device threshold"),
        (lambda: av.centre_gate(mid, side, 100), "levels: need a contiguous uint8 CUDA vector"),
        (lambda: av.detect_device_centre(pcm, 100, 16000, float("nan")), "non_speech_label"),
        (lambda: av.detect_device_centre(pcm, 100, 0, 0.0), "need at least one PCM sample per frame"),
        (lambda: av.detect_device_centre(pcm, 100, 16000, 0.0, rule="best"), "unknown rule"),
        (lambda: av.detect_device_centre(pcm, 100, 16000, 0.0, bogus=1), "unknown parameter bogus"),
        (lambda: av.detect_device_centre(pcm, 100, 16000, 0.0, min_contrast_bins=300), "min_contrast_bins=300"),
        (lambda: av.detect_device_centre(pcm, 100, 16000, 0.0, steady=1), "steady=1"),
        (lambda: av.detect_device_centre(pcm, 100, 16000, 0.0, steady=True, max_run=0), "max_run=0"),
        (lambda: av.detect_device_centre(pcm, 100, 16000, 0.0, dip_bins=-1), "dip_bins=-1"),
        (lambda: av.detect_device_centre(pcm, 100, 16000, 0.0), "pcm: need a contiguous int16 CUDA vector"),
        (lambda: av.detect_pinned_stream_centre(mid, 100, 16000, 0.0), "pcm: need a contiguous int16 CPU vector"),
        (lambda: av.detect_pinned_stream_centre(pcm[:-1], 100, 16000, 0.0), "not interleaved (L, R) pairs"),
        (lambda: av.detect_pinned_stream_centre(pcm, 100, 16000, 0.0, min_contrast_bins=-2), "min_contrast_bins=-2"),
        (lambda: av.detect_pinned_stream_centre(pcm, 100, 16000, 0.0, lo_bin=-1), "lo_bin"),
        (lambda: __import__("ffsubsync_amd.speech_transformers", fromlist=["x"]).PCMSpeechTransformer("centre:wide", 100, 16000).fit(b"\0" * 64),
         "need min_contrast_bins as an integer"),
        (lambda: __import__("ffsubsync_amd.speech_transformers", fromlist=["x"]).PCMSpeechTransformer("centre_steady:256", 100, 16000).fit(b"\0" * 64),
         "min_contrast_bins=256"),
        (lambda: av.assess_centre(rec, 1.5), "max_rejected_share=1.5"),
        (lambda: av.assess_centre(rec, True), "max_rejected_share=True"),
    ]
