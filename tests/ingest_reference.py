"""TEST INFRASTRUCTURE ONLY -- plain exact references for the ingest kernels (everything between decoded PCM and the
vector the aligner reads), and the input builders that tests/test_ingest_reference_host.py (CPU) and
tests/test_gpu_ingest.py (GPU) share, so that the conditions asserted on the CPU are conditions of the very inputs the
GPU module runs.

Independent of oracle/vad_oracle.py where that is possible: the frame rule here is the one the C header states,
``sum(x^2) >= 10^(thr/10) * n``, in exact integers for thresholds that are multiples of 10 dB; the oracle's is
``10*log10(sum/n) >= thr``.  The host test holds the two against each other.

VAD parity with auditok itself stays unpinned (the package is not available to check against): what is pinned here is
kernel against restatement and exact arithmetic.
"""
import math

import numpy as np

from oracle import vad_oracle as vo

# ---- frame energy ------------------------------------------------------------------------------------------------


def frame_sums(pcm, frame_len):
    """(sum of squares as int64, sample count as int64) per frame, short tail frame included.
    Exact: at most 4800 * 2^30 < 2^43 for every frame length used here."""
    x = np.asarray(pcm).astype(np.int64)
    fl = int(frame_len)
    n_full = x.size // fl
    sums = (x[: n_full * fl].reshape(n_full, fl) ** 2).sum(axis=1)
    counts = np.full(n_full, fl, dtype=np.int64)
    if x.size > n_full * fl:
        tail = x[n_full * fl:]
        sums = np.append(sums, (tail ** 2).sum())
        counts = np.append(counts, tail.size)
    return sums.astype(np.int64), counts


def decade(threshold_db):
    """k when the threshold is 10 k dB with an integer k >= 0 (so 10^(thr/10) is the integer 10^k), else None."""
    k = threshold_db / 10.0
    return int(k) if k == int(k) and k >= 0 else None


def energy_labels(pcm, frame_len, threshold_db):
    """(speech flag per frame, smallest relative distance of a frame from the threshold) by the rule of the header:
    speech <=> sum >= 10^(thr/10) * n.  For a threshold of 10 k dB the comparison is in exact integers
    (sum >= 10^k * n: below 2^63 for k <= 9 and n <= 4800), so frames exactly at the threshold are decided exactly and
    the distance is reported as inf (nothing is ambiguous).  Otherwise it is the fp64 comparison, and the second
    value is min |sum - T n| / (T n) so that a test can assert that rounding cannot move any frame."""
    sums, counts = frame_sums(pcm, frame_len)
    k = decade(threshold_db)
    if k is not None:
        assert k <= 9 and int(frame_len) <= 4800
        return sums >= (10 ** k) * counts, math.inf
    t = 10.0 ** (threshold_db / 10.0) * counts.astype(np.float64)
    s = sums.astype(np.float64)
    dist = float(np.min(np.abs(s - t) / t)) if s.size else math.inf
    return s >= t, dist


def boundary_frame(frame_len, k, delta):
    """An int16 frame whose sum of squares is exactly 10^k * frame_len + delta (greedy decomposition into squares of
    values up to 32768, zero-padded), or None when that needs more than frame_len samples (or the sum is negative)."""
    target = 10 ** int(k) * int(frame_len) + int(delta)
    if target < 0:
        return None
    vals = []
    rem = target
    while rem > 0:
        if len(vals) == frame_len:
            return None
        v = min(math.isqrt(rem), 32768)
        vals.append(v)
        rem -= v * v
    out = np.zeros(int(frame_len), dtype=np.int64)
    # +32768 is not an int16: 32768 always goes in negated, the other values on odd positions
    for i, v in enumerate(vals):
        out[i] = -v if (v == 32768 or i % 2) else v
    frame = out.astype(np.int16)
    assert int((frame.astype(np.int64) ** 2).sum()) == target
    return frame


VECTOR, ELEMENT_TAIL, ELEMENT_UNALIGNED, ELEMENT_ODD, ELEMENT_ROUNDS = (
    "vector", "element_after_vector", "element_unaligned", "element_odd", "element_rounds")
BRANCH_CLASSES = (VECTOR, ELEMENT_TAIL, ELEMENT_UNALIGNED, ELEMENT_ODD, ELEMENT_ROUNDS)


def vector_path(frame_len, byte_offset, first_frame, n_samples):
    """Which branch of k_vad_energy serves the group of four frames that starts at ``first_frame`` (a multiple of 4),
    restated from the dispatch rule in ffs_kernels.h: the 16-byte vector path needs frame_len % 8 == 0,
    frame_len <= 512 (one vector per lane), a 16-byte aligned base and four whole frames left; everything else goes
    through the element loop, in ceil(n / 512) rounds per frame.  Used to COUNT coverage only, never for a label."""
    fl = int(frame_len)
    if fl > 512:
        return ELEMENT_ROUNDS
    if fl % 8:
        return ELEMENT_ODD
    if byte_offset % 16:
        return ELEMENT_UNALIGNED
    return VECTOR if (first_frame + 4) * fl <= n_samples else ELEMENT_TAIL


# ---- inputs of the frame-energy sweep --------------------------------------------------------------------------------

FRAME_LENS = (1, 2, 7, 8, 16, 80, 160, 221, 320, 441, 480, 504, 512, 520, 960, 1920, 4800)
START_OFFSETS = (0, 1, 3, 8)           # samples into a 16-byte aligned allocation
DECADE_THRESHOLDS = (0.0, 30.0, 50.0, 90.0)
OTHER_THRESHOLDS = (47.3, 61.8)
THRESHOLDS = DECADE_THRESHOLDS + OTHER_THRESHOLDS
ENERGY_LABELS = (0.0, -1.0, 0.1, 0.7)
WHOLE_FRAMES = tuple(range(40, 48))    # every residue mod 8; 41-43 and 45-47 leave 1-3 whole frames behind a group of 4
POOL_FRAMES = 49                       # frames in a pool: the longest slice plus one frame to cut a tail from
GUARD_SAMPLES = 64                     # loud samples behind every slice: reading past n_samples changes a label


def tails(frame_len):
    """Tail lengths: none, one sample, frame_len - 1 samples (where those are distinct and shorter than a frame)."""
    return tuple(sorted({0, 1, frame_len - 1} & set(range(frame_len))))


def _extreme_frames(frame_len):
    alt = np.where(np.arange(frame_len) % 2 == 0, -32768, 32767)
    return [np.full(frame_len, -32768), np.full(frame_len, 32767), alt]


def energy_pool(frame_len, threshold_db):
    """POOL_FRAMES frames (int16 [POOL_FRAMES, frame_len]) for one (frame length, threshold): for decade thresholds
    loud and quiet noise around 10^k with boundary_frame(.., delta in {-1, 0, 1}) spliced in, for the others
    vo.synth_pcm; the three full-scale frames in both."""
    seed = (1000 * int(frame_len) + int(round(threshold_db * 10))) % (2 ** 31)
    rng = np.random.RandomState(seed)
    k = decade(threshold_db)
    if k is None:
        pcm, _ = vo.synth_pcm(POOL_FRAMES * frame_len, seed=seed, frame=frame_len)
        frames = pcm.reshape(POOL_FRAMES, frame_len).astype(np.int64)
        # synth_pcm's stretches are long against 49 frames: make every third frame loud so both labels occur
        loud = np.clip(np.rint(rng.randn(POOL_FRAMES, frame_len) * 3000.0), -32768, 32767).astype(np.int64)
        frames[::3] = loud[::3]
        special = _extreme_frames(frame_len)
    else:
        amp = math.sqrt(10.0 ** k)
        loud = np.clip(np.rint(rng.randn(POOL_FRAMES, frame_len) * amp * 4.0), -32768, 32767)
        quiet = np.clip(np.rint(rng.randn(POOL_FRAMES, frame_len) * amp * 0.25), -32768, 32767)
        frames = np.where((rng.rand(POOL_FRAMES) < 0.5)[:, None], loud, quiet).astype(np.int64)
        special = [boundary_frame(frame_len, k, d) for d in (-1, 0, 1)] + _extreme_frames(frame_len)
        special = [f for f in special if f is not None]
    # spread the special frames so that the slots of a group of four and the frames behind the last group meet them
    slots = rng.permutation(POOL_FRAMES)
    for j, slot in enumerate(slots[: 4 * len(special)]):
        frames[slot] = special[j % len(special)]
    return frames.astype(np.int16)


def energy_cases(frame_len):
    """The sweep's cases for one frame length: dicts with ``threshold``, ``offset`` (samples into the allocation),
    ``n_samples``, ``label`` and ``buffer`` (int16: ``offset`` loud samples, the pool, a loud guard; one object per
    (threshold, offset)).  The slice under test is buffer[offset : offset + n_samples]; what lies behind it is the
    rest of the pool and the guard, so a read past n_samples shows.  Every (offset, whole-frame count, tail)
    combination; thresholds and labels cycle through them (every pair within 24 consecutive cases), so each threshold
    meets each offset, each tail kind and each residue of the frame count."""
    guard = np.where(np.arange(GUARD_SAMPLES) % 2 == 0, 32767, -32768).astype(np.int16)
    pools = [energy_pool(frame_len, thr).ravel() for thr in THRESHOLDS]
    i = 0
    for off in START_OFFSETS:
        bufs = [np.concatenate([guard[:off], pool, guard]) for pool in pools]
        for tail in tails(frame_len):
            for whole in WHOLE_FRAMES:
                t = i % len(THRESHOLDS)
                yield {"threshold": THRESHOLDS[t], "offset": off, "n_samples": whole * frame_len + tail,
                       "label": ENERGY_LABELS[(i // len(THRESHOLDS)) % len(ENERGY_LABELS)], "buffer": bufs[t]}
                i += 1
            i += 1  # 8 counts per tail: shift, so that a threshold does not stay with the same residues


def case_pcm(case):
    return case["buffer"][case["offset"]: case["offset"] + case["n_samples"]]


GRID_STRIDE_FRAME_LEN = 8
GRID_STRIDE_FRAMES = 524288 + 8 * 4099 + 5   # k_vad_energy's grid covers 16384 blocks x 4 waves x 8 frames per trip


def fast_pcm(n_samples, frame_len, seed):
    """Cheap stand-in for vo.synth_pcm at tens of millions of samples: uniform noise of +-6000 in 'speech' stretches
    (about 71 dB) and the same noise shifted down by 7 bits elsewhere (about 29 dB)."""
    rng = np.random.RandomState(seed)
    n_frames = (n_samples + frame_len - 1) // frame_len
    seg = np.maximum(1, rng.geometric(1.0 / 120.0, size=n_frames // 40 + 8))
    state = np.repeat(rng.rand(seg.size) < 0.4, seg)[:n_frames]
    if state.size < n_frames:
        state = np.concatenate([state, np.zeros(n_frames - state.size, bool)])
    x = rng.randint(-6000, 6001, size=n_samples).astype(np.int16)
    shift = np.repeat(np.where(state, 0, 7).astype(np.int16), frame_len)[:n_samples]
    return x >> shift


def grid_stride_pcm():
    """More than 524 288 frames of 8 samples (under 5 M samples), one sample short of a whole last frame."""
    return fast_pcm(GRID_STRIDE_FRAME_LEN * GRID_STRIDE_FRAMES - 1, GRID_STRIDE_FRAME_LEN, 77)


def expected_f32(speech, label):
    return np.where(speech, np.float32(1.0), np.float32(label)).astype(np.float32)


def expected_bits(speech):
    return np.packbits(np.asarray(speech, bool), bitorder="little")


# ---- streaming entry ---------------------------------------------------------------------------------------------

STREAM_RATES = (48000, 44100, 16000)
STREAM_BUFFERS = 5       # whole 100 s buffers in front of the short last one: each staging buffer is used three times
STREAM_EXTRA = 12345     # samples of the last buffer: not a multiple of 480, 441 or 160


def stream_samples(frame_rate, buffers=STREAM_BUFFERS, extra=STREAM_EXTRA):
    fl = vo.frame_len(100, frame_rate)
    assert extra % fl
    return buffers * fl * 10000 + extra


def stream_source():
    """One PCM array that every streaming case cuts its file from (stretches in 10 ms frames of 48 kHz)."""
    return fast_pcm(stream_samples(48000), 480, 48)


# ---- tokenizer ---------------------------------------------------------------------------------------------------

TOKEN_CASES = [(20, 500, 25), (3, 10, 2), (5, 5, 1), (1, 7, 0), (4, 40, 30), (2, 9, 9), (1, 1, 0), (0, 3, -1),
               (2, 70, 100), (9, 4, 2)]     # (min_length, max_length, max_continuous_silence) of the existing tests
TOKEN_LENGTHS = (30011, 10000, 257, 28672, 3000, 65, 20480, 256, 64, 10000)   # one per case; the existing tests' lengths
TOKEN_CHUNKS = (10000, 997, 30011)
TOK_SCAN_MAX = 28672                        # longest chunk the workgroup kernel takes (ffs_kernels.h)
DYADIC_LABELS = (0.0, 0.25, -1.0)
NON_DYADIC_LABELS = (0.1, 0.3, -0.3, 1.0 / 3.0, 1e-3, 0.7)
TOKEN_ULP = 2.0 ** -23


def validity_pattern(rng, n):
    """Random validity vector of n frames in runs (the generator of the existing tokenizer tests)."""
    p_on = rng.choice([0.02, 0.2, 0.6, 0.95])
    runs = rng.geometric(1.0 / rng.choice([1, 3, 15, 80, 700]), size=n + 4)
    return np.repeat(rng.rand(runs.size) < p_on, runs)[:n]


def token_inputs(seed=21):
    """(valid, (min, max, silence)) per parameter case."""
    rng = np.random.RandomState(seed)
    for n, case in zip(TOKEN_LENGTHS, TOKEN_CASES):
        yield validity_pattern(rng, n), case


def serial_kernel_serves(n, chunk, case):
    """The dispatch rule of ffs_vad_tokenize, restated to COUNT coverage: one thread per chunk unless the longest
    chunk fits the workgroup kernel and max_length >= min_length >= 0."""
    mn, mx, _ = case
    return not (min(n, chunk) <= TOK_SCAN_MAX and mx >= mn and mn >= 0)


def chunk_tokens(valid, case):
    return vo._Tokenizer(*case).tokenize(valid)


def token_markers(valid, min_length, max_length, max_silence, tokens=None):
    """(cp, cm): the number of +1 markers and of end markers at or in front of every frame of ONE chunk, from
    vo._Tokenizer's token list with the reference's in-order assignment (marker[start] = 1, marker[end + 1] = label - 1:
    a +1 overwrites an end marker that fell on the same frame)."""
    n = len(valid)
    if tokens is None:
        tokens = chunk_tokens(valid, (min_length, max_length, max_silence))
    code = np.zeros(n + 1, dtype=np.int8)
    for start, end in tokens:
        code[start] = 1
        code[end + 1] = -1
    return np.cumsum(code[:n] == 1), np.cumsum(code[:n] == -1)


def rasterise_tokens(n, tokens, label):
    """The reference's rasterisation of one chunk's tokens in float64 (speech_transformers.py:143-150)."""
    marks = np.zeros(n + 1)
    for start, end in tokens:
        marks[start] = 1.0
        marks[end + 1] = label - 1.0
    return np.clip(np.cumsum(marks)[:-1], 0.0, 1.0)


def tokenize_f64(valid, labels, chunk, case):
    """({label: float64 restatement}, cp, cm) over the chunk loop; the token lists do not depend on the label."""
    want, cps, cms = {label: [] for label in labels}, [], []
    for o in range(0, len(valid), chunk):
        c = valid[o:o + chunk]
        tokens = chunk_tokens(c, case)
        for label in labels:
            want[label].append(rasterise_tokens(len(c), tokens, label))
        cp, cm = token_markers(c, *case, tokens=tokens)
        cps.append(cp)
        cms.append(cm)
    return {label: np.concatenate(w) for label, w in want.items()}, np.concatenate(cps), np.concatenate(cms)


def token_model_f32_marker(cp, cm, label):
    """float32(clip(cp + cm * float64(float32(l) - float32(1)), 0, 1)): the end marker formed in float32."""
    m = np.float64(np.float32(label) - np.float32(1.0))
    return np.clip(cp + cm * m, 0.0, 1.0).astype(np.float32)


def token_model(cp, cm, label):
    """What both tokenizer kernels compute: the float32 label, the end marker float64(float32(l)) - 1 (exact in
    float64), the running sum cp + cm * marker in float64, clipped, rounded to float32 once."""
    m = np.float64(np.float32(label)) - 1.0
    return np.clip(cp + cm * m, 0.0, 1.0).astype(np.float32)


def token_bound(cm):
    """Derived, not measured.  For |label| <= 1 each end marker carries at most 2^-25 from rounding the label to
    float32 and 2^-24 from a float32 subtraction (its result lies in (-2, 0]); the float32 output adds 2^-25; the
    float64 restatement's own rounding is far below these.  (cm + 1) * 2^-23 covers the sum with less than a factor
    of two to spare."""
    return (np.asarray(cm, dtype=np.float64) + 1.0) * TOKEN_ULP


AUDITOK30 = (30, 48000)   # sample_rate, frame_rate: frame_len 1600, tokenizer (0.2 * 30, 150, 0.25 * 30) = (6.0, 150, 7.5)


def auditok30_pcm():
    """(pcm, validity) for the auditok-like detector at sample_rate 30: speech runs separated by silences of 7, 8 and
    9 frames among random ones -- a silence of exactly 8 frames is tolerated by a limit of 7.5 and by its ceiling, not
    by its floor.  The last frame is short."""
    rng = np.random.RandomState(30)
    runs = []
    for i in range(40):
        runs.append((True, int(rng.randint(1, 40))))
        runs.append((False, int((7, 8, 9, rng.randint(1, 30))[i % 4])))
    valid = np.concatenate([np.full(length, v) for v, length in runs])
    x = rng.randn(valid.size, 1600) * np.where(valid, 3000.0, 30.0)[:, None]
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16).ravel()[:-123], valid


# ---- host loops ----------------------------------------------------------------------------------------------------


def fit_boundaries(speech_frames):
    """speech_transformers.py:310-317: (first, last) index with value > 0.5 in the array's own precision, or
    (None, None)."""
    nz = np.nonzero(np.asarray(speech_frames) > 0.5)[0]
    return (int(nz[0]), int(nz[-1])) if nz.size else (None, None)


def pack_bits(x, threshold=None):
    """uint8 little-endian bit image padded to whole 32-bit words: bit = (byte != 0) for uint8 input,
    (float64(x) > threshold) for float input."""
    x = np.asarray(x)
    flags = (x != 0) if x.dtype == np.uint8 else (x.astype(np.float64) > threshold)
    b = np.packbits(flags, bitorder="little")
    return np.concatenate([b, np.zeros(-b.size % 4, np.uint8)])


def scatter(segments, begins, out_len):
    """The loop of MultiSegmentVideoSpeechTransformer.fit (speech_transformers.py:871, 886-890), windows applied in
    the order given; ``begins`` are frame indices."""
    sparse = np.zeros(int(out_len), dtype=float)
    for begin, seg in zip(begins, segments):
        begin = int(begin)
        end = min(begin + len(seg), len(sparse))
        if end > begin:
            sparse[begin:end] = seg[: end - begin]
    return sparse


BOUNDS_LENGTHS = (1, 63, 64, 65, 255, 256, 257, 131071, 131072, 131073, 2 ** 20 + 5)
F32_ABOVE_HALF = np.nextafter(np.float32(0.5), np.float32(1.0))
F32_BELOW_HALF = np.nextafter(np.float32(0.5), np.float32(0.0))


def bounds_patterns(n):
    """(name, float32 vector) cases of length n: no speech, all speech, single speech frames at the edges, in the
    middle and at the first index of the kernel's second grid-stride trip (131 072), values at and next to 0.5, NaN
    and infinities."""
    above, below = F32_ABOVE_HALF, F32_BELOW_HALF
    yield "none", np.zeros(n, np.float32)
    yield "all", np.ones(n, np.float32)
    yield "at_half", np.full(n, 0.5, np.float32)
    yield "below_half", np.full(n, below, np.float32)
    for name, idx in (("first", 0), ("last", n - 1), ("middle", n // 2), ("second_trip", 131072)):
        if idx < n:
            x = np.full(n, 0.5, np.float32)
            x[idx] = above
            yield name, x
    x = np.full(n, np.nan, np.float32)
    yield "nan", x.copy()
    x[n // 3] = above
    x[(2 * n) // 3] = np.inf
    yield "nan_and_speech", x
    x = np.full(n, -np.inf, np.float32)
    x[n - 1] = np.inf
    x[0] = np.nan
    yield "inf", x
    rng = np.random.RandomState(n % 9973)
    values = np.array([0.0, 0.5, below, above, 1.0, -1.0, np.nan, np.inf, -np.inf], np.float32)
    yield "mixed", values[rng.choice(values.size, n, p=[0.6, 0.1, 0.1, 0.02, 0.02, 0.06, 0.06, 0.02, 0.02])]
