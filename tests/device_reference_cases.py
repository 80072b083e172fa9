"""TEST INFRASTRUCTURE ONLY -- the forms in which one two-level reference reaches ``batch_gss.PreparedRatioSolve`` (the
one place where ``fit_gss_batch``, ``ratio_profile_batch`` / ``sweep_sync``, ``null_sync`` and ``stable_sync`` prepare
their references), the problems they are tried on and the models' answers, shared by
tests/test_device_reference_cases_host.py (which proves that every case holds what it names) and
tests/test_gpu_device_references.py.  Host data only: imports without a GPU and without the package; the builders take
``torch`` and import ``DeviceRaster`` when they are called.

A 0/1 vector ``v`` of ``n`` samples with levels (lo, hi) is passed as

  host     np.where(v, hi, lo) as float64: the control (bit-packed and copied into the solver's own upload buffer)
  packed   DeviceRaster(words, lo, hi, n): an allocation of its own, the bits at positions >= n zero
  lists    the same with ``attach_runs()``: the solver still extracts from the bits
  bytes    DeviceRaster(uint8 0/1 tensor, lo, hi): not packed, ``n`` omitted
  slice1   the packed words as a slice that starts 1 word into a larger int32 buffer ...
  slice3   ... or 3 words: the pointer is 4-byte aligned and not 16-byte aligned (residues 4 and 12 mod 16), which
           include/ffsubsync_amd.h grants a U1 vector.  Everything that is not a sample is ones, the convention of
           tests/layout_cases.py: the words in front and behind are 0xFFFFFFFF and so are the bits of the last word at
           positions >= n.  The words behind are ``GUARD_WORDS`` (256 KiB, wider than the widest look-ahead of any kernel),
           so an over-read stays inside the allocation and reads ones.

Problems are reused so that the cached model answers stay valid: the two 300 s sweep problems of
tests/test_gpu_ratio_sweep.py, the twelve sync problems of tests/surrogate_cases.py (problem i in form
FORMS[i % len(FORMS)], so one call mixes host and device references and matched and wrong files both meet every form) and
the tiny files and tracks of tests/resample_edge_cases.py.  Their reference lengths are 3000, 1777 and 5003 samples, n % 32
= 24, 17 and 11, so three tiny tracks are added here whose references have n % 32 = 0, 1 and 31 and end before their
tracks do: the overlap of nearly every lag then ends at the reference's last sample, and a bit read behind it counts.
"""
import functools

import numpy as np

import resample_edge_cases as rc
import stability_model as stm
import surrogate_cases as cases
import surrogate_model as sm
import sweep_cases
import sweep_model

FORMS = ("host", "packed", "lists", "bytes", "slice1", "slice3")
DEVICE_FORMS = FORMS[1:]
SLICE_WORDS = {"slice1": 1, "slice3": 3}
GUARD_WORDS = 65536
LEVELS = ((0.0, 1.0), (0.1, 1.0))  # the default; what a VAD raster made with non_speech_label=0.1 carries
LIST_CAP = 32768  # batch_gss.PreparedRatioSolve.LIST_CAP, restated


# ---- host images ---------------------------------------------------------------------------------------------------------
def bits_of(v):
    return np.asarray(v) != 0


def host_values(v, levels):
    return np.where(bits_of(v), float(levels[1]), float(levels[0])).astype(np.float64)


def n_words(n):
    return (int(n) + 31) // 32


def boundaries(v):
    """Run boundaries of a 0/1 vector: the entries of its boundary list."""
    return int(np.count_nonzero(np.diff(bits_of(v).astype(np.int8), prepend=0, append=0)))


def packed_image(v):
    """uint32 words of the vector, sample i = bit i & 31 of word i >> 5; the bits at positions >= n are zero."""
    v = bits_of(v)
    return np.packbits(np.concatenate([v, np.zeros(-v.size % 32, bool)]), bitorder="little").view(np.uint32).copy()


def slice_image(v, form):
    """(uint32 buffer, first word of the vector in it) of a slice form: every bit that is not a sample is 1."""
    v = bits_of(v)
    start = SLICE_WORDS[form]
    words = np.packbits(np.concatenate([v, np.ones(-v.size % 32, bool)]), bitorder="little").view(np.uint32)
    buf = np.full(start + words.size + GUARD_WORDS, 0xFFFFFFFF, np.uint32)
    buf[start:start + words.size] = words
    return buf, start


def unpack(words, n):
    """The first n samples of uint32 words: a read with the length mask."""
    return np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8), bitorder="little")[:int(n)].astype(bool)


def build(form, v, levels, torch):
    """What is passed as the reference: the vector in form ``form`` with levels ``levels``."""
    v = bits_of(v)
    lo, hi = float(levels[0]), float(levels[1])
    if form == "host":
        return host_values(v, levels)
    from ffsubsync_amd.subtitle_raster import DeviceRaster

    if form == "bytes":
        return DeviceRaster(torch.from_numpy(v.astype(np.uint8)).cuda(), lo, hi)
    if form in SLICE_WORDS:
        buf, start = slice_image(v, form)
        dev = torch.from_numpy(buf.view(np.int32)).cuda()
        assert dev.data_ptr() % 64 == 0  # (so the slice's residue mod 16 is 4 * start)
        return DeviceRaster(dev[start:start + n_words(v.size)], lo, hi, v.size)
    assert form in ("packed", "lists"), form
    raster = DeviceRaster(torch.from_numpy(packed_image(v).view(np.int32)).cuda(), lo, hi, v.size)
    return raster.attach_runs() if form == "lists" else raster


# ---- the ratio profile and the sweep ---------------------------------------------------------------------------------------
W = sweep_cases.W
SWEEP_SEEDS = (5, 2)  # sweep_cases.problem("free", seed, 300.0): true ratios 1.0326 and 0.9498
PROFILE_RANGE = (1.02, 1.05)  # 5 to 8 grid points a file (tests/test_gpu_ratio_sweep.py)
SWEEP_RANGE = {5: (1.02, 1.05), 2: (0.935, 0.965)}  # around each true ratio: a model sweep of tens of oracle solves
SWEEP_LEVELS = {5: LEVELS[0], 2: LEVELS[1]}
SWEEP_FORMS = {5: ("host", "packed", "slice3"), 2: ("bytes", "host", "slice1", "lists")}


def sweep_problem(seed):
    return sweep_cases.problem("free", seed, 300.0)


@functools.lru_cache(maxsize=None)
def exact_profile(seed, levels, lo=PROFILE_RANGE[0], hi=PROFILE_RANGE[1]):
    """(grid, [(offset, score)]) of the sweep problem with reference levels ``levels``: ``exact_reference.candidate`` at
    every point of the grid, the candidate's amplitude min(1 / r, 1)."""
    import exact_reference as er
    from oracle import raster_oracle as ro

    p = sweep_problem(seed)
    grid, _ = sweep_model.grid(sweep_model.duration_samples(p.track), lo, hi, 40.0)
    spec = er.RefSpectrum(bits_of(p.reference))
    out = []
    for r in grid:
        sub = ro.rasterize(p.track[0], p.track[1], p.track[2], float(r), 100, 0) != 0
        rec = er.candidate(spec, sub, levels, (0.0, min(1.0 / float(r), 1.0)), W)
        assert rec["flags"] == 0
        out.append((rec["offset"], rec["score"]))
    return grid, out


@functools.lru_cache(maxsize=None)
def model_sweep(seed):
    """``sweep_model.sweep`` of the sweep problem on its host values (levels SWEEP_LEVELS[seed]) over SWEEP_RANGE[seed]."""
    p = sweep_problem(seed)
    lo, hi = SWEEP_RANGE[seed]
    return sweep_model.sweep(host_values(p.reference, SWEEP_LEVELS[seed]), p.track, W, lo=lo, hi=hi)


# ---- the golden-section search ---------------------------------------------------------------------------------------------
GSS_FORMS = (("slice3", LEVELS[0]), ("bytes", LEVELS[1]), ("lists", LEVELS[1]))  # (form, levels) of file i


@functools.lru_cache(maxsize=None)
def gss_files():
    """[(reference 0/1 vector, track)]: the three files of tests/test_gpu_raster.py's golden-section test (six minutes,
    120 cues, true ratios 1.0427, 0.9590 and 1.0, the reference shifted by 250, -130 and 77 samples)."""
    from oracle import raster_oracle as ro

    out = []
    for seed, true_ratio, shift in [(41, 1.0427, 250), (42, 0.9590, -130), (43, 1.0, 77)]:
        s, e, m = ro.synth_subtitles(seed, n=120, minutes=6.0)
        truth = (ro.rasterize(s, e, m, true_ratio, 100, 0) > 0).astype(float)
        ref = np.concatenate([np.zeros(max(shift, 0)), truth[max(-shift, 0):], np.zeros(500)])
        out.append((bits_of(ref), (s, e, m)))
    return out


# ---- the twelve sync problems ------------------------------------------------------------------------------------------------
def sync_form(i):
    return FORMS[i % len(FORMS)]


# ---- tiny tracks -------------------------------------------------------------------------------------------------------------
RESIDUE_LENGTHS = (2464, 2465, 2495)  # n % 32 = 0, 1, 31; shorter than their tracks
TRACK_FORMS = ("slice1", "bytes", "slice3", "bytes", "slice1", "slice3", "bytes", "slice1")  # of tiny track j
TRACK_LEVELS = tuple(LEVELS[j % 2] for j in range(len(TRACK_FORMS)))


@functools.lru_cache(maxsize=None)
def track_problems():
    """[(reference 0/1 vector, track)]: the five tiny tracks of tests/resample_edge_cases.py, then three of nine cues
    whose references have RESIDUE_LENGTHS samples."""
    out = [(bits_of(ref), track) for ref, track in rc.track_problems()]
    for i, n in enumerate(RESIDUE_LENGTHS):
        rng = np.random.RandomState(1300 + i)
        ref = rc.frames_vector(rng, n)
        start = np.sort(rng.choice(np.arange(10, 250), 9, replace=False)).astype(np.int64) * 100000
        end = start + rng.randint(4, 20, 9).astype(np.int64) * 100000 + 30000
        out.append((bits_of(ref), (start, end, np.zeros(9, np.uint8))))
    assert len(out) == len(TRACK_FORMS)
    return out


@functools.lru_cache(maxsize=None)
def track_null_model(j):
    ref, track = track_problems()[j]
    return sm.null_sync(host_values(ref, TRACK_LEVELS[j]), track, rc.TRACK_W, None, rc.TRACK_K, 1, rc.TRACK_SEED, j, rc.TRACK_MIN_Z,
                        levels=TRACK_LEVELS[j])


@functools.lru_cache(maxsize=None)
def track_stable_model(j):
    ref, track = track_problems()[j]
    return stm.stable_sync(host_values(ref, TRACK_LEVELS[j]), track, rc.TRACK_W, None, rc.TRACK_K, 1, rc.TRACK_SEED, j, rc.TRACK_TOL,
                           rc.TRACK_MIN_SHARE, levels=TRACK_LEVELS[j])


# ---- tiny files (device-resident lists on both sides) ------------------------------------------------------------------------
TINY_FORMS = ("slice1", "bytes", "slice3", "slice3", "bytes", "slice1", "bytes")  # of the reference of tiny file i
TINY_BLOCK, TINY_K = 2, 5


# ---- a dense and a silent device reference ---------------------------------------------------------------------------------
DENSE_HEAD = 40000  # alternating samples: 40 000 boundaries
SMALL_SECONDS = 4  # the lag window of the dense, silent and PCM problems: 400 samples
SMALL_W = 400
DENSE_RANGE = (0.93, 1.07)
DENSE_TOLERANCE = 10.0
DENSE_FORMS = tuple((form, LEVELS[k % 2]) for k, form in enumerate(DEVICE_FORMS))
SILENT_LEVELS = (0.0, 1.0)


@functools.lru_cache(maxsize=None)
def dense_reference():
    """40 000 alternating samples, then 3 007 samples of random frames: more boundaries than a list holds, n % 32 = 31."""
    tail = rc.frames_vector(np.random.RandomState(77), 3007)
    return np.concatenate([np.arange(DENSE_HEAD) % 2, tail]).astype(bool)


def small_track():
    """The nine-cue tiny track (about 26 s) that goes with the dense and the silent reference."""
    return rc.track_problems()[3][1]


def silent_reference():
    return np.zeros(3000, bool)


@functools.lru_cache(maxsize=None)
def exact_records(name, levels, ratios):
    """[(offset, score, flags)] of ``exact_reference.candidate`` of the "dense" or "silent" reference against the small
    track at every ratio of the tuple ``ratios``."""
    import exact_reference as er
    from oracle import raster_oracle as ro

    ref = dense_reference() if name == "dense" else silent_reference()
    spec, tr, out = er.RefSpectrum(ref), small_track(), []
    for r in ratios:
        sub = ro.rasterize(tr[0], tr[1], tr[2], float(r), 100, 0) != 0
        rec = er.candidate(spec, sub, levels, (0.0, min(1.0 / float(r), 1.0)), SMALL_W)
        out.append((rec["offset"], rec["score"], rec["flags"]))
    return out


def small_grid(lo, hi, tolerance):
    tr = small_track()
    return sweep_model.grid(sweep_model.duration_samples(tr), lo, hi, tolerance)[0]


# ---- PCM to answer -----------------------------------------------------------------------------------------------------------
PCM_LABEL = 0.1
PCM_LEVELS = (PCM_LABEL, 1.0)
PCM_OFFSET = 150  # samples: the reference is the track, 1.5 s late ...
PCM_RATIO_INDEX = 5  # ... and the track runs at 1 / sweep_model.SEVEN[5] of the reference's speed
PCM_K = 16
PCM_SEED = 11
PCM_SWEEP = dict(tolerance_samples=10.0, top_k=1)  # (lo, hi) = PCM ratio -+ 0.03: 5 coarse points, 33 + 7 fine ones
PCM_GAINS = (0, -12, -30)


def pcm_ratio():
    return float(sweep_model.SEVEN[PCM_RATIO_INDEX])


def pcm_sweep_range():
    return pcm_ratio() - 0.03, pcm_ratio() + 0.03


@functools.lru_cache(maxsize=None)
def pcm_speech():
    """The adaptive model's speech flags of the loudest gain file (the other gains give the same, asserted on the host)."""
    import adaptive_vad_model as am

    fl, files = am.gain_files()
    return am.detect(files[0], fl, **pcm_pick_args())[0]


def pcm_pick_args():
    """The shipped defaults of ``adaptive_vad.detect_device_adaptive`` as ``adaptive_vad_model.pick`` takes them (restated:
    this module does not import the package; tests/test_device_reference_cases_host.py compares them)."""
    return dict(rule=0, lo_bin=0, t_min=1, floor_ppm=200000, margin_bins=10)


@functools.lru_cache(maxsize=None)
def pcm_track():
    """One cue per run of ``pcm_speech()``: reference sample a is track time (a - PCM_OFFSET) / (100 ratio); the runs that
    would start before time 0 are left out."""
    v = pcm_speech()
    edges = np.flatnonzero(np.diff(v.astype(np.int8), prepend=0, append=0))
    a, b = edges[0::2], edges[1::2]
    keep = a >= PCM_OFFSET
    scale = 1e6 / (100.0 * pcm_ratio())
    start = np.rint((a[keep] - PCM_OFFSET) * scale).astype(np.int64)
    end = np.rint((b[keep] - PCM_OFFSET) * scale).astype(np.int64)
    return start, end, np.zeros(start.size, np.uint8)


@functools.lru_cache(maxsize=None)
def pcm_models(silent=False):
    """The models' answers on np.where(speech, 1.0, 0.1) (or, with ``silent``, on the quiet file under the fixed rule: no
    speech at all): dict(seven=[(offset, score)] of the exact seven-ratio solve, best, null, stable, sweep)."""
    import exact_reference as er
    from oracle import raster_oracle as ro

    v = np.zeros(pcm_speech().size, bool) if silent else pcm_speech()
    values, tr = host_values(v, PCM_LEVELS), pcm_track()
    spec, seven = er.RefSpectrum(v), []
    for r in sweep_model.SEVEN:
        sub = ro.rasterize(tr[0], tr[1], tr[2], float(r), 100, 0) != 0
        rec = er.candidate(spec, sub, PCM_LEVELS, (0.0, min(1.0 / r, 1.0)), SMALL_W)
        seven.append((rec["offset"], rec["score"]))
    best = int(np.argmax([s for _, s in seven]))  # (the first maximal candidate)
    lo, hi = pcm_sweep_range()
    return dict(seven=seven, best=best,
                null=sm.null_sync(values, tr, SMALL_W, None, PCM_K, 1, PCM_SEED, 0, rc.TRACK_MIN_Z, levels=PCM_LEVELS),
                stable=stm.stable_sync(values, tr, SMALL_W, None, PCM_K, 1, PCM_SEED, 0, rc.TRACK_TOL, rc.TRACK_MIN_SHARE, levels=PCM_LEVELS),
                sweep=sweep_model.sweep(values, tr, SMALL_W, lo=lo, hi=hi, **PCM_SWEEP))
