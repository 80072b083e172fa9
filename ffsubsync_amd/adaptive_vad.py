"""Adaptive energy VAD: a per-file threshold from frame-level counts.

The fixed rule of the energy detector (a frame is speech iff its mean square reaches 50 dB on the raw s16 scale) depends
on the file's gain: 30 dB down it finds nothing.  Here the whole file decides.  Pass 1 streams the PCM once and reduces
every frame to a LEVEL, the number of edges of a half-dB table its mean square reaches; three small kernels count the
levels, pick one threshold bin from the counts and label the frames with it.

    frame_levels                   ``ffs_vad_levels``: uint8 level per frame, chunk by chunk if need be
    level_hist                     ``ffs_vad_level_hist``: the level counts
    pick_threshold                 ``ffs_vad_pick_threshold``: one record per histogram (Otsu, or noise floor + margin)
    level_labels                   ``ffs_vad_level_labels``: float32 labels or the packed raster the aligner reads
    detect_device_adaptive         the four launches queued on the current stream for PCM resident in HBM
    detect_pinned_stream_adaptive  the same behind ``detect_pinned_stream``'s double-buffered copy loop
    assess                         reasons not to trust a record
    steady_gate                    ``ffs_vad_steady_gate``: the labels without the stretches of uninterrupted activity
                                   longer than ``max_run`` frames -- music, hum, hiss
    detect_device_gated            detect_device_adaptive with the gate behind the pick
    detect_pinned_stream_gated     detect_pinned_stream_adaptive with the gate behind the pick
    assess_gate                    what a gate record says about the file
    stereo_levels                  ``ffs_vad_stereo_levels``: mid (L + R) and side (L - R) level per frame of interleaved
                                   stereo PCM
    centre_gate                    ``ffs_vad_centre_gate``: the mid levels with every frame zeroed whose mid level does not
                                   stand ``min_contrast_bins`` above its side level -- wide music, ambience, audiences
    detect_device_centre           stereo sweep, histogram and pick of the mid levels, centre gate, labels (or, with
                                   ``steady``, the steady-run gate on the centre gate's output)
    detect_pinned_stream_centre    the same behind ``detect_pinned_stream``'s double-buffered copy loop
    assess_centre                  what a centre record says about the file

``PCMSpeechTransformer(vad="adaptive")`` runs it behind the pipelined chunk loop, ``vad="gated"`` with the gate,
``vad="centre"`` and ``vad="centre_steady"`` the centre-channel path on two interleaved channels.  Nothing
existing changes behaviour: the fixed rule stays the default everywhere, and every fallback of the pick IS the fixed
rule (bin 100 of the default table is 50 dB).

What it says and what it does not.  This is the project's own rule with no upstream counterpart (the reference's
adaptive detector is WebRTC's): parity is against the in-repo model ``tests/adaptive_vad_model.py`` only.  It is still
an ENERGY rule: loud music is labelled speech, by this rule as by the fixed one.  The defaults below come from
SYNTHETIC data only (profiles/adaptive_vad_calibration.json); nobody has measured real files.
"""
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Union

import numpy as np

from . import _native

# By the rules of profiles/adaptive_vad_calibrate.py on the CPU model (profiles/adaptive_vad_calibration.json; synthetic PCM,
# 10 min and 1 h, gains 0 .. -40 dB, 0 / 12 / 40 % digital silence).  Worst error over all mixed files under Otsu: 0.196 at
# lo_bin 0 (a file with 40 % digital silence at gain 0: the split falls between silence and everything else) against
# 0.252 at lo_bin 1, 10 and 20 (at -40 dB the noise floor rounds to zeros and only speech is counted), so 0 ships; the
# floor rule's best pair reaches the same 0.196, so Otsu ships; eta does not separate files without speech (up to 0.999)
# from good picks (down to 0.76), so no bound ships.  A caller who knows the file is not 40 dB down is better off with lo_bin=1
# (worst error 0 at every gain down to -30 dB).
DEFAULT_RULE = "otsu"
DEFAULT_LO_BIN = 0
DEFAULT_FLOOR_PPM = 200000
DEFAULT_MARGIN_BINS = 10
DEFAULT_MIN_ETA = None
DEFAULT_FALLBACK_BIN = 100  # edges[99] = 10^5: the fixed 50 dB rule
MAX_FRAMES = _native.VAD_MAX_FRAMES

_edges_cache = {}


@dataclass
class ThresholdRecord:
    threshold_bin: int  # speech <=> level >= threshold_bin
    flags: int  # _native.VAD_THR_*
    floor_bin: int  # the floor_ppm quantile of the counted bins, or -1
    top_bin: int  # the highest occupied counted bin, or -1
    n_frames: int
    n_counted: int  # frames at or above lo_bin
    n_speech: int
    eta: float  # Otsu's separability in [0, 1]; 0 under the floor rule and on a fallback


def record_of(row) -> ThresholdRecord:
    """One ``_native.VAD_THRESHOLD_DTYPE`` row as Python numbers."""
    return ThresholdRecord(*(int(row[name]) for name in _native.VAD_THRESHOLD_DTYPE.names[:-1]), float(row["eta"]))


def default_edges() -> np.ndarray:
    """The default table: 10^(k / 20) for k = 1 .. 191, half-dB steps of the mean square from 0.5 to 95.5 dB (191 edges,
    192 level bins); edges[19 + 20 j] are the exact decades, edges[99] = 10^5 is the fixed rule's 50 dB."""
    return np.array([10.0 ** ((k * 0.5) / 10.0) for k in range(1, 192)], dtype=np.float64)


def _check_edges(edges) -> np.ndarray:
    e = np.asarray(edges)
    if e.ndim != 1 or e.dtype.kind not in "fiu" or not 1 <= e.size <= _native.VAD_MAX_EDGES:
        raise ValueError("edges: need 1 to %d numbers in one dimension" % _native.VAD_MAX_EDGES)
    e = np.ascontiguousarray(e, dtype=np.float64)
    if not (np.all(np.isfinite(e)) and np.all(e > 0) and np.all(np.diff(e) > 0)):
        raise ValueError("edges: need positive finite values in strictly ascending order")
    return e


def _edges_checked(edges):
    """(table, n_edges) before anything touches the device: None for the default table, a checked float64 host table, or
    a float64 CUDA vector the caller uploaded (and checked) already."""
    if edges is None:
        return None, 191
    if hasattr(edges, "is_cuda"):
        import torch

        if not (edges.is_cuda and edges.dtype == torch.float64 and edges.dim() == 1 and edges.is_contiguous()
                and 1 <= edges.numel() <= _native.VAD_MAX_EDGES):
            raise ValueError("edges: a device table must be a contiguous float64 CUDA vector of 1 to %d entries" % _native.VAD_MAX_EDGES)
        return edges, int(edges.numel())
    e = _check_edges(edges)
    return e, int(e.size)


def _edges_dev(table, device):
    """The checked table of :func:`_edges_checked` as a float64 CUDA tensor (the default one is uploaded once per device)."""
    torch = _native.require_gpu()
    if table is None:
        key = str(device)
        if key not in _edges_cache:
            _edges_cache[key] = torch.from_numpy(default_edges()).to(device)
        return _edges_cache[key]
    return table if hasattr(table, "is_cuda") else torch.from_numpy(table).to(device)


def _check_pcm(pcm_dev, frame_len) -> int:
    import torch

    if isinstance(frame_len, bool) or not isinstance(frame_len, (int, np.integer)) or frame_len < 1:
        raise ValueError("frame_len=%r: need an integer >= 1" % (frame_len,))
    if not (hasattr(pcm_dev, "is_cuda") and pcm_dev.is_cuda and pcm_dev.dtype == torch.int16 and pcm_dev.dim() == 1
            and pcm_dev.is_contiguous()):
        raise ValueError("pcm: need a contiguous int16 CUDA vector")
    return int(frame_len)


def _check_levels(levels) -> None:
    import torch

    if not (hasattr(levels, "is_cuda") and levels.is_cuda and levels.dtype == torch.uint8 and levels.dim() == 1
            and levels.is_contiguous()):
        raise ValueError("levels: need a contiguous uint8 CUDA vector")


def _check_label(non_speech_label) -> float:
    if isinstance(non_speech_label, bool) or not isinstance(non_speech_label, (int, float)) or not math.isfinite(non_speech_label):
        raise ValueError("non_speech_label=%r: need a finite number" % (non_speech_label,))
    return float(non_speech_label)


def rule_code(rule) -> int:
    if isinstance(rule, str) and rule.strip().lower() in _native.VAD_RULES:
        return _native.VAD_RULES[rule.strip().lower()]
    raise ValueError("unknown rule %r: expected one of %s" % (rule, ", ".join(sorted(_native.VAD_RULES))))


def _check_pick(n_bins, rule, lo_bin, t_min, t_max, fallback_bin, floor_ppm, margin_bins):
    """The ranges of ``ffs_vad_pick_threshold``; returns the integer arguments behind n_bins, defaults filled in."""
    code = rule_code(rule)
    if isinstance(n_bins, bool) or not isinstance(n_bins, (int, np.integer)) or not 2 <= n_bins <= _native.VAD_MAX_BINS:
        raise ValueError("n_bins=%r: need an integer in [2, %d]" % (n_bins, _native.VAD_MAX_BINS))
    if isinstance(lo_bin, bool) or not isinstance(lo_bin, (int, np.integer)):
        raise ValueError("lo_bin=%r: need an integer" % (lo_bin,))
    t_min = lo_bin + 1 if t_min is None else t_min
    t_max = n_bins - 1 if t_max is None else t_max
    fallback_bin = min(DEFAULT_FALLBACK_BIN, n_bins) if fallback_bin is None else fallback_bin
    for name, v in (("lo_bin", lo_bin), ("t_min", t_min), ("t_max", t_max), ("fallback_bin", fallback_bin),
                    ("floor_ppm", floor_ppm), ("margin_bins", margin_bins)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s=%r: need an integer" % (name, v))
    if not 0 <= lo_bin < t_min <= t_max <= n_bins - 1:
        raise ValueError("need 0 <= lo_bin=%d < t_min=%d <= t_max=%d <= n_bins - 1 = %d" % (lo_bin, t_min, t_max, n_bins - 1))
    if not 0 <= fallback_bin <= n_bins:
        raise ValueError("fallback_bin=%d: need a bin in [0, %d]" % (fallback_bin, n_bins))
    if not 0 <= floor_ppm <= 1000000:
        raise ValueError("floor_ppm=%d: need parts per million in [0, 1000000]" % floor_ppm)
    if not 0 <= margin_bins <= _native.VAD_MAX_EDGES:
        raise ValueError("margin_bins=%d: need bins in [0, %d]" % (margin_bins, _native.VAD_MAX_EDGES))
    return code, int(lo_bin), int(t_min), int(t_max), int(fallback_bin), int(floor_ppm), int(margin_bins)


def frame_levels(pcm_dev, frame_len: int, edges=None, out=None):
    """uint8 CUDA level per frame of an int16 CUDA vector of mono PCM: the number of ``edges`` (default
    :func:`default_edges`) the frame's mean square reaches.  ``out``: a contiguous uint8 CUDA vector to write into, e.g.
    ``levels[first_frame:]`` of a whole file's vector when the file is swept chunk by chunk; any offset will do."""
    table, n_edges = _edges_checked(edges)
    frame_len = _check_pcm(pcm_dev, frame_len)
    torch = _native.require_gpu()
    n = int(pcm_dev.numel())
    n_frames = (n + frame_len - 1) // frame_len
    table = _edges_dev(table, pcm_dev.device)
    if out is None:
        out = torch.empty(n_frames, dtype=torch.uint8, device=pcm_dev.device)
    else:
        _check_levels(out)
        if out.numel() < n_frames or out.device != pcm_dev.device:
            raise ValueError("out: need %d level bytes on the PCM's device" % n_frames)
    if n:
        _native.check(_native.load().ffs_vad_levels(pcm_dev.data_ptr(), n, frame_len, table.data_ptr(), n_edges,
                                                    out.data_ptr(), _native.current_stream_ptr(torch)))
    return out[:n_frames]


def level_hist(levels, n_bins: int = 192, out=None):
    """int32 CUDA counts of the level bytes, ``n_bins`` = edges + 1 of them (overwrites ``out`` when given)."""
    if isinstance(n_bins, bool) or not isinstance(n_bins, (int, np.integer)) or not 2 <= n_bins <= _native.VAD_MAX_BINS:
        raise ValueError("n_bins=%r: need an integer in [2, %d]" % (n_bins, _native.VAD_MAX_BINS))
    _check_levels(levels)
    torch = _native.require_gpu()
    if out is None:
        out = torch.empty(int(n_bins), dtype=torch.int32, device=levels.device)
    elif not (out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and out.numel() >= n_bins and out.device == levels.device):
        raise ValueError("out: need a contiguous int32 CUDA vector of %d counts on the levels' device" % n_bins)
    n = int(levels.numel())
    _native.check(_native.load().ffs_vad_level_hist(levels.data_ptr() if n else None, n, int(n_bins), out.data_ptr(),
                                                    _native.current_stream_ptr(torch)))
    return out[:int(n_bins)]


def pick_threshold_device(hist, rule: str = DEFAULT_RULE, lo_bin: int = DEFAULT_LO_BIN, t_min: Optional[int] = None,
                          t_max: Optional[int] = None, fallback_bin: Optional[int] = None, floor_ppm: int = DEFAULT_FLOOR_PPM,
                          margin_bins: int = DEFAULT_MARGIN_BINS, out=None):
    """``ffs_vad_pick_threshold`` on the current stream: ``hist`` an int32 CUDA tensor, [n_bins] or [n_hist, n_bins];
    returns the uint8 CUDA tensor of the 48-byte records (nothing is read back; ``level_labels`` takes it as is)."""
    import torch

    if not (hasattr(hist, "is_cuda") and hist.dtype == torch.int32 and hist.dim() in (1, 2) and hist.is_contiguous()):
        raise ValueError("hist: need a contiguous int32 CUDA tensor, [n_bins] or [n_hist, n_bins]")
    n_bins = int(hist.shape[-1])
    n_hist = 1 if hist.dim() == 1 else int(hist.shape[0])
    args = _check_pick(n_bins, rule, lo_bin, t_min, t_max, fallback_bin, floor_ppm, margin_bins)
    if not hist.is_cuda:
        raise ValueError("hist: need a contiguous int32 CUDA tensor, [n_bins] or [n_hist, n_bins]")
    torch = _native.require_gpu()
    if out is None:
        out = torch.empty(max(n_hist, 1) * _native.VAD_THRESHOLD_BYTES, dtype=torch.uint8, device=hist.device)
    elif not (out.is_cuda and out.is_contiguous() and _native._nbytes(out) >= n_hist * _native.VAD_THRESHOLD_BYTES
              and out.device == hist.device):
        raise ValueError("out: need %d bytes on the histogram's device" % (n_hist * _native.VAD_THRESHOLD_BYTES))
    _native.check(_native.load().ffs_vad_pick_threshold(hist.data_ptr(), n_hist, n_bins, *args, out.data_ptr(),
                                                        _native.current_stream_ptr(torch)))
    return out


def _records(raw, n_hist) -> List[ThresholdRecord]:
    rows = raw.cpu().numpy()[:n_hist * _native.VAD_THRESHOLD_BYTES].view(_native.VAD_THRESHOLD_DTYPE)
    return [record_of(r) for r in rows]


def pick_threshold(hist, rule: str = DEFAULT_RULE, **params) -> Union[ThresholdRecord, List[ThresholdRecord]]:
    """The record of one histogram ([n_bins]) or the list of records of many ([n_hist, n_bins]); see
    :func:`pick_threshold_device` for the parameters.  Reads the records back."""
    raw = pick_threshold_device(hist, rule, **params)
    return _records(raw, 1)[0] if hist.dim() == 1 else _records(raw, int(hist.shape[0]))


def level_labels(levels, threshold, non_speech_label: float = 0.0, packed: bool = False):
    """Labels of the level bytes: speech iff level >= threshold.  ``threshold``: a bin in [0, 256], or a CUDA tensor
    whose first four bytes hold it (the record tensor of :func:`pick_threshold_device`, or an int32 tensor) -- read on
    the device, nothing waits for it.  Returns float32 CUDA labels (1.0 / float32(non_speech_label)), or with ``packed``
    the bit-packed ``DeviceRaster`` the aligner reads (``non_speech_label`` becomes its low level)."""
    import torch

    non_speech_label = _check_label(non_speech_label)
    if hasattr(threshold, "is_cuda"):
        if not (threshold.is_cuda and threshold.is_contiguous() and _native._nbytes(threshold) >= 4
                and threshold.dtype in (torch.uint8, torch.int32)):
            raise ValueError("threshold: a device threshold must be a contiguous uint8 or int32 CUDA tensor of 4 bytes or more")
        thr_dev, thr_host = threshold.data_ptr(), 0
    elif isinstance(threshold, bool) or not isinstance(threshold, (int, np.integer)) or not 0 <= threshold <= _native.VAD_MAX_BINS:
        raise ValueError("threshold=%r: need a bin in [0, %d] or a device tensor" % (threshold, _native.VAD_MAX_BINS))
    else:
        thr_dev, thr_host = None, int(threshold)
    _check_levels(levels)
    if thr_dev is not None and threshold.device != levels.device:
        raise ValueError("threshold: a device threshold must be on the levels' device")
    torch = _native.require_gpu()
    n = int(levels.numel())
    if packed:
        out = torch.zeros((n + 31) // 32, dtype=torch.int32, device=levels.device)
    else:
        out = torch.empty(n, dtype=torch.float32, device=levels.device)
    if n:
        _native.check(_native.load().ffs_vad_level_labels(levels.data_ptr(), n, thr_dev, thr_host, float(non_speech_label),
                                                          None if packed else out.data_ptr(), out.data_ptr() if packed else None,
                                                          _native.current_stream_ptr(torch)))
    if packed:
        from .subtitle_raster import DeviceRaster

        return DeviceRaster(out, float(non_speech_label), 1.0, n)
    return out


def threshold_db(record: ThresholdRecord, edges=None) -> float:
    """The record's threshold as a level of the mean square in dB: 10 log10(edges[threshold_bin - 1]); -inf for bin 0
    (every frame is speech), +inf for a bin behind the table (none is)."""
    e = default_edges() if edges is None else _check_edges(edges)
    t = int(record.threshold_bin)
    if t <= 0:
        return -math.inf
    return math.inf if t > e.size else 10.0 * math.log10(float(e[t - 1]))


def _finish(levels, n_bins, non_speech_label, packed, rule, params, gate=None, centre=None):
    """Histogram, pick and labels queued behind pass 1 on the current stream; only the record is read back.  With
    ``gate`` = (dip_bins, max_run) the labels are :func:`steady_gate`'s and its record is read back too.  With ``centre``
    = (side levels, min_contrast_bins) ``levels`` are the mid levels: the pick runs on their histogram, the labels (or
    the steady-run gate) on :func:`centre_gate`'s output, and the centre record follows the threshold's."""
    raw = pick_threshold_device(level_hist(levels, n_bins), rule, **params)
    records = ()
    if centre is not None:
        levels, centre_raw = centre_gate(levels, centre[0], raw, centre[1])
        records = (centre_raw,)
    if gate is None:
        labels = level_labels(levels, raw, non_speech_label, packed)
    else:
        labels, gate_raw = steady_gate(levels, raw, gate[0], gate[1], non_speech_label, packed)
    out = (labels, _records(raw, 1)[0])
    if centre is not None:
        out += (centre_record_of(records[0].cpu().numpy().view(_native.VAD_CENTRE_DTYPE)[0]),)
    if gate is not None:
        out += (gate_record_of(gate_raw.cpu().numpy().view(_native.VAD_GATE_DTYPE)[0]),)
    return out


def _check_detect(sample_rate, frame_rate, non_speech_label, n_bins, rule, params) -> int:
    from .speech_transformers import frames_per_window

    _check_label(non_speech_label)
    if not (sample_rate > 0 and frame_rate > 0) or frames_per_window(sample_rate, frame_rate) < 1:
        raise ValueError("sample_rate=%r, frame_rate=%r: need at least one PCM sample per frame" % (sample_rate, frame_rate))
    unknown = set(params) - {"lo_bin", "t_min", "t_max", "fallback_bin", "floor_ppm", "margin_bins"}
    if unknown:
        raise ValueError("unknown parameter %s" % ", ".join(sorted(unknown)))
    full = dict(lo_bin=DEFAULT_LO_BIN, t_min=None, t_max=None, fallback_bin=None, floor_ppm=DEFAULT_FLOOR_PPM,
                margin_bins=DEFAULT_MARGIN_BINS)
    full.update(params)
    _check_pick(n_bins, rule, **full)
    return frames_per_window(sample_rate, frame_rate)


def detect_device_adaptive(pcm_dev, sample_rate: int, frame_rate: int, non_speech_label: float, rule: str = DEFAULT_RULE,
                           edges=None, packed: bool = False, **params):
    """The adaptive detector for PCM resident in HBM (int16 CUDA vector): (float32 CUDA labels, or with ``packed`` the
    bit-packed ``DeviceRaster``; the file's ``ThresholdRecord``).  The four launches are queued on the current stream
    and only the 48-byte record is read back.  ``params``: lo_bin, t_min, t_max, fallback_bin, floor_ppm, margin_bins."""
    table, n_edges = _edges_checked(edges)
    frame_len = _check_detect(sample_rate, frame_rate, non_speech_label, n_edges + 1, rule, params)
    _check_pcm(pcm_dev, frame_len)
    table = _edges_dev(table, pcm_dev.device)
    levels = frame_levels(pcm_dev, frame_len, table)
    return _finish(levels, n_edges + 1, non_speech_label, packed, rule, params)


def _pinned_levels(pcm_host, frame_len, table, n_edges, staging):
    """Pass 1 behind ``stream_pinned_buffers``: the level bytes of the whole pinned stream, queued on the current stream."""
    from .speech_transformers import WINDOWS_PER_BUFFER, stream_pinned_buffers

    torch = _native.require_gpu()
    table = _edges_dev(table, torch.device("cuda", torch.cuda.current_device()))
    n = int(pcm_host.numel())
    levels = torch.empty((n + frame_len - 1) // frame_len, dtype=torch.uint8, device="cuda")
    lib = _native.load()

    def sweep(buf, m, o, main):
        _native.check(lib.ffs_vad_levels(buf.data_ptr(), m, frame_len, table.data_ptr(), n_edges,
                                         levels.data_ptr() + o // frame_len, main.cuda_stream))

    stream_pinned_buffers(pcm_host, frame_len * WINDOWS_PER_BUFFER, staging, sweep)
    return levels


def _check_pinned(pcm_host) -> None:
    import torch

    if not (hasattr(pcm_host, "is_cuda") and not pcm_host.is_cuda and pcm_host.dtype == torch.int16 and pcm_host.dim() == 1
            and pcm_host.is_contiguous()):
        raise ValueError("pcm: need a contiguous int16 CPU vector (pinned for the copies to overlap)")


def detect_pinned_stream_adaptive(pcm_host, sample_rate: int, frame_rate: int, non_speech_label: float,
                                  rule: str = DEFAULT_RULE, edges=None, staging=None, packed: bool = False, **params):
    """The adaptive detector behind ``detect_pinned_stream``'s double-buffered copy loop, for decoded s16le PCM in pinned
    host memory (int16 CPU tensor): pass 1 runs per 100 s buffer while the next one is copied, the histogram, the pick
    and the labels run once at the end.  Returns what :func:`detect_device_adaptive` returns."""
    table, n_edges = _edges_checked(edges)
    frame_len = _check_detect(sample_rate, frame_rate, non_speech_label, n_edges + 1, rule, params)
    _check_pinned(pcm_host)
    levels = _pinned_levels(pcm_host, frame_len, table, n_edges, staging)
    return _finish(levels, n_edges + 1, non_speech_label, packed, rule, params)


def assess(record: ThresholdRecord, min_eta: Optional[float] = DEFAULT_MIN_ETA) -> List[str]:
    """Reasons not to trust the record's threshold ([] = none found): a fallback to the fixed rule and why, a clamped
    result, a flat file, and -- only with a ``min_eta``; the calibration ships none -- an Otsu split that explains too
    little of the level variance."""
    if min_eta is not None and not (isinstance(min_eta, (int, float)) and 0.0 <= min_eta <= 1.0):
        raise ValueError("min_eta=%r: need a share in [0, 1]" % (min_eta,))
    f, reasons = int(record.flags), []
    if f & _native.VAD_THR_TOO_LONG:
        reasons.append("too many frames for one histogram (%d > %d): fixed rule used" % (record.n_frames, MAX_FRAMES))
    elif f & _native.VAD_THR_EMPTY:
        reasons.append("no frame at or above the silence bin (%d frames): fixed rule used" % record.n_frames)
    elif f & _native.VAD_THR_FALLBACK:
        reasons.append("all %d counted frames share level bin %d: fixed rule used" % (record.n_counted, record.top_bin))
    elif f & _native.VAD_THR_FLAT:
        reasons.append("all %d counted frames share level bin %d" % (record.n_counted, record.top_bin))
    if f & _native.VAD_THR_CLAMPED_LO:
        reasons.append("threshold clamped up to bin %d" % record.threshold_bin)
    if f & _native.VAD_THR_CLAMPED_HI:
        reasons.append("threshold clamped down to bin %d" % record.threshold_bin)
    if min_eta is not None and not f & _native.VAD_THR_FALLBACK and record.eta < min_eta:
        reasons.append("levels do not split into two classes (eta %.2f < %.2f)" % (record.eta, min_eta))
    return reasons


# ---- steady-run gate ---------------------------------------------------------------------------------
# By the rule of profiles/steady_gate_calibrate.py on the CPU model (profiles/steady_gate_calibration.json; the synthetic
# 10 min files of the adaptive calibration, SYNTHETIC data only): dip_bins = 0 rejects the least (the kept set shrinks
# as dip_bins grows) and already takes the music share labelled speech from 1.000 to 0.000, so 0 ships.  max_run is the
# reference's longest cue, DEFAULT_MAX_SUBTITLE_SECONDS, in frames.
DEFAULT_DIP_BINS = 0


def default_max_run(sample_rate: int = 100) -> int:
    """The longest cue the reference lets through, in frames of ``sample_rate`` per second: no subtitle can vouch for a
    longer stretch of uninterrupted activity."""
    from .constants import DEFAULT_MAX_SUBTITLE_SECONDS

    return int(DEFAULT_MAX_SUBTITLE_SECONDS * sample_rate)


DEFAULT_MAX_RUN = default_max_run()


@dataclass
class GateRecord:
    threshold_bin: int  # the threshold the gate used
    flags: int  # _native.VAD_GATE_*
    n_stretches: int
    n_rejected: int  # stretches longer than max_run
    longest_run: int  # frames of the longest stretch, 0: none
    n_frames: int
    n_active: int  # frames at or above the threshold
    n_kept: int  # of them, labelled speech


def gate_record_of(row) -> GateRecord:
    """One ``_native.VAD_GATE_DTYPE`` row as Python numbers."""
    return GateRecord(*(int(row[name]) for name in _native.VAD_GATE_DTYPE.names if name != "reserved"))


def _check_gate(dip_bins, max_run):
    if isinstance(dip_bins, bool) or not isinstance(dip_bins, (int, np.integer)) or not 0 <= dip_bins <= _native.VAD_MAX_EDGES:
        raise ValueError("dip_bins=%r: need bins in [0, %d]" % (dip_bins, _native.VAD_MAX_EDGES))
    if isinstance(max_run, bool) or not isinstance(max_run, (int, np.integer)) or not 1 <= max_run <= 2 ** 31 - 1:
        raise ValueError("max_run=%r: need frames in [1, 2^31 - 1]" % (max_run,))
    return int(dip_bins), int(max_run)


def steady_gate(levels, threshold, dip_bins: int = DEFAULT_DIP_BINS, max_run: int = DEFAULT_MAX_RUN,
                non_speech_label: float = 0.0, packed: bool = False):
    """:func:`level_labels` without the stretches of uninterrupted activity longer than ``max_run`` frames
    (``ffs_vad_steady_gate``): a frame is speech iff level >= threshold and its stretch -- from the first active frame
    behind a frame below ``threshold - dip_bins`` to the last one in front of the next -- is at most ``max_run`` long.
    ``threshold``: a bin in [0, 256], a :class:`ThresholdRecord`, or the device tensor of :func:`pick_threshold_device`
    (read on the device, never read back).  Returns (float32 CUDA labels or with ``packed`` the ``DeviceRaster``, the uint8
    CUDA tensor of the 48-byte gate record); three launches queued on the current stream, nothing is read back."""
    import torch

    non_speech_label = _check_label(non_speech_label)
    dip_bins, max_run = _check_gate(dip_bins, max_run)
    if isinstance(threshold, ThresholdRecord):
        threshold = threshold.threshold_bin
    if hasattr(threshold, "is_cuda"):
        if not (threshold.is_cuda and threshold.is_contiguous() and _native._nbytes(threshold) >= 4
                and threshold.dtype in (torch.uint8, torch.int32)):
            raise ValueError("threshold: a device threshold must be a contiguous uint8 or int32 CUDA tensor of 4 bytes or more")
        thr_dev, thr_host = threshold.data_ptr(), 0
    elif isinstance(threshold, bool) or not isinstance(threshold, (int, np.integer)) or not 0 <= threshold <= _native.VAD_MAX_BINS:
        raise ValueError("threshold=%r: need a bin in [0, %d], a ThresholdRecord or a device tensor" % (threshold, _native.VAD_MAX_BINS))
    else:
        thr_dev, thr_host = None, int(threshold)
    _check_levels(levels)
    if thr_dev is not None and threshold.device != levels.device:
        raise ValueError("threshold: a device threshold must be on the levels' device")
    torch = _native.require_gpu()
    lib = _native.load()
    n = int(levels.numel())
    if packed:
        out = torch.zeros((n + 31) // 32, dtype=torch.int32, device=levels.device)
    else:
        out = torch.empty(n, dtype=torch.float32, device=levels.device)
    record = torch.empty(_native.VAD_GATE_BYTES, dtype=torch.uint8, device=levels.device)
    ws_bytes = int(lib.ffs_vad_steady_gate_workspace_bytes(n))
    workspace = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=levels.device)
    with torch.cuda.device(levels.device):
        _native.check(lib.ffs_vad_steady_gate(levels.data_ptr() if n else None, n, thr_dev, thr_host, dip_bins, max_run,
                                              float(non_speech_label), None if packed or not n else out.data_ptr(),
                                              out.data_ptr() if packed and n else None, record.data_ptr(), workspace.data_ptr(),
                                              ws_bytes, _native.current_stream_ptr(torch)))
    if packed:
        from .subtitle_raster import DeviceRaster

        return DeviceRaster(out, float(non_speech_label), 1.0, n), record
    return out, record


def _check_detect_gated(sample_rate, dip_bins, max_run):
    return _check_gate(dip_bins, default_max_run(sample_rate) if max_run is None else max_run)


def detect_device_gated(pcm_dev, sample_rate: int, frame_rate: int, non_speech_label: float, rule: str = DEFAULT_RULE,
                        edges=None, packed: bool = False, dip_bins: int = DEFAULT_DIP_BINS, max_run: Optional[int] = None,
                        **params):
    """:func:`detect_device_adaptive` with the steady-run gate behind the pick: (labels or ``DeviceRaster``, the file's
    ``ThresholdRecord``, its ``GateRecord``).  ``max_run`` defaults to ``default_max_run(sample_rate)``, ten seconds of
    frames.  Seven launches queued on the current stream; only the two 48-byte records are read back."""
    table, n_edges = _edges_checked(edges)
    frame_len = _check_detect(sample_rate, frame_rate, non_speech_label, n_edges + 1, rule, params)
    gate = _check_detect_gated(sample_rate, dip_bins, max_run)
    _check_pcm(pcm_dev, frame_len)
    table = _edges_dev(table, pcm_dev.device)
    levels = frame_levels(pcm_dev, frame_len, table)
    return _finish(levels, n_edges + 1, non_speech_label, packed, rule, params, gate)


def detect_pinned_stream_gated(pcm_host, sample_rate: int, frame_rate: int, non_speech_label: float,
                               rule: str = DEFAULT_RULE, edges=None, staging=None, packed: bool = False,
                               dip_bins: int = DEFAULT_DIP_BINS, max_run: Optional[int] = None, **params):
    """:func:`detect_pinned_stream_adaptive` with the steady-run gate behind the pick; returns what
    :func:`detect_device_gated` returns."""
    table, n_edges = _edges_checked(edges)
    frame_len = _check_detect(sample_rate, frame_rate, non_speech_label, n_edges + 1, rule, params)
    gate = _check_detect_gated(sample_rate, dip_bins, max_run)
    _check_pinned(pcm_host)
    levels = _pinned_levels(pcm_host, frame_len, table, n_edges, staging)
    return _finish(levels, n_edges + 1, non_speech_label, packed, rule, params, gate)


def assess_gate(record: GateRecord, max_rejected_share: Optional[float] = None) -> List[str]:
    """What the gate record says about the file ([] = nothing to report): the gate was skipped, no frame could close a
    stretch, everything active was rejected, and -- only with a ``max_rejected_share``; the calibration ships none --
    more than that share of the active frames was dropped.  It reports; it decides nothing."""
    if max_rejected_share is not None and not (isinstance(max_rejected_share, (int, float)) and not isinstance(max_rejected_share, bool)
                                               and 0.0 <= max_rejected_share <= 1.0):
        raise ValueError("max_rejected_share=%r: need a share in [0, 1]" % (max_rejected_share,))
    f, reasons = int(record.flags), []
    if f & _native.VAD_GATE_TOO_LONG:
        reasons.append("too many frames for the gate (%d > %d): plain labels" % (record.n_frames, MAX_FRAMES))
        return reasons
    if f & _native.VAD_GATE_NO_QUIET:
        reasons.append("no level lies below threshold bin %d minus the dip: nothing can close a stretch" % record.threshold_bin)
    if f & _native.VAD_GATE_ALL_REJECTED:
        reasons.append("all %d active frames lie in stretches longer than the limit (longest %d)" % (record.n_active, record.longest_run))
    elif max_rejected_share is not None and record.n_active > 0:
        share = (record.n_active - record.n_kept) / float(record.n_active)
        if share > max_rejected_share:
            reasons.append("%.2f of the active frames dropped in %d of %d stretches (limit %.2f)"
                           % (share, record.n_rejected, record.n_stretches, max_rejected_share))
    return reasons


# ---- centre-channel VAD: mid / side contrast of stereo PCM -------------------------------------------
# The project's own rule with no upstream counterpart: parity is against the in-repo model tests/stereo_vad_model.py only.
# By the rule of profiles/centre_gate_calibrate.py on the CPU model (profiles/centre_gate_calibration.json; the synthetic
# 10 min "mixed" files of the adaptive calibration made stereo, SYNTHETIC data only): the largest candidate of 0, 6, 12,
# 18, 24 bins that keeps at least 0.99 of the speech frames c = 0 keeps on every file where the pick finds the speech.
# Speech over a wide bed 10 dB below its mean level loses 1.7 % of its frames at c = 6 already (16 % at 12: the quietest
# frames of a burst lie below the bed), so no candidate above 0 qualifies and 0 SHIPS: a frame is rejected only when its
# side level exceeds its mid level.  That takes the share of uncorrelated (rho = 0) music labelled speech from 1.00 to
# 0.76 only; c = 6 takes it to 0.00 and c = 12 does the same up to rho = 0.5 (0.02) while keeping 1.00 of plain speech
# and of speech over a bed 20 dB down.  A caller who knows the beds pass ``min_contrast_bins`` (``vad="centre:12"``).
DEFAULT_MIN_CONTRAST_BINS = 0


@dataclass
class CentreRecord:
    threshold_bin: int  # the threshold the gate used
    flags: int  # _native.VAD_CENTRE_*
    min_contrast_bins: int  # the contrast the gate asked for
    max_side: int  # the largest side level, 0: none (dual mono)
    n_frames: int
    n_active: int  # frames whose mid level reaches the threshold
    n_kept: int  # of them, with mid - side >= min_contrast_bins
    sum_contrast: int  # signed sum of mid - side over the active frames


def centre_record_of(row) -> CentreRecord:
    """One ``_native.VAD_CENTRE_DTYPE`` row as Python numbers."""
    return CentreRecord(*(int(row[name]) for name in _native.VAD_CENTRE_DTYPE.names))


def _check_contrast(min_contrast_bins) -> int:
    if isinstance(min_contrast_bins, bool) or not isinstance(min_contrast_bins, (int, np.integer)) \
            or not 0 <= min_contrast_bins <= _native.VAD_MAX_EDGES:
        raise ValueError("min_contrast_bins=%r: need bins in [0, %d]" % (min_contrast_bins, _native.VAD_MAX_EDGES))
    return int(min_contrast_bins)


def _check_stereo_pcm(pcm_dev, frame_len) -> int:
    frame_len = _check_pcm(pcm_dev, frame_len)
    if int(pcm_dev.numel()) % 2:
        raise ValueError("pcm: %d int16 values are not interleaved (L, R) pairs" % int(pcm_dev.numel()))
    return frame_len


def stereo_levels(pcm_dev, frame_len: int, edges=None, out=None):
    """(mid, side): uint8 CUDA levels per frame of an int16 CUDA vector of interleaved (L, R) pairs, ``frame_len`` pairs a
    frame: the number of ``edges`` (default :func:`default_edges`) that sum (L + R)^2 / (4 n) and sum (L - R)^2 / (4 n)
    reach.  For L == R mid is :func:`frame_levels` of one channel and side is all zero.  ``out``: a pair of contiguous
    uint8 CUDA vectors to write into (any offset will do)."""
    table, n_edges = _edges_checked(edges)
    frame_len = _check_stereo_pcm(pcm_dev, frame_len)
    n = int(pcm_dev.numel()) // 2
    n_frames = (n + frame_len - 1) // frame_len
    if out is not None:
        if not (isinstance(out, (tuple, list)) and len(out) == 2):
            raise ValueError("out: need a pair of level vectors (mid, side)")
        for o in out:
            _check_levels(o)
            if o.numel() < n_frames or o.device != pcm_dev.device:
                raise ValueError("out: need %d level bytes on the PCM's device" % n_frames)
    torch = _native.require_gpu()
    table = _edges_dev(table, pcm_dev.device)
    if out is None:
        both = torch.empty((2, n_frames), dtype=torch.uint8, device=pcm_dev.device)
        mid, side = both[0], both[1]
    else:
        mid, side = out
    if n:
        _native.check(_native.load().ffs_vad_stereo_levels(pcm_dev.data_ptr(), n, frame_len, table.data_ptr(), n_edges,
                                                           mid.data_ptr(), side.data_ptr(), _native.current_stream_ptr(torch)))
    return mid[:n_frames], side[:n_frames]


def centre_gate(mid, side, threshold, min_contrast_bins: int = DEFAULT_MIN_CONTRAST_BINS, out=None):
    """The mid levels with every frame zeroed whose mid level stands less than ``min_contrast_bins`` above its side level
    (``ffs_vad_centre_gate``): :func:`level_labels` and :func:`steady_gate` run on the result unchanged.  ``threshold``
    (it only counts: a frame is active iff mid >= threshold): a bin in [0, 256], a :class:`ThresholdRecord`, or the device
    tensor of :func:`pick_threshold_device` (read on the device, never read back).  Returns (uint8 CUDA levels, the uint8
    CUDA tensor of the 48-byte centre record); two launches queued on the current stream, nothing is read back."""
    import torch

    c = _check_contrast(min_contrast_bins)
    if isinstance(threshold, ThresholdRecord):
        threshold = threshold.threshold_bin
    if hasattr(threshold, "is_cuda"):
        if not (threshold.is_cuda and threshold.is_contiguous() and _native._nbytes(threshold) >= 4
                and threshold.dtype in (torch.uint8, torch.int32)):
            raise ValueError("threshold: a device threshold must be a contiguous uint8 or int32 CUDA tensor of 4 bytes or more")
        thr_dev, thr_host = threshold.data_ptr(), 0
    elif isinstance(threshold, bool) or not isinstance(threshold, (int, np.integer)) or not 0 <= threshold <= _native.VAD_MAX_BINS:
        raise ValueError("threshold=%r: need a bin in [0, %d], a ThresholdRecord or a device tensor" % (threshold, _native.VAD_MAX_BINS))
    else:
        thr_dev, thr_host = None, int(threshold)
    _check_levels(mid)
    _check_levels(side)
    n = int(mid.numel())
    if int(side.numel()) != n or side.device != mid.device:
        raise ValueError("side: need %d level bytes on the mid levels' device" % n)
    if thr_dev is not None and threshold.device != mid.device:
        raise ValueError("threshold: a device threshold must be on the levels' device")
    if out is not None:
        _check_levels(out)
        if out.numel() < n or out.device != mid.device:
            raise ValueError("out: need %d level bytes on the levels' device" % n)
        lo, hi = out.data_ptr(), out.data_ptr() + n
        if n and any(lo < t.data_ptr() + n and t.data_ptr() < hi for t in (mid, side)):
            raise ValueError("out: must not overlap mid or side")
    torch = _native.require_gpu()
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=mid.device)
    record = torch.empty(_native.VAD_CENTRE_BYTES, dtype=torch.uint8, device=mid.device)
    with torch.cuda.device(mid.device):
        _native.check(_native.load().ffs_vad_centre_gate(mid.data_ptr() if n else None, side.data_ptr() if n else None, n,
                                                         thr_dev, thr_host, c, out.data_ptr() if n else None,
                                                         record.data_ptr(), _native.current_stream_ptr(torch)))
    return out[:n], record


def _check_detect_centre(sample_rate, min_contrast_bins, steady, dip_bins, max_run):
    if not isinstance(steady, bool):
        raise ValueError("steady=%r: need True or False" % (steady,))
    c = _check_contrast(min_contrast_bins)
    gate = _check_detect_gated(sample_rate, dip_bins, max_run)
    return c, (gate if steady else None)


def detect_device_centre(pcm_dev, sample_rate: int, frame_rate: int, non_speech_label: float, rule: str = DEFAULT_RULE,
                         edges=None, packed: bool = False, min_contrast_bins: int = DEFAULT_MIN_CONTRAST_BINS,
                         steady: bool = False, dip_bins: int = DEFAULT_DIP_BINS, max_run: Optional[int] = None, **params):
    """The centre-channel detector for stereo PCM resident in HBM (int16 CUDA vector of interleaved (L, R) pairs,
    ``frame_rate`` pairs a second): (labels or ``DeviceRaster``, the file's ``ThresholdRecord`` -- picked on the histogram
    of the mid levels of all frames --, its ``CentreRecord``) and, with ``steady``, the ``GateRecord`` of the steady-run
    gate run on the centre gate's output.  Everything is queued on the current stream; only the records are read back."""
    table, n_edges = _edges_checked(edges)
    frame_len = _check_detect(sample_rate, frame_rate, non_speech_label, n_edges + 1, rule, params)
    c, gate = _check_detect_centre(sample_rate, min_contrast_bins, steady, dip_bins, max_run)
    _check_stereo_pcm(pcm_dev, frame_len)
    table = _edges_dev(table, pcm_dev.device)
    mid, side = stereo_levels(pcm_dev, frame_len, table)
    return _finish(mid, n_edges + 1, non_speech_label, packed, rule, params, gate, (side, c))


def _pinned_stereo_levels(pcm_host, frame_len, table, n_edges, staging):
    """The stereo pass 1 behind ``stream_pinned_buffers``: buffers of WINDOWS_PER_BUFFER frames of pairs."""
    from .speech_transformers import WINDOWS_PER_BUFFER, stream_pinned_buffers

    torch = _native.require_gpu()
    table = _edges_dev(table, torch.device("cuda", torch.cuda.current_device()))
    n = int(pcm_host.numel()) // 2
    both = torch.empty((2, (n + frame_len - 1) // frame_len), dtype=torch.uint8, device="cuda")
    lib = _native.load()

    def sweep(buf, m, o, main):  # m, o in int16 values: two a pair
        first = o // (2 * frame_len)
        _native.check(lib.ffs_vad_stereo_levels(buf.data_ptr(), m // 2, frame_len, table.data_ptr(), n_edges,
                                                both[0].data_ptr() + first, both[1].data_ptr() + first, main.cuda_stream))

    stream_pinned_buffers(pcm_host, 2 * frame_len * WINDOWS_PER_BUFFER, staging, sweep)
    return both[0], both[1]


def detect_pinned_stream_centre(pcm_host, sample_rate: int, frame_rate: int, non_speech_label: float,
                                rule: str = DEFAULT_RULE, edges=None, staging=None, packed: bool = False,
                                min_contrast_bins: int = DEFAULT_MIN_CONTRAST_BINS, steady: bool = False,
                                dip_bins: int = DEFAULT_DIP_BINS, max_run: Optional[int] = None, **params):
    """:func:`detect_device_centre` behind ``detect_pinned_stream``'s double-buffered copy loop, for decoded two-channel
    s16le PCM in pinned host memory (int16 CPU tensor of interleaved pairs; staging buffers of their own hold
    2 * frame_len * WINDOWS_PER_BUFFER values)."""
    table, n_edges = _edges_checked(edges)
    frame_len = _check_detect(sample_rate, frame_rate, non_speech_label, n_edges + 1, rule, params)
    c, gate = _check_detect_centre(sample_rate, min_contrast_bins, steady, dip_bins, max_run)
    _check_pinned(pcm_host)
    if int(pcm_host.numel()) % 2:
        raise ValueError("pcm: %d int16 values are not interleaved (L, R) pairs" % int(pcm_host.numel()))
    mid, side = _pinned_stereo_levels(pcm_host, frame_len, table, n_edges, staging)
    return _finish(mid, n_edges + 1, non_speech_label, packed, rule, params, gate, (side, c))


def assess_centre(record: CentreRecord, max_rejected_share: Optional[float] = None) -> List[str]:
    """What the centre record says about the file ([] = nothing to report): it is dual mono (no frame has a side level,
    the gate decided nothing), every active frame was rejected, and -- only with a ``max_rejected_share``; the
    calibration ships none -- more than that share of the active frames was dropped.  It reports; it decides nothing."""
    if max_rejected_share is not None and not (isinstance(max_rejected_share, (int, float)) and not isinstance(max_rejected_share, bool)
                                               and 0.0 <= max_rejected_share <= 1.0):
        raise ValueError("max_rejected_share=%r: need a share in [0, 1]" % (max_rejected_share,))
    f, reasons = int(record.flags), []
    if f & _native.VAD_CENTRE_MONO:
        reasons.append("no frame has a side level: the file is dual mono, the centre gate decides nothing")
    if f & _native.VAD_CENTRE_ALL_REJECTED:
        reasons.append("all %d active frames stand less than %d bins above their side level" % (record.n_active, record.min_contrast_bins))
    elif max_rejected_share is not None and record.n_active > 0:
        share = (record.n_active - record.n_kept) / float(record.n_active)
        if share > max_rejected_share:
            reasons.append("%.2f of the active frames rejected by the centre gate (limit %.2f)" % (share, max_rejected_share))
    return reasons
