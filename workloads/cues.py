"""Seeded workload for the per-cue evidence report (ffsubsync_amd.cue_report): a subtitle file that is
synced correctly as a whole and wrong in single lines.

Built on ``synth.make_pair_spec``: the reference is the spec's, the track is the true ratio's candidate written back
as a subtitle file with millisecond stamps, and the "sync" applies the true ratio and the true offset to every cue.
``n_moved`` of the cues are displaced in the file by a drawn +-[0.8, 2.5] s (a late or early line), and ``n_extra`` cues
are added at random places (lines the video has no speech for, unless they land on some by chance).  The truth per cue
is its kind and, for a displaced cue, the displacement in output samples: the report's best_delta should be its negative.
"""
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from ffsubsync_amd.constants import SAMPLE_RATE

from . import synth

UNTOUCHED, DISPLACED, EXTRA = 0, 1, 2
KIND_NAMES = ("untouched", "displaced", "extra")


@dataclass
class CueProblem:
    seed: int
    ref: np.ndarray  # 0/1 uint8 reference at 100 Hz
    start_us: np.ndarray  # the subtitle file, in file order (sorted by start)
    end_us: np.ndarray
    meta: np.ndarray
    ratio: float  # the true framerate ratio
    offset: int  # the true offset (samples): t_ref = t_sub * ratio + offset / rate
    kind: np.ndarray  # UNTOUCHED / DISPLACED / EXTRA per cue
    displacement: np.ndarray  # per cue, output samples (0 unless DISPLACED)

    @property
    def problem(self):
        """(reference, track) as the syncs take it."""
        return self.ref.astype(np.float64), (self.start_us, self.end_us, self.meta)


def make_cue_problem(seed: int, duration_s: float = 7200.0, n_moved: int = 40, n_extra: int = 40,
                     sample_rate: int = SAMPLE_RATE) -> CueProblem:
    spec = synth.make_pair_spec(seed, duration_s, sample_rate=sample_rate)
    rng = np.random.RandomState(seed + 918273)
    k = spec.true_ratio_index
    ratio = spec.ratios[k]
    ref = synth.rasterize(spec.ref_len, spec.ref_starts, spec.ref_ends)
    # the true ratio's runs, back in the file's clock, at srt resolution
    st, en = spec.cand_starts[k].astype(np.float64), spec.cand_ends[k].astype(np.float64)
    start_ms = np.rint(st / sample_rate / ratio * 1e3).astype(np.int64)
    end_ms = np.maximum(np.rint(en / sample_rate / ratio * 1e3).astype(np.int64), start_ms + 10)
    n = start_ms.size
    kind = np.zeros(n, np.int64)
    disp_ms = np.zeros(n, np.int64)
    moved = rng.choice(n, size=min(n_moved, n), replace=False)
    sign = np.where(rng.rand(moved.size) < 0.5, -1.0, 1.0)
    disp_ms[moved] = np.rint(sign * rng.uniform(0.8, 2.5, moved.size) * 1e3).astype(np.int64)
    disp_ms[moved] = np.maximum(disp_ms[moved], -start_ms[moved])  # stamps stay >= 0
    kind[moved] = DISPLACED
    start_ms, end_ms = start_ms + disp_ms, end_ms + disp_ms
    # extra cues anywhere in the file
    file_ms = int(end_ms.max()) if n else int(duration_s * 1e3)
    x_start = np.rint(rng.uniform(0.0, max(file_ms - 4000, 1), n_extra)).astype(np.int64)
    x_end = x_start + np.rint(rng.uniform(0.5, 4.0, n_extra) * 1e3).astype(np.int64)
    start_ms = np.concatenate([start_ms, x_start])
    end_ms = np.concatenate([end_ms, x_end])
    kind = np.concatenate([kind, np.full(n_extra, EXTRA, np.int64)])
    disp_ms = np.concatenate([disp_ms, np.zeros(n_extra, np.int64)])
    order = np.argsort(start_ms, kind="stable")
    start_ms, end_ms, kind, disp_ms = start_ms[order], end_ms[order], kind[order], disp_ms[order]
    displacement = np.rint(disp_ms / 1e3 * ratio * sample_rate).astype(np.int64)
    return CueProblem(seed, ref, start_ms * 1000, end_ms * 1000, np.zeros(start_ms.size, np.uint8), float(ratio),
                      int(spec.true_offset_samples), kind, displacement)


def true_sync(pr: CueProblem, sample_rate: int = SAMPLE_RATE):
    """What a correct whole-file sync returns: the true ratio, every cue scaled and shifted by the true offset."""
    from ffsubsync_amd.split_align import _scaled_us

    shift = int(round(pr.offset * 10 ** 6 / float(sample_rate)))
    cs = np.array([_scaled_us(u, pr.ratio) + shift for u in pr.start_us], dtype=np.int64)
    ce = np.array([_scaled_us(u, pr.ratio) + shift for u in pr.end_us], dtype=np.int64)
    return SimpleNamespace(ratio=pr.ratio, cue_start_us=cs, cue_end_us=ce)


def host_subtitle_vector(pr: CueProblem, ratio=None, sample_rate: int = SAMPLE_RATE) -> np.ndarray:
    """The 0/1 subtitle vector of the file at ``ratio`` (the true one by default), by the rasteriser's own interval
    arithmetic (host only)."""
    from ffsubsync_amd import _native

    ratio = pr.ratio if ratio is None else float(ratio)
    n = _native.raster_length(pr.end_us, ratio, sample_rate)
    iv = _native.raster_intervals(pr.start_us, pr.end_us, pr.meta, ratio, sample_rate, 0.0, n)
    return synth.rasterize(n, iv[:, 0].astype(np.int64), iv[:, 1].astype(np.int64))
