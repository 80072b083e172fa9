"""Seeded workload for the joint cue retiming (ffsubsync_amd.cue_retime): a subtitle file that is synced
correctly as a whole, with stretches of consecutive lines that a re-edit moved together.

Built on ``workloads.cues``: the reference, the track at the true ratio and the "sync" (``cues.true_sync``) are the
same.  On top of the untouched cues: ``n_stretches`` runs of 3-12 consecutive cues are moved in the file by one common
shift in +-[0.8, 2.5] s each, ``n_isolated`` single cues outside the stretches are displaced by their own drawn shift,
and ``n_extra`` cues are added at random places.  The truth per cue is its kind, the stretch it belongs to and its
displacement in output samples: a retiming's delta should be the negative.  The file stays in file order (sorted by
start), as the retiming's chain needs it.
"""
from dataclasses import dataclass

import numpy as np

from ffsubsync_amd.constants import SAMPLE_RATE

from . import synth
from .cues import host_subtitle_vector, true_sync  # noqa: F401  (the sync and the host raster are shared)

UNTOUCHED, STRETCH, ISOLATED, EXTRA = 0, 1, 2, 3
KIND_NAMES = ("untouched", "stretch", "isolated", "extra")


@dataclass
class StretchProblem:
    seed: int
    ref: np.ndarray  # 0/1 uint8 reference at 100 Hz
    start_us: np.ndarray  # the subtitle file, in file order (sorted by start)
    end_us: np.ndarray
    meta: np.ndarray
    ratio: float  # the true framerate ratio
    offset: int  # the true offset (samples)
    kind: np.ndarray  # UNTOUCHED / STRETCH / ISOLATED / EXTRA per cue
    stretch: np.ndarray  # per cue the stretch it belongs to, -1 outside
    displacement: np.ndarray  # per cue, output samples (0 unless STRETCH or ISOLATED)

    @property
    def problem(self):
        """(reference, track) as the syncs take it."""
        return self.ref.astype(np.float64), (self.start_us, self.end_us, self.meta)


def _shift_ms(rng, n):
    sign = np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    return np.rint(sign * rng.uniform(0.8, 2.5, n) * 1e3).astype(np.int64)


def make_stretch_problem(seed: int, duration_s: float = 7200.0, n_stretches: int = 8, n_isolated: int = 16,
                         n_extra: int = 16, sample_rate: int = SAMPLE_RATE) -> StretchProblem:
    spec = synth.make_pair_spec(seed, duration_s, sample_rate=sample_rate)
    rng = np.random.RandomState(seed + 5550123)
    k = spec.true_ratio_index
    ratio = spec.ratios[k]
    ref = synth.rasterize(spec.ref_len, spec.ref_starts, spec.ref_ends)
    st, en = spec.cand_starts[k].astype(np.float64), spec.cand_ends[k].astype(np.float64)
    start_ms = np.rint(st / sample_rate / ratio * 1e3).astype(np.int64)
    end_ms = np.maximum(np.rint(en / sample_rate / ratio * 1e3).astype(np.int64), start_ms + 10)
    n = start_ms.size
    kind, stretch, disp_ms = np.zeros(n, np.int64), np.full(n, -1, np.int64), np.zeros(n, np.int64)
    # stretches: disjoint runs of 3-12 consecutive cues with a gap of at least one cue between two of them
    taken = np.zeros(n + 1, bool)
    for j in range(n_stretches):
        length = int(rng.randint(3, 13))
        for _ in range(50):
            first = int(rng.randint(0, max(n - length, 1)))
            lo, hi = max(first - 1, 0), min(first + length + 1, n)
            if first + length <= n and not taken[lo:hi].any():
                taken[first:first + length] = True
                kind[first:first + length], stretch[first:first + length] = STRETCH, j
                disp_ms[first:first + length] = _shift_ms(rng, 1)[0]
                break
    free = np.flatnonzero(kind == UNTOUCHED)
    alone = rng.choice(free, size=min(n_isolated, free.size), replace=False)
    kind[alone] = ISOLATED
    disp_ms[alone] = _shift_ms(rng, alone.size)
    disp_ms = np.maximum(disp_ms, -start_ms)  # stamps stay >= 0
    start_ms, end_ms = start_ms + disp_ms, end_ms + disp_ms
    file_ms = int(end_ms.max()) if n else int(duration_s * 1e3)
    x_start = np.rint(rng.uniform(0.0, max(file_ms - 4000, 1), n_extra)).astype(np.int64)
    x_end = x_start + np.rint(rng.uniform(0.5, 4.0, n_extra) * 1e3).astype(np.int64)
    start_ms, end_ms = np.concatenate([start_ms, x_start]), np.concatenate([end_ms, x_end])
    kind = np.concatenate([kind, np.full(n_extra, EXTRA, np.int64)])
    stretch = np.concatenate([stretch, np.full(n_extra, -1, np.int64)])
    disp_ms = np.concatenate([disp_ms, np.zeros(n_extra, np.int64)])
    order = np.argsort(start_ms, kind="stable")
    start_ms, end_ms, kind, stretch, disp_ms = start_ms[order], end_ms[order], kind[order], stretch[order], disp_ms[order]
    displacement = np.rint(disp_ms / 1e3 * ratio * sample_rate).astype(np.int64)
    return StretchProblem(seed, ref, start_ms * 1000, end_ms * 1000, np.zeros(start_ms.size, np.uint8), float(ratio),
                          int(spec.true_offset_samples), kind, stretch, displacement)
