"""The ratio sweep's test problems and the model's answers on them, computed once per process and shared between
tests/test_ratio_sweep_host.py and tests/test_gpu_ratio_sweep.py (a 10-minute model sweep is ~230 oracle solves)."""
import functools

import sweep_model as sm
from workloads import unknown_ratio as ur

W = 6000
FREE_SEEDS = (1, 5, 7)  # 10-minute `free` problems: true ratios 0.9867, 1.0326, 1.0626
EXTRA_FREE_SEED = 3  # 0.9502
SEVEN_SEED = 102  # 24/25
WRONG_SEED = 200


@functools.lru_cache(maxsize=None)
def problem(kind, seed, duration_s=600.0):
    return ur.make_problem(kind, seed, duration_s)


@functools.lru_cache(maxsize=None)
def model_sweep(kind, seed, duration_s=600.0, tolerance_samples=None):
    """``sweep_model.sweep`` of the problem at the lag window W; ``tolerance_samples`` None = the module's default."""
    from ffsubsync_amd import ratio_sweep

    tol = ratio_sweep.DEFAULT_TOLERANCE if tolerance_samples is None else tolerance_samples
    p = problem(kind, seed, duration_s)
    return sm.sweep(p.reference, p.track, W, tolerance_samples=tol)
