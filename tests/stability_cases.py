"""The half-sample test's answers of the model on the shared problems of tests/surrogate_cases.py (seeds 0-5 at 10 min,
matched then wrong), computed once per process and shared between tests/test_stability_model_host.py and
tests/test_gpu_stability.py (a model run of one 10-minute file is 7 + 65 exact solves).

TOL and MIN_SHARE are the tests' own arguments, not shipped defaults (the calibration ships no verdict):
TOL = twice the largest matched max_dev of the block_runs = 1 cells of profiles/stability_calibration.json (4 samples),
MIN_SHARE = one half."""
import functools

import stability_model as stm
import surrogate_cases as cases

TOL = 8
MIN_SHARE = 0.5


@functools.lru_cache(maxsize=None)
def model_sync(index, block_runs=1):
    """``stability_model.stable_sync`` of problem ``index`` of ``cases.sync_problems()`` as file ``index`` of a call with
    ``cases.SEED``."""
    ref, tr = cases.sync_problems()[index]
    return stm.stable_sync(ref, tr, cases.W, None, cases.K, block_runs, cases.SEED, index, TOL, MIN_SHARE)
