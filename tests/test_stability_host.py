"""Host side of the half-sample stability test (ffsubsync_amd.stability): every ValueError before any native
call, the exports and the record against the header, the library's own refusals, the wording of the reasons and the
calibration rule recomputed from the committed JSON.  No device."""
import json
import os
import re

import numpy as np
import pytest

import stability_model as stm
import surrogate_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ffsubsync_amd.h")
CALIBRATION = os.path.join(ROOT, "profiles", "stability_calibration.json")


def test_exports_and_record_against_the_header():
    from ffsubsync_amd import _native, stability

    text = open(HEADER).read()
    lib = _native.load()
    for name in ("ffs_subsample_lists", "ffs_offset_stats"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name)
        decl = re.search(r"int %s\(([^;]*)\);" % name, text).group(1)
        assert "plan" not in decl  # stateless: not one of the side plans' batch exports
    args = lambda name: [" ".join(a.split()[:-1]).replace("const ", "")
                         for a in re.search(r"int %s\(([^;]*)\);" % name, text).group(1).split(",")]
    assert args("ffs_offset_stats") == ["ffs_cand_result*", "int", "int", "int64_t", "ffs_stability_result*", "void*"]
    assert args("ffs_subsample_lists") == args("ffs_surrogate_lists")  # the same argument shapes
    body = re.search(r"typedef struct ffs_stability_result \{(.*?)\} ffs_stability_result;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(double|int32_t|int64_t)\s+([^;]+);", body):
        fields += [(n.strip(), {"double": "<f8", "int32_t": "<i4", "int64_t": "<i8"}[ctype]) for n in names.split(",")]
    dt = _native.STABILITY_RESULT_DTYPE
    assert [(n, dt.fields[n][0].str) for n in dt.names] == fields
    assert [n for n in dt.names if n != "reserved"] == list(stm.FIELDS)
    assert all(dt.fields[n][1] % dt.fields[n][0].itemsize == 0 for n in dt.names)  # no field off its natural alignment
    size = int(re.search(r"sizeof\(ffs_stability_result\) == (\d+)", text).group(1))
    assert size == dt.itemsize == _native.STABILITY_RESULT_BYTES and size % 8 == 0
    csrc = open(os.path.join(ROOT, "ffsubsync_amd", "csrc", "ffs_stability.h")).read()
    assert "static_assert(sizeof(StabilityResult) == %d" % size in csrc
    for name, value in [("EMPTY", _native.STAB_EMPTY), ("AMBIGUOUS", _native.STAB_AMBIGUOUS), ("NO_PAIRS", _native.STAB_NO_PAIRS)]:
        assert int(re.search(r"#define FFS_STAB_%s (\d+)" % name, text).group(1)) == value == getattr(stm, name)
    for name, value in [("ODD", _native.SUB_BAD_ODD), ("TRUNCATED", _native.SUB_BAD_TRUNCATED), ("BOUND", _native.SUB_BAD_BOUND)]:
        assert int(re.search(r"#define FFS_SUB_BAD_%s (\d+)" % name, text).group(1)) == value == getattr(stm, "BAD_" + name)
        assert value == int(re.search(r"#define FFS_SURR_BAD_%s (\d+)" % name, text).group(1))  # the surrogate's values
    assert int(re.search(r"#define FFS_STAB_MAX_K (\d+)", text).group(1)) == _native.STAB_MAX_K == stm.MAX_K == stability.MAX_SUBSAMPLES
    assert int(re.search(r"#define FFS_STAB_MAX_BLOCK_RUNS (\d+)", text).group(1)) == _native.STAB_MAX_BLOCK_RUNS == stm.MAX_BLOCK_RUNS == 1 << 24
    assert stability.MAX_BLOCK_RUNS == 1 << 24 and stability.MIN_BLOCKS == stm.MIN_BLOCKS == 8


def test_the_library_refuses_bad_arguments_without_a_device():
    """The ABI's own argument checks come before anything touches the device."""
    from ffsubsync_amd import _native

    lib = _native.load()
    one = np.zeros(1, np.int64)
    tab = [one.ctypes.data] * 5

    def lists(*args):
        rc = lib.ffs_subsample_lists(*args)
        if rc:
            assert lib.ffs_last_error().decode().startswith("ffs_subsample_lists: "), lib.ffs_last_error()
        return rc

    for k, b in ((0, 1), (4097, 1), (-1, 1), (1, 0), (1, (1 << 24) + 1), (1, -3)):
        assert lists(*tab, 1, k, b, 8, 64, 8, None) == -1, (k, b)
    assert lists(None, None, None, None, None, -1, 1, 1, None, 0, None, None) == -1  # a negative count
    assert lists(*tab, 1, 1, 1, 8, -64, 8, None) == -1
    assert lists(None, None, None, None, None, 1, 1, 1, 8, 64, 8, None) == -1  # null tables
    assert lists(*tab, 1, 1, 1, None, 64, 8, None) == -1 and lists(*tab, 1, 1, 1, 8, 64, None, None) == -1  # null pointers
    assert lists(*tab, 1, 1, 1, 12, 64, 8, None) == -1 and lists(*tab, 1, 1, 1, 8, 64, 6, None) == -1  # misaligned
    assert lists(*tab, 1 << 30, 2, 1, 8, 64, 8, None) == -1  # n_vec * K >= 2^31
    assert "2^31" in lib.ffs_last_error().decode()
    ptr, bound, seed = np.array([4096], np.uint64), np.array([4], np.int32), np.array([1], np.uint32)

    def vec(ptr=ptr, bound=bound, off=(8,), cap=(5,), k=2, nbytes=8 + 2 * 56):
        off, cap = np.array(off, np.int64), np.array(cap, np.int64)
        return lists(ptr.ctypes.data, bound.ctypes.data, seed.ctypes.data, off.ctypes.data, cap.ctypes.data, 1, k, 1, 8, nbytes, 8, None)

    for kw in (dict(ptr=np.array([0], np.uint64)), dict(ptr=np.array([4100], np.uint64)), dict(bound=np.array([-1], np.int32)),
               dict(off=(12,)), dict(off=(-8,)), dict(cap=(4,)), dict(cap=(1 << 28,), nbytes=1 << 40), dict(nbytes=8 + 2 * 56 - 8),
               dict(off=(16,))):
        assert vec(**kw) == -1, kw
    assert lists(None, None, None, None, None, 0, 1, 1, None, 0, None, None) == 0  # nothing to do
    for args in ((8, -1, 1, 0, 8), (8, 1, 0, 0, 8), (8, 1, 4097, 0, 8), (8, 1, 1, -1, 8), (None, 1, 1, 0, 8), (8, 1, 1, 0, None),
                 (12, 1, 1, 0, 8), (8, 1, 1, 0, 12)):
        assert lib.ffs_offset_stats(*args, None) == -1, args
        assert lib.ffs_last_error().decode().startswith("ffs_offset_stats: ")
    assert lib.ffs_offset_stats(8, 0, 1, 0, 8, None) == 0


def test_shared_pieces_are_the_surrogate_module_s():
    from ffsubsync_amd import stability, surrogate

    assert stability.fmix32 is surrogate.fmix32 and stability.file_seed is surrogate.file_seed
    assert stability._check_lists is surrogate._check_lists and stability._check_seed is surrogate._check_seed
    assert stability._winning_lists is surrogate._winning_lists
    for n in (0, 2, 4, 6, 16, 18, 130):
        for b in (1, 7, 64):
            assert stability.n_blocks(n, b) == stm.n_blocks(n, b)
    assert stability.n_blocks(18, 8) == 2 and stability.n_blocks(2, 8) == 1  # every run is in a block, the last one too


@pytest.mark.parametrize("kwargs,match", [
    (dict(n_subsamples=0), "n_subsamples=0"), (dict(n_subsamples=4097), "n_subsamples=4097"),
    (dict(n_subsamples=1.5), "n_subsamples=1.5"), (dict(block_runs=0), "block_runs=0"),
    (dict(block_runs=(1 << 24) + 1), "block_runs=16777217"), (dict(seeds=[-1]), "one seed in"), (dict(seeds=[1 << 32]), "one seed in"),
    (dict(seeds=[1, 2]), "one seed in"), (dict(list_ptr=[0]), "null or not 8-byte aligned"),
    (dict(list_ptr=[4100]), "null or not 8-byte aligned"), (dict(lens=[0]), "a vector of 0 samples"),
    (dict(n_bound=[-2]), "negative list bound"), (dict(n_bound=[1 << 28]), "above what a list block holds"),
    (dict(n_bound=[4, 4]), "different sizes")])
def test_subsample_lists_refuses_before_any_native_call(kwargs, match):
    from ffsubsync_amd import stability

    args = dict(list_ptr=[4096], n_bound=[10], lens=[100], seeds=[1], n_subsamples=4, block_runs=1)
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        stability.subsample_lists(**args)


@pytest.mark.parametrize("kwargs,match", [
    (dict(max_offset_samples=0), "max_offset_samples=0"), (dict(n_subsamples=0), "n_subsamples=0"),
    (dict(block_runs=-1), "block_runs=-1"), (dict(seed=-1), "seed=-1"), (dict(seed=1 << 32), "seed="),
    (dict(tol=-1), "tol=-1"), (dict(tol=1.5), "tol=1.5"),
    (dict(budget_bytes=0), "budget_bytes=0"), (dict(ref_ptr=[4096, 4096]), "different sizes"),
    (dict(ref_ptr=[4096, 8192], ref_len=[5, 5], ref_bound=[4, 4]), "2 references for 1 subtitle lists"),
    (dict(sub_bound=[1 << 28]), "above what a list block holds"), (dict(ref_bound=[32768]), "too dense for a list"),
    (dict(sub_hi=[float("nan")]), "one finite level"), (dict(sub_hi=[1.0, 1.0]), "one finite level"),
    (dict(seeds=[1, 2]), "one seed in"), (dict(sub_ptr=[4097]), "not 8-byte aligned"), (dict(sub_len=[0]), "0 samples")])
def test_stability_test_lists_refuses_before_any_native_call(kwargs, match):
    from ffsubsync_amd import stability

    args = dict(ref_ptr=[4096], ref_len=[100], ref_bound=[10], sub_ptr=[8192], sub_len=[90], sub_bound=[10], max_offset_samples=50)
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        stability.stability_test_lists(**args)


def test_offset_stats_refuses_before_any_native_call():
    from ffsubsync_amd import stability

    for n_files, k, tol, match in ((1, 0, 0, "n_subsamples=0"), (1, 4097, 0, "n_subsamples=4097"), (-1, 4, 0, "n_files=-1"),
                                   (1.5, 4, 0, "n_files=1.5"), (1, 4, -1, "tol=-1"), (1, 4, 0.5, "tol=0.5")):
        with pytest.raises(ValueError, match=match):
            stability.offset_stats(None, n_files, k, tol)


def test_stable_sync_refuses_by_name_before_any_device_work():
    from ffsubsync_amd import stability
    from workloads import synth

    track = synth.make_subtitle_records(3, duration_s=120.0)
    ref = (np.arange(12000) % 700 < 300).astype(np.float64)
    ok = [(ref, track)]
    with pytest.raises(ValueError, match="stable_sync needs start_seconds <= 0"):
        stability.stable_sync(ok, start_seconds=1.0)
    levels = ref.copy()
    levels[::3] *= 0.4
    with pytest.raises(ValueError, match="stable_sync needs a two-level reference: a multi-level float reference"):
        stability.stable_sync([(levels, track)])
    dense = np.zeros(40000)
    dense[1:32768:2] = 1.0
    with pytest.raises(ValueError, match="stable_sync: a reference has 32768 or more run boundaries: too dense"):
        stability.stable_sync([(dense, track)])
    for kwargs, match in ((dict(n_subsamples=0), "n_subsamples=0"), (dict(block_runs=0), "block_runs=0"), (dict(seed=-3), "seed=-3"),
                          (dict(tol=-2), "tol=-2"), (dict(min_share=float("nan")), "min_share="), (dict(min_share=1.5), "min_share=1.5"),
                          (dict(ratios=[]), "ratios="), (dict(ratios=[0.0]), "ratios="), (dict(max_offset_seconds=0), "max_offset_seconds=0")):
        with pytest.raises(ValueError, match=match):
            stability.stable_sync(ok, **kwargs)
    with pytest.raises(ValueError, match="cannot align empty speech data"):
        stability.stable_sync([(ref, (np.zeros(0, np.int64), np.zeros(0, np.int64), None))])
    assert stability.stable_sync([]) == []


def _record(scores, offsets, tol, flags=None):
    from ffsubsync_amd import stability

    rec = stm.offset_stats(scores, offsets, np.zeros(len(scores), np.int32) if flags is None else flags, tol)
    return rec, stability.StabilityRecord(**rec)


def test_verdict_and_wording():
    from ffsubsync_amd import _native, stability

    offsets = [100] + [100, 101, 99, 100] * 5 + [3000, -2500, 100, 100]  # 24 half-samples, two of them elsewhere
    rec, record = _record([50.0] + [30.0] * 24, offsets, 2)
    assert stability.share_within(record) == stm.share_within(rec) == 22 / 24
    assert stability.stable(record, 0.9) is True and stm.stable(rec, 0.9) and stability.assess(record, 40, 0.9) == [] == stm.reasons(rec, 40, 0.9)
    assert stability.stable(record, 0.95) is False and not stm.stable(rec, 0.95)
    want = ["22 of 24 half-samples within 2 samples of the offset (share 0.92 < 0.95; 90 % interval [99, 101])"]
    assert (record.off_lo, record.off_hi) == (99, 101) and (record.off_min, record.off_max) == (-2500, 3000)
    # ((c - 1) // 20 = 1: one offset is cut at either end of the interval, the extremes keep them)
    assert stability.assess(record, 40, 0.95) == want == stm.reasons(rec, 40, 0.95)
    assert stability.assess(record, 7, 0.95) == want + ["too few cues to resample (7 blocks < 8)"] == stm.reasons(rec, 7, 0.95)
    # no min_share: no verdict, the warnings alone
    assert stability.stable(record) is None and stability.assess(record, 40) == []
    assert stability.assess(record, 3) == ["too few cues to resample (3 blocks < 8)"]
    # an EMPTY record is never stable
    rec, record = _record([-np.inf, 5.0, 6.0], [0, 4, 4], 100, flags=np.array([1, 0, 0], np.int32))
    assert record.flags == stm.EMPTY and stability.stable(record, 0.0) is False and not stm.stable(rec, 0.0)
    assert stability.assess(record, 40, 0.5) == ["empty record (no usable half-sample solve)"] == stm.reasons(rec, 40, 0.5)
    assert stability.assess(record, 40) == ["empty record (no usable half-sample solve)"]
    row = np.zeros(1, _native.STABILITY_RESULT_DTYPE)
    for i, name in enumerate(stm.FIELDS):
        row[name] = i + 1
    got = stability.record_of(row[0])
    assert [getattr(got, name) for name in stm.FIELDS] == list(range(1, len(stm.FIELDS) + 1))
    assert isinstance(got.real_score, float) and isinstance(got.pair_score_min, float) and isinstance(got.tol, int)


def test_the_defaults_follow_the_rule_from_the_committed_calibration():
    """DEFAULT_TOL = twice the largest matched max_dev over every cell; DEFAULT_MIN_SHARE = the midpoint between the
    smallest matched and the largest wrong share at that tol if they separate, else no verdict is shipped."""
    from ffsubsync_amd import stability

    cal = json.load(open(CALIBRATION))
    files = cal["files"]
    assert cal["seeds"] == 32 and cal["durations"] == [600.0, 3600.0] and cal["block_runs"] == [1, 8] and cal["n_subsamples"] == 64
    assert len(files) == 2 * 2 * 32 * 2 and {(f["duration"], f["block_runs"], f["kind"]) for f in files} == {
        (d, b, k) for d in (600.0, 3600.0) for b in (1, 8) for k in ("matched", "wrong")}
    assert all(f["n_sub"] == 64 == len(f["devs"]) and f["max_dev"] == f["devs"][-1] and f["flags"] == 0 for f in files)
    matched = [f for f in files if f["kind"] == "matched"]
    wrong = [f for f in files if f["kind"] == "wrong"]
    tol = 2 * max(f["max_dev"] for f in matched)
    share = lambda f: sum(1 for d in f["devs"] if d <= tol) / f["n_sub"]
    lo, hi = min(share(f) for f in matched), max(share(f) for f in wrong)
    assert stability.DEFAULT_TOL == tol == cal["shipped"]["tol"]
    assert cal["shipped"]["separate"] == (lo > hi)
    if lo > hi:
        assert stability.DEFAULT_MIN_SHARE == round((lo + hi) / 2.0, 2) == cal["shipped"]["min_share"]
    else:
        assert stability.DEFAULT_MIN_SHARE is None and cal["shipped"]["min_share"] is None
    # what the docs quote beside the rule: the interval separates the classes in every cell
    assert max(f["off_hi"] - f["off_lo"] for f in matched) == 5 and min(f["off_hi"] - f["off_lo"] for f in wrong) == 5203
    # and the arguments of tests/stability_cases.py: the block_runs = 1 cells alone
    import stability_cases as sc

    assert sc.TOL == 2 * max(f["max_dev"] for f in matched if f["block_runs"] == 1)


PARENT_SIGNATURES = {
    "surrogate.surrogate_lists": "(list_ptr, n_bound, lens, seeds, n_surrogates: int = 64, block_units: int = 1)",
    "surrogate.null_stats": "(table, n_files: int, n_surrogates: int, raw: bool = False)",
    "surrogate.null_test_lists": "(ref_ptr, ref_len, ref_bound, sub_ptr, sub_len, sub_bound, max_offset_samples: int, "
                                 "n_surrogates: int = 64, block_units: int = 1, seed: int = 0, ref_lo=None, ref_hi=None, "
                                 "sub_lo=None, sub_hi=None, seeds=None, budget_bytes: int = 2147483648, raw: bool = False) "
                                 "-> ffsubsync_amd.surrogate.NullTest",
    "surrogate.null_sync": "(problems, max_offset_seconds: float = 60, ratios: Optional[Sequence[float]] = None, "
                           "n_surrogates: int = 64, block_units: int = 1, seed: int = 0, min_z: float = 6.7, "
                           "sample_rate: int = 100, start_seconds: float = 0) -> List[ffsubsync_amd.surrogate.NullSyncResult]",
    "stability.subsample_lists": "(list_ptr, n_bound, lens, seeds, n_subsamples: int = 64, block_runs: int = 1, raw: bool = False)",
    "stability.offset_stats": "(table, n_files: int, n_subsamples: int, tol: int = 16364, raw: bool = False)",
    "stability.stability_test_lists": "(ref_ptr, ref_len, ref_bound, sub_ptr, sub_len, sub_bound, max_offset_samples: int, "
                                      "n_subsamples: int = 64, block_runs: int = 1, seed: int = 0, tol: int = 16364, ref_lo=None, "
                                      "ref_hi=None, sub_lo=None, sub_hi=None, seeds=None, budget_bytes: int = 2147483648, "
                                      "raw: bool = False) -> ffsubsync_amd.stability.StabilityTest",
    "stability.stable_sync": "(problems, max_offset_seconds: float = 60, ratios: Optional[Sequence[float]] = None, "
                             "n_subsamples: int = 64, block_runs: int = 1, seed: int = 0, tol: int = 16364, "
                             "min_share: Optional[float] = None, sample_rate: int = 100, start_seconds: float = 0) "
                             "-> List[ffsubsync_amd.stability.StableSyncResult]",
}


def test_both_modules_go_through_the_one_resampling_core(monkeypatch):
    """``surrogate`` and ``stability`` are callers of ``resample_call``: their ``*_lists``, ``*_test_lists`` and
    ``_careful`` reach its one ``list_blocks``, ``test_lists`` and ``_careful`` with what is their own as arguments; the
    names that callers, profiles and tests use still resolve; the eight entry points keep their signatures."""
    import functools
    import inspect

    import ffsubsync_amd
    from ffsubsync_amd import _native, resample_call, stability, surrogate

    for mod in (surrogate, stability):
        assert mod.list_blocks is resample_call.list_blocks and mod.test_lists is resample_call.test_lists
        assert isinstance(mod._careful, functools.partial) and mod._careful.func is resample_call._careful
        for name in ("fmix32", "file_seed", "_check_seed", "_check_lists", "_list_vector", "_winning_lists", "CHUNK_BUDGET",
                     "CHUNK_CAP"):
            assert getattr(mod, name) is getattr(resample_call, name), name
        for name in ("MAX_BOUND", "MIN_BLOCKS", "n_blocks", "record_of", "assess", "_check_sync", "_KIND"):
            assert hasattr(mod, name), name
        assert not hasattr(mod, "_levels") and not hasattr(mod, "pairs_for_budget")  # (once, in the core)
    for name in ("_speech_cues", "_host_boundaries", "_check_shuffle", "derive", "trusted", "MAX_SURROGATES", "MAX_UNITS",
                 "DEFAULT_MIN_Z", "DEFAULT_SURROGATES"):
        assert hasattr(surrogate, name), name
    for name in ("_check_resample", "_check_tol", "share_within", "stable", "MAX_SUBSAMPLES", "MAX_BLOCK_RUNS", "DEFAULT_TOL",
                 "DEFAULT_MIN_SHARE", "DEFAULT_SUBSAMPLES"):
        assert hasattr(stability, name), name
    # the list makers that the careful redo and the chunk loop call are the modules' own entry points
    assert surrogate._careful.args == (surrogate.surrogate_lists,) and surrogate._KIND.make_lists is surrogate.surrogate_lists
    raw_lists = stability._KIND.make_lists
    assert stability._careful.args == (raw_lists,) and raw_lists.func is stability.subsample_lists and raw_lists.keywords == {"raw": True}
    assert (surrogate._KIND.name, surrogate._KIND.k_name, surrogate._KIND.block_name) == ("null_test_lists", "n_surrogates", "block_units")
    assert (stability._KIND.name, stability._KIND.k_name, stability._KIND.block_name) == ("stability_test_lists", "n_subsamples", "block_runs")
    assert surrogate._KIND.record_dtype is _native.NULL_RESULT_DTYPE and surrogate._KIND.ambiguous == _native.NULL_AMBIGUOUS
    assert stability._KIND.record_dtype is _native.STABILITY_RESULT_DTYPE and stability._KIND.ambiguous == _native.STAB_AMBIGUOUS
    assert surrogate._KIND.max_bound == surrogate.MAX_BOUND and stability._KIND.max_bound == stability.MAX_BOUND

    # the calls themselves: a module's own checks, then the core with the module's pieces
    calls = []

    def spy(result):
        def call(*args):
            calls.append(args)
            return result
        return call

    lists = ([4096], [10], [100], [1])
    monkeypatch.setattr(surrogate, "list_blocks", spy("blocks"))
    assert surrogate.surrogate_lists(*lists, 4, 2) == "blocks"
    assert calls.pop() == ("surrogate_lists", _native.surrogate_lists, surrogate.MAX_BOUND, surrogate._LIMIT_TEXT, *lists, 4, 2)
    monkeypatch.setattr(stability, "list_blocks", spy(("buffer", "offsets", "status")))
    assert stability.subsample_lists(*lists, 4, 2, raw=True) == ("buffer", "offsets", "status")
    assert calls.pop() == ("subsample_lists", _native.subsample_lists, stability.MAX_BOUND, stability._LIMIT_TEXT, *lists, 4, 2)
    files = ([4096], [100], [10], [8192], [90], [10], 50)
    monkeypatch.setattr(surrogate, "test_lists", spy(("records", "table", "status", "seeds", {"n_surrogates": 4})))
    assert surrogate.null_test_lists(*files, 4, 2, 7) == surrogate.NullTest("records", "table", "status", "seeds", {"n_surrogates": 4})
    assert calls.pop() == (surrogate._KIND, _native.null_stats, *files, 4, 2, 7, None, None, None, None, None,
                           resample_call.CHUNK_BUDGET, False)
    monkeypatch.setattr(stability, "test_lists", spy(("records", "table", "status", "seeds", {"n_subsamples": 4})))
    got = stability.stability_test_lists(*files, 4, 2, 7, 33, raw=True)
    assert got == stability.StabilityTest("records", "table", "status", "seeds", {"n_subsamples": 4})
    kind, stats_call, *rest = calls.pop()
    assert kind is stability._KIND and stats_call.func is _native.offset_stats and stats_call.keywords == {"tol": 33}
    assert tuple(rest) == (*files, 4, 2, 7, None, None, None, None, None, resample_call.CHUNK_BUDGET, True) and not calls
    with pytest.raises(ValueError, match="n_surrogates=0"):  # (the module's own check comes first)
        surrogate.null_test_lists(*files, 0)
    with pytest.raises(ValueError, match="tol=-1"):
        stability.stability_test_lists(*files, tol=-1)
    assert not calls

    for name, want in PARENT_SIGNATURES.items():
        mod, fn = name.split(".")
        assert str(inspect.signature(getattr(getattr(ffsubsync_amd, mod), fn))).replace("typing.", "") == want, name
