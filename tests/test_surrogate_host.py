"""Host side of the shuffled-cue significance test (ffsubsync_amd.surrogate): every ValueError before any
native call, the exports and the record against the header, the derived figures and the wording of the reasons.  No
device."""
import math
import os
import re

import numpy as np
import pytest

import surrogate_model as sm

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ffsubsync_amd.h")


def test_exports_and_record_against_the_header():
    from ffsubsync_amd import _native, surrogate

    text = open(HEADER).read()
    lib = _native.load()
    for name in ("ffs_surrogate_lists", "ffs_null_stats"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name)
        decl = re.search(r"int %s\(([^;]*)\);" % name, text).group(1)
        assert "plan" not in decl  # stateless: not one of the side plans' batch exports
    decl = re.search(r"int ffs_null_stats\(([^;]*)\);", text).group(1)
    assert [" ".join(a.split()[:-1]).replace("const ", "") for a in decl.split(",")] == [
        "ffs_cand_result*", "int", "int", "ffs_null_result*", "void*"]
    decl = re.search(r"int ffs_surrogate_lists\(([^;]*)\);", text).group(1)
    assert [" ".join(a.split()[:-1]).replace("const ", "") for a in decl.split(",")] == [
        "void* const*", "int32_t*", "uint32_t*", "int64_t*", "int64_t*", "int64_t", "int", "int", "void*", "int64_t",
        "int32_t*", "void*"]
    body = re.search(r"typedef struct ffs_null_result \{(.*?)\} ffs_null_result;", text, re.S).group(1)
    fields = []
    for ctype, names in re.findall(r"(double|int32_t)\s+([^;]+);", body):
        fields += [(n.strip(), "<f8" if ctype == "double" else "<i4") for n in names.split(",")]
    dt = _native.NULL_RESULT_DTYPE
    assert [(n, dt.fields[n][0].str) for n in dt.names] == fields
    assert int(re.search(r"sizeof\(ffs_null_result\) == (\d+)", text).group(1)) == dt.itemsize == _native.NULL_RESULT_BYTES
    for name, value in [("FLAT", _native.NULL_FLAT), ("EMPTY", _native.NULL_EMPTY), ("AMBIGUOUS", _native.NULL_AMBIGUOUS)]:
        assert int(re.search(r"#define FFS_NULL_%s (\d+)" % name, text).group(1)) == value == getattr(sm, name)
    for name, value in [("ODD", _native.SURR_BAD_ODD), ("TRUNCATED", _native.SURR_BAD_TRUNCATED),
                        ("BOUND", _native.SURR_BAD_BOUND), ("UNITS", _native.SURR_BAD_UNITS)]:
        assert int(re.search(r"#define FFS_SURR_BAD_%s (\d+)" % name, text).group(1)) == value == getattr(sm, "BAD_" + name)
    assert int(re.search(r"#define FFS_SURR_MAX_UNITS (\d+)", text).group(1)) == _native.SURR_MAX_UNITS == sm.MAX_UNITS == surrogate.MAX_UNITS
    assert int(re.search(r"#define FFS_SURR_MAX_K (\d+)", text).group(1)) == _native.SURR_MAX_K == sm.MAX_K == surrogate.MAX_SURROGATES
    assert surrogate.MAX_BOUND == 16386 and surrogate.MIN_BLOCKS == sm.MIN_BLOCKS


def test_the_library_refuses_bad_arguments_without_a_device():
    """The ABI's own argument checks come before anything touches the device."""
    from ffsubsync_amd import _native

    lib = _native.load()
    one = np.zeros(1, np.int64)
    for k, b in ((0, 1), (4097, 1), (1, 0), (1, 8193)):
        assert lib.ffs_surrogate_lists(one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data,
                                       1, k, b, 8, 64, 8, None) == -1
        assert lib.ffs_last_error().decode().startswith("ffs_surrogate_lists: ")
    assert lib.ffs_surrogate_lists(None, None, None, None, None, -1, 1, 1, None, 0, None, None) == -1
    assert lib.ffs_surrogate_lists(None, None, None, None, None, 1, 1, 1, 8, 64, 8, None) == -1
    assert lib.ffs_surrogate_lists(None, None, None, None, None, 0, 1, 1, None, 0, None, None) == 0
    for args in ((8, -1, 1, 8), (8, 1, 0, 8), (8, 1, 4097, 8), (None, 1, 1, 8), (8, 1, 1, None), (12, 1, 1, 8)):
        assert lib.ffs_null_stats(*args, None) == -1
        assert lib.ffs_last_error().decode().startswith("ffs_null_stats: ")
    assert lib.ffs_null_stats(8, 0, 1, 8, None) == 0


def test_hash_and_blocks_equal_the_model():
    from ffsubsync_amd import surrogate

    for h in (0, 1, 0xFFFFFFFF, 123456789):
        assert surrogate.fmix32(h) == sm.fmix32(h)
    assert [surrogate.file_seed(7, i) for i in range(5)] == [sm.file_seed(7, i) for i in range(5)]
    assert surrogate.file_seed(0xFFFFFFFF, 1) == sm.fmix32(0)
    for n in (0, 2, 4, 6, 16, 18, 130):
        for b in (1, 7, 64):
            assert surrogate.n_blocks(n, b) == sm.n_blocks(n, b)


@pytest.mark.parametrize("kwargs,match", [
    (dict(n_surrogates=0), "n_surrogates=0"), (dict(n_surrogates=4097), "n_surrogates=4097"),
    (dict(n_surrogates=1.5), "n_surrogates=1.5"), (dict(block_units=0), "block_units=0"),
    (dict(block_units=8193), "block_units=8193"), (dict(seeds=[-1]), "one seed in"), (dict(seeds=[1 << 32]), "one seed in"),
    (dict(seeds=[1, 2]), "one seed in"), (dict(list_ptr=[0]), "null or not 8-byte aligned"),
    (dict(list_ptr=[4100]), "null or not 8-byte aligned"), (dict(lens=[0]), "a vector of 0 samples"),
    (dict(n_bound=[-2]), "negative list bound"), (dict(n_bound=[16388]), "above the unit limit"),
    (dict(n_bound=[4, 4]), "different sizes")])
def test_surrogate_lists_refuses_before_any_native_call(kwargs, match):
    from ffsubsync_amd import surrogate

    args = dict(list_ptr=[4096], n_bound=[10], lens=[100], seeds=[1], n_surrogates=4, block_units=1)
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        surrogate.surrogate_lists(**args)


@pytest.mark.parametrize("kwargs,match", [
    (dict(max_offset_samples=0), "max_offset_samples=0"), (dict(n_surrogates=0), "n_surrogates=0"),
    (dict(block_units=-1), "block_units=-1"), (dict(seed=-1), "seed=-1"), (dict(seed=1 << 32), "seed="),
    (dict(budget_bytes=0), "budget_bytes=0"), (dict(ref_ptr=[4096, 4096]), "different sizes"),
    (dict(ref_ptr=[4096, 8192], ref_len=[5, 5], ref_bound=[4, 4]), "2 references for 1 subtitle lists"),
    (dict(sub_bound=[16388]), "above the unit limit"), (dict(ref_bound=[32768]), "too dense for a list"),
    (dict(sub_hi=[float("nan")]), "one finite level"), (dict(sub_hi=[1.0, 1.0]), "one finite level"),
    (dict(seeds=[1, 2]), "one seed in"), (dict(sub_ptr=[4097]), "not 8-byte aligned"), (dict(sub_len=[0]), "0 samples")])
def test_null_test_lists_refuses_before_any_native_call(kwargs, match):
    from ffsubsync_amd import surrogate

    args = dict(ref_ptr=[4096], ref_len=[100], ref_bound=[10], sub_ptr=[8192], sub_len=[90], sub_bound=[10], max_offset_samples=50)
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        surrogate.null_test_lists(**args)


def test_null_stats_refuses_before_any_native_call():
    from ffsubsync_amd import surrogate

    for n_files, k, match in ((1, 0, "n_surrogates=0"), (1, 4097, "n_surrogates=4097"), (-1, 4, "n_files=-1"), (1.5, 4, "n_files=1.5")):
        with pytest.raises(ValueError, match=match):
            surrogate.null_stats(None, n_files, k)


def test_null_sync_refuses_by_name_before_any_device_work():
    from ffsubsync_amd import surrogate
    from workloads import synth

    track = synth.make_subtitle_records(3, duration_s=120.0)
    ref = (np.arange(12000) % 700 < 300).astype(np.float64)
    ok = [(ref, track)]
    with pytest.raises(ValueError, match="start_seconds <= 0"):
        surrogate.null_sync(ok, start_seconds=1.0)
    levels = ref.copy()
    levels[::3] *= 0.4
    with pytest.raises(ValueError, match="multi-level float reference"):
        surrogate.null_sync([(levels, track)])
    many = (np.arange(8194) * 1000000, np.arange(8194) * 1000000 + 400000, np.zeros(8194, np.uint8))
    with pytest.raises(ValueError, match="track 0 has 8194 cues that are not metadata: above the unit limit"):
        surrogate.null_sync([(ref, many)])
    meta = np.zeros(8194, np.uint8)
    meta[5] = 1  # a cue the rasteriser skips does not count
    assert surrogate._speech_cues((many[0], many[1], meta)) == 8193 == surrogate.MAX_UNITS + 1
    assert surrogate._speech_cues((many[0], many[1], None)) == 8194
    # a host reference too dense for a list is counted on the host: runs of one sample, two boundaries each
    from ffsubsync_amd.aligners import _Vec

    dense = np.zeros(40000)
    dense[1:32768:2] = 1.0
    assert surrogate._host_boundaries(_Vec(dense)) == 32768 and surrogate._host_boundaries(_Vec(ref)) == 2 * 18
    with pytest.raises(ValueError, match="a reference has 32768 or more run boundaries: too dense"):
        surrogate.null_sync([(dense, track)])
    for kwargs, match in ((dict(n_surrogates=0), "n_surrogates=0"), (dict(block_units=0), "block_units=0"),
                          (dict(seed=-3), "seed=-3"), (dict(min_z=float("nan")), "min_z="), (dict(ratios=[]), "ratios="),
                          (dict(ratios=[0.0]), "ratios="), (dict(max_offset_seconds=0), "max_offset_seconds=0")):
        with pytest.raises(ValueError, match=match):
            surrogate.null_sync(ok, **kwargs)
    with pytest.raises(ValueError, match="cannot align empty speech data"):
        surrogate.null_sync([(ref, (np.zeros(0, np.int64), np.zeros(0, np.int64), None))])
    assert surrogate.null_sync([]) == []


def _record(real, nulls, flags=None):
    from ffsubsync_amd import surrogate

    sc = np.array([real] + list(nulls), np.float64)
    rec = sm.stats(sc, np.zeros(sc.size, np.int32) if flags is None else np.asarray(flags))
    return rec, surrogate.NullRecord(**rec)


def test_derived_figures_verdict_and_wording():
    from ffsubsync_amd import surrogate

    assert surrogate.DEFAULT_MIN_Z == 6.7 and surrogate.DEFAULT_SURROGATES == 64
    rec, null = _record(100.0, [10.0, 12.0, 8.0, 10.0])
    z, p = surrogate.derive(null)
    assert (z, p) == sm.z_p(rec) and p == 0.2 and math.isclose(z, 90.0 / math.sqrt(2.0))
    assert surrogate.trusted(null) and surrogate.assess(null, 40) == [] == sm.reasons(rec, 40, surrogate.DEFAULT_MIN_Z)
    assert surrogate.assess(null, 7) == ["too few cues to shuffle (7 blocks < 8)"] == sm.reasons(rec, 7, 6.7)
    assert surrogate.trusted(null) == sm.trusted(rec, 6.7)
    # a null that reached the score, and a z below the threshold
    rec, null = _record(11.0, [10.0, 12.0, 8.0, 11.0])
    assert not surrogate.trusted(null)
    assert surrogate.assess(null, 40) == ["2 of 4 nulls reached the score (p = 0.600)", "z 0.5 < 6.7"] == sm.reasons(rec, 40, 6.7)
    rec, null = _record(14.0, [10.0, 12.0, 8.0, 10.0])
    assert surrogate.assess(null, 40, min_z=3.0) == ["z 2.8 < 3.0"] == sm.reasons(rec, 40, 3.0) and not surrogate.trusted(null, 3.0)
    assert surrogate.trusted(null, 2.5) and sm.trusted(rec, 2.5)
    # flat and empty nulls: z = 0
    rec, null = _record(14.0, [10.0, 10.0, 10.0])
    assert surrogate.derive(null) == (0.0, 0.25) and surrogate.assess(null, 40) == ["flat null (std 0)"] == sm.reasons(rec, 40, 6.7)
    assert not surrogate.trusted(null)
    rec, null = _record(14.0, [-np.inf, np.nan])
    assert null.flags == sm.FLAT | sm.EMPTY and surrogate.derive(null) == (0.0, 1.0)
    assert surrogate.assess(null, 40) == ["empty null (no usable surrogate score)"] == sm.reasons(rec, 40, 6.7)
    assert not surrogate.trusted(null, 0.0) and not sm.trusted(rec, 0.0)
    rec, null = _record(-np.inf, [10.0, 12.0], flags=[1, 0, 0])  # an unusable real record
    assert null.flags == sm.EMPTY and not surrogate.trusted(null, -1e9) and surrogate.assess(null, 40)[0].startswith("empty null")
    got = surrogate.record_of(np.array([(1.5, 2.0, 3.0, 1.0, 4.0, 5, 1, 0, 4)], dtype=__import__("ffsubsync_amd")._native.NULL_RESULT_DTYPE)[0])
    assert got == surrogate.NullRecord(1.5, 2.0, 3.0, 1.0, 4.0, 5, 1, 0, 4)
