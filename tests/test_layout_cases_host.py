"""tests/layout_cases.py itself, on the host: slicing a layout at its offsets gives the samples back, every residue the
header's alignments allow occurs, every byte and bit that is not a sample is poisoned, ``abutting`` has no gaps, the guards
have their size, and the problem sets of tests/test_gpu_layout.py hold the lengths they must."""
import numpy as np
import pytest

import layout_cases as lc

KINDS = {"u1": lc.U1, "u8": lc.U8, "f32": lc.F32, "f64": lc.F64, "runs": lc.RUNS}
LENS = [1, 19, 31, 32, 33, 64, 95, 96, 97, 127, 128, 129, 300, 1000, 1023, 1024, 1025, 2999]


def _vectors(kind, seed=0):
    rng = np.random.RandomState(seed)
    out = []
    for i, n in enumerate(LENS):
        run = [1, 2, 7, 40][i % 4]
        x = np.repeat(rng.rand(n // run + 1) < 0.5, run)[:n].astype(np.uint8)
        if i % 5 == 0:
            x[-1] = 1  # a run that reaches the end
        if kind == lc.F32:
            x = x.astype(np.float32) * np.float32(0.75)
        elif kind == lc.F64:
            x = x * 0.6 + 0.125
        out.append(x)
    return out


def _sample_extent(img, i):
    """[first, end) bytes of vector i that hold samples (for a list block: header and entries up to e[n])."""
    o = int(img.offs[i])
    m = img.mask[o:o + int(img.nbytes[i])]
    return o, o + int(np.flatnonzero(m).max()) + 1


@pytest.mark.parametrize("name", sorted(KINDS))
@pytest.mark.parametrize("layout", lc.LAYOUTS)
def test_round_trip_alignment_and_poison(layout, name):
    kind = KINDS[name]
    vecs = _vectors(kind)
    img = lc.build(vecs, kind, layout)
    fill = 0 if layout == "clean" else 0xFF
    # the samples come back from the image's own offsets
    for i, v in enumerate(vecs):
        got = img.vector(i)
        want = (v != 0).astype(np.uint8) if kind in (lc.U1, lc.U8, lc.RUNS) else v
        assert got.dtype == want.dtype and np.array_equal(got, want), (layout, name, i)
        if kind == lc.U1:
            o = int(img.offs[i])
            assert np.array_equal(np.unpackbits(img.host[o:o + (v.size + 31) // 32 * 4], bitorder="little")[:v.size], want)
    # alignment: never below what the header grants, and the layout's own rule
    assert not (img.offs % lc.ALIGN[kind]).any()
    if layout in ("clean", "poisoned"):
        assert not (img.offs % 64).any()
    if layout == "shifted":
        assert set((img.offs % 64).tolist()) == set(lc.RESIDUES[kind])
    if layout == "abutting":
        assert img.offs[0] % 64 == lc.RESIDUES[kind][0]
        # (one element type: a vector's bytes are a multiple of its alignment, so the next one starts on its last byte's heel)
        assert np.array_equal(img.offs[1:], (img.offs + img.nbytes)[:-1])
    # vectors do not overlap, every bit that is not a sample is poison (zero in the control), sample bits are untouched
    assert (img.offs[1:] >= img.offs[:-1] + img.nbytes[:-1]).all()
    assert np.array_equal(img.host & ~img.mask, np.full(img.host.size, fill, np.uint8) & ~img.mask)
    # guards
    assert img.offs[0] >= lc.GUARD and img.host.size - int(img.offs[-1] + img.nbytes[-1]) >= lc.GUARD
    assert not img.mask[: lc.GUARD].any() and not img.mask[-lc.GUARD:].any()
    assert lc.GUARD == 256 * 1024 > 1024 * 2 * 16


def test_bit_tails_and_list_tails_are_poisoned():
    vecs = _vectors(lc.U1)
    for layout in lc.HOSTILE:
        img = lc.build(vecs, lc.U1, layout)
        for i, v in enumerate(vecs):
            o, n = int(img.offs[i]), v.size
            bits = np.unpackbits(img.host[o:o + int(img.nbytes[i])], bitorder="little")
            assert bits.size == (n + 31) // 32 * 32 and bits[n:].all(), (layout, i)
        img = lc.build(vecs, lc.RUNS, layout)
        for i, v in enumerate(vecs):
            o = int(img.offs[i])
            words = img.host[o:o + int(img.nbytes[i])].view(np.int32)
            n, cap = int(words[0]), int(words[3])
            assert cap == lc.list_cap(v) >= n + 4 and words.size == 4 + 2 * cap and int(words[2]) == v.size
            pos, before = lc.rm.boundaries(v)
            assert n == pos.size and np.array_equal(words[4:4 + 2 * n:2], pos) and np.array_equal(words[5:5 + 2 * n:2], before)
            assert tuple(words[4 + 2 * n: 6 + 2 * n]) == (lc.INT32_MAX, int(v.sum()))
            assert (words[6 + 2 * n:] == -1).all() and words[6 + 2 * n:].size >= 2 * 3
            assert _sample_extent(img, i) == (o, o + 16 + 8 * (n + 1))


def test_mixed_element_types_share_one_image():
    """float64 references among bit-packed candidates: every vector at its own type's alignment and residues."""
    vecs = [_vectors(lc.F64)[12], _vectors(lc.U1)[3], _vectors(lc.U1)[13], _vectors(lc.F64, 1)[11], _vectors(lc.U1, 1)[5],
            _vectors(lc.U1, 1)[16]]
    kinds = [lc.F64, lc.U1, lc.U1] * 2
    for layout in lc.LAYOUTS:
        img = lc.build(vecs, kinds, layout)
        for i, (v, k) in enumerate(zip(vecs, kinds)):
            assert img.offs[i] % lc.ALIGN[k] == 0
            assert np.array_equal(img.vector(i), v if k == lc.F64 else (v != 0).astype(np.uint8))
        if layout == "shifted":
            assert [int(o) % 64 for o in img.offs] == [8, 4, 8, 24, 12, 20]
        if layout == "abutting":
            gaps = img.offs[1:] - (img.offs + img.nbytes)[:-1]
            assert (gaps >= 0).all() and (gaps < 8).all() and (gaps[[0, 1, 3, 4]] == 0).all()
        if layout != "clean":
            assert np.isnan(img.host[img.offs[0] - 8: img.offs[0]].view(np.float64)[0])
            assert np.isnan(img.host[img.offs[0] - 4: img.offs[0]].view(np.float32)[0])


def test_cover_lengths_and_the_gpu_problem_sets():
    assert lc.length_gaps([64, 33, 95]) == ["words % 4 == 0", "words % 4 == 1", "a vector shorter than 32 samples"]
    rng = np.random.RandomState(0)
    for _ in range(50):
        lens = rng.randint(192, 20000, size=rng.randint(5, 13)).tolist()
        got = lc.cover_lengths(lens)
        assert not lc.length_gaps(got) and len(got) == len(lens)
        assert all(0 <= a - b < 160 for a, b in zip(lens[:-1], got[:-1])) and got[-1] == 19
    import test_gpu_layout as tgl

    for name, lens in tgl.problem_set_lengths().items():
        assert not lc.length_gaps(lens), (name, lc.length_gaps(lens))
    # the three extraction widths, and one sweep of each width: one sample short of it, equal to it and 33 past it
    counts = {name: len(lens) for name, lens in tgl.problem_set_lengths().items() if name.startswith("extract")}
    assert counts == {"extract3": 3 + 9, "extract300": 300, "extract800": 800}
    sweeps = {d + s for s in (65536, 131072, 262144) for d in (-1, 0, 33)}
    assert sweeps <= set(tgl.problem_set_lengths()["extract3"])
