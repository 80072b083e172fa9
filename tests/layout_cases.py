"""TEST INFRASTRUCTURE ONLY -- hostile input layouts and canaried outputs for tests/test_gpu_layout.py, checked on the
host by tests/test_layout_cases_host.py.  Imports without a GPU.

include/ffsubsync_amd.h grants the callers less than the suite's builders give them: bit-packed (U1) and float32 vectors
need 4-byte alignment, float64 vectors and ``ffs_runs_list`` blocks 8, bytes none, and nothing is said about what lies
around a vector.  ``build`` lays host vectors of any of these element types into ONE byte image:

  clean     the control, what ``batch.pack_pairs`` makes: 64-byte offsets, zero gaps, zero bits behind ``len``
  poisoned  the same offsets; every byte that is not a sample is 0xFF -- the gaps, a guard region in front of the first and
            behind the last vector, the bits of a U1 vector's last word at positions >= len, the list entries behind the
            sentinel e[n].  0xFF bytes are "1" samples for U8 and U1 and NaN for F32 and F64.
  shifted   poisoned, and every vector starts at the least alignment the header grants: byte offsets cycle through
            ``RESIDUES`` of the element type (mod 64)
  abutting  shifted without gaps: a vector starts at the first legally aligned byte behind the vector in front of it, so
            what lies behind a vector is another vector's data, not a constant (ones OR-ed into ones hide an over-read)

The guard regions (``GUARD`` bytes each) are wider than the widest look-ahead in the kernels -- the next-sweep request of
the 1024-thread list extraction, 1024 threads x 2 groups x 16 B = 32 KiB -- so an over-read of a hostile vector stays
inside the allocation and reads poison; nothing here relies on, or tries to cause, an access outside an allocation.
``Image.upload`` keeps the image, ``assert_inputs_untouched`` compares the device buffer with it byte for byte after a
call.  ``canaried`` / ``Canaries`` are the same idea for caller-owned outputs.
"""
import numpy as np

from ffsubsync_amd import _native
from oracle import runs_model as rm

U8, F32, U1, F64, RUNS = (_native.FFS_DTYPE_U8, _native.FFS_DTYPE_F32, _native.FFS_DTYPE_U1, _native.FFS_DTYPE_F64,
                          _native.FFS_DTYPE_RUNS)
LAYOUTS = ("clean", "poisoned", "shifted", "abutting")
HOSTILE = LAYOUTS[1:]  # mildest first
GUARD = 256 * 1024
POISON = 0xFF
ALIGN = {U1: 4, F32: 4, U8: 1, F64: 8, RUNS: 8}  # what include/ffsubsync_amd.h grants
RESIDUES = {U1: (4, 8, 12, 20, 60), F32: (4, 8, 12, 20, 60), U8: (1, 2, 3, 5, 31, 63), F64: (8, 24, 56), RUNS: (8, 24, 40, 56)}
LIST_SLACK = 4  # entries a hostile list block holds behind what its list needs (n boundaries + the sentinel)
INT32_MAX = int(np.iinfo(np.int32).max)


def list_cap(v01) -> int:
    """Capacity of the block ``encode`` makes for a 0/1 vector: n + 1 + LIST_SLACK >= n + 4 entries."""
    return int(rm.boundaries(np.asarray(v01) != 0)[0].size) + 1 + LIST_SLACK


def encode(vec, kind, poison: bool):
    """(bytes of the vector in memory, mask of the bits in them that are samples).  The bytes that are not samples -- a
    U1 vector's bits behind ``len``, a list block's entries behind e[n] -- are 0xFF with ``poison``, else zero."""
    vec = np.asarray(vec)
    fill = POISON if poison else 0
    if kind == U8:
        raw = (vec != 0).astype(np.uint8)
        return raw, np.full(raw.size, 0xFF, np.uint8)
    if kind in (F32, F64):
        raw = np.ascontiguousarray(vec, dtype=np.float32 if kind == F32 else np.float64).view(np.uint8)
        return raw.copy(), np.full(raw.size, 0xFF, np.uint8)
    if kind == U1:
        n = vec.size
        mask = np.packbits(np.concatenate([np.ones(n, np.uint8), np.zeros(-n % 32, np.uint8)]), bitorder="little")
        raw = np.packbits(np.concatenate([(vec != 0).astype(np.uint8), np.zeros(-n % 32, np.uint8)]), bitorder="little")
        return raw | (~mask & fill), mask
    if kind == RUNS:
        v01 = vec != 0
        pos, before = rm.boundaries(v01)
        n, ones, cap = int(pos.size), int(v01.sum()), list_cap(v01)
        words = np.full(4 + 2 * cap, -1 if poison else 0, dtype=np.int32)
        words[:4] = (n, ones, v01.size, cap)
        words[4:4 + 2 * n:2], words[5:5 + 2 * n:2] = pos, before
        words[4 + 2 * n: 6 + 2 * n] = (INT32_MAX, ones)
        mask = np.zeros(words.size * 4, np.uint8)
        mask[: 16 + 8 * (n + 1)] = 0xFF
        return words.view(np.uint8), mask
    raise ValueError("unknown element type %r" % (kind,))


def decode(raw, kind, n):
    """The ``n`` samples back from a vector's bytes (lists: the 0/1 vector the entries in front of e[n] describe)."""
    raw = np.ascontiguousarray(raw)
    if kind == U8:
        return raw[:n].copy()
    if kind == F32:
        return raw[: 4 * n].view(np.float32).copy()
    if kind == F64:
        return raw[: 8 * n].view(np.float64).copy()
    if kind == U1:
        return np.unpackbits(raw, bitorder="little")[:n]
    words = raw.view(np.int32)
    return rm.bits_from_list(words[4:4 + 2 * int(words[0]):2], n)


def _up(x, a):
    return -(-x // a) * a


class Image:
    """One host byte image of many vectors: ``host`` (guards included), byte ``offs`` / ``nbytes`` / sample ``lens`` /
    element ``kinds`` per vector (flat, in the order given) and ``mask``, the bits of ``host`` that are samples."""

    def __init__(self, layout, host, mask, offs, nbytes, lens, kinds):
        self.layout, self.host, self.mask = layout, host, mask
        self.offs, self.nbytes, self.lens, self.kinds = offs, nbytes, lens, kinds
        self.data = None

    def vector(self, i):
        """Vector i's samples, sliced out of the image at its offset."""
        o = int(self.offs[i])
        return decode(self.host[o:o + int(self.nbytes[i])], int(self.kinds[i]), int(self.lens[i]))

    def upload(self):
        """The image as a uint8 CUDA tensor (kept in ``data``; torch allocations are at least 64-byte aligned)."""
        import torch

        self.data = torch.from_numpy(self.host).cuda()
        assert self.data.data_ptr() % 64 == 0
        return self

    def ptrs(self):
        return np.uint64(self.data.data_ptr()) + self.offs.astype(np.uint64)

    def device_batch(self, shape, lo, hi, dtype, ref_dtype=None, bounds=None):
        """``batch.DeviceBatch`` over the uploaded image: vectors in row-major order of ``shape`` = (pairs, 1 + cands)."""
        from ffsubsync_amd.batch import DeviceBatch

        return DeviceBatch(self.data, self.offs.reshape(shape).copy(), self.lens.reshape(shape).copy(),
                           np.asarray(lo, np.float64).reshape(shape), np.asarray(hi, np.float64).reshape(shape), dtype,
                           ref_dtype, bounds)

    def assert_inputs_untouched(self, what=""):
        got = self.data.cpu().numpy()
        if not np.array_equal(got, self.host):
            at = np.flatnonzero(got != self.host)
            owner = np.searchsorted(self.offs, at[0], side="right") - 1
            raise AssertionError("%s [%s]: %d input bytes changed, the first at byte %d (vector %d starts at %d)"
                                 % (what, self.layout, at.size, at[0], owner, self.offs[max(owner, 0)]))


def build(vectors, kinds, layout) -> Image:
    """Lay ``vectors`` (host arrays; 0/1 for U8 / U1 / RUNS) of element types ``kinds`` (one, or one per vector) out in
    one image.  The residues of ``shifted`` cycle per element type in the order of ``RESIDUES``; ``abutting`` starts its
    first vector at its type's first residue."""
    assert layout in LAYOUTS
    kinds = [int(kinds)] * len(vectors) if np.isscalar(kinds) else [int(k) for k in kinds]
    poison = layout != "clean"
    parts = [encode(v, k, poison) for v, k in zip(vectors, kinds)]
    turn = {k: 0 for k in RESIDUES}
    offs, cursor = [], GUARD
    for i, ((raw, _), k) in enumerate(zip(parts, kinds)):
        if layout in ("clean", "poisoned"):
            o = _up(cursor, 64)
        elif layout == "shifted" or i == 0:
            res = RESIDUES[k][turn[k] % len(RESIDUES[k])]
            turn[k] += 1
            o = cursor + (res - cursor) % 64
        else:
            o = _up(cursor, ALIGN[k])
        assert o % ALIGN[k] == 0
        offs.append(o)
        cursor = o + raw.size
    total = _up(cursor, 64) + GUARD
    host = np.full(total, POISON if poison else 0, dtype=np.uint8)
    mask = np.zeros(total, dtype=np.uint8)
    for (raw, m), o in zip(parts, offs):
        host[o:o + raw.size] = raw
        mask[o:o + raw.size] = m
    return Image(layout, host, mask, np.array(offs, np.int64), np.array([p[0].size for p in parts], np.int64),
                 np.array([np.asarray(v).size for v in vectors], np.int64), np.array(kinds, np.int64))


# ---- lengths ---------------------------------------------------------------------------------------------------------
def length_gaps(lens):
    """What a problem set's vector lengths still miss of: len % 32 in {0, 1, 31}, word counts % 4 in {0, 1, 2, 3} (the
    residue of the 16-byte groups) and one vector shorter than 32 samples.  Empty when all are covered."""
    lens = np.asarray(lens, dtype=np.int64).ravel()
    miss = ["len %% 32 == %d" % r for r in (0, 1, 31) if not (lens % 32 == r).any()]
    miss += ["words %% 4 == %d" % r for r in range(4) if not ((lens + 31) // 32 % 4 == r).any()]
    return miss + ([] if (lens < 32).any() else ["a vector shorter than 32 samples"])


def cover_lengths(lens, short=19):
    """``lens`` (at least five, all but the last >= 192) shortened by fewer than 160 samples each so that ``length_gaps``
    is empty: vector i gets len % 32 = (0, 1, 31)[i % 3] and words % 4 = i % 4, the last vector ``short`` samples."""
    lens = [int(n) for n in lens]
    assert len(lens) >= 5 and min(lens[:-1]) >= 192 and lens[-1] >= short
    out = []
    for i, n in enumerate(lens[:-1]):
        a, b = (0, 1, 31)[i % 3], i % 4
        out.append(next(m for m in range(n, n - 160, -1) if m % 32 == a and (m + 31) // 32 % 4 == b))
    out.append(short)
    assert not length_gaps(out)
    return out


# ---- caller-owned outputs --------------------------------------------------------------------------------------------
class Canaries:
    """A 0xFF-filled CUDA buffer with output slots at chosen residues (mod 64) and a guard in front of the first and
    behind the last: ``tensor(i, dtype, shape)`` is a view of slot i, ``assert_canaries_intact`` checks every byte
    outside the slots."""

    def __init__(self, slot_bytes, residues, guard=GUARD):
        import torch

        self.offs, cursor = [], guard
        for nb, res in zip(slot_bytes, residues):
            o = cursor + (int(res) - cursor) % 64
            self.offs.append(o)
            cursor = o + int(nb)
        self.slot_bytes = [int(nb) for nb in slot_bytes]
        self.buf = torch.full((_up(cursor, 64) + guard,), POISON, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 64 == 0
        self.outside = np.ones(self.buf.numel(), dtype=bool)
        for o, nb in zip(self.offs, self.slot_bytes):
            self.outside[o:o + nb] = False

    def ptr(self, i):
        return self.buf.data_ptr() + self.offs[i]

    def tensor(self, i, dtype=None, shape=None):
        t = self.buf[self.offs[i]: self.offs[i] + self.slot_bytes[i]]
        t = t if dtype is None else t.view(dtype)
        return t if shape is None else t.reshape(shape)

    def assert_canaries_intact(self, what=""):
        got = self.buf.cpu().numpy()
        bad = np.flatnonzero((got != POISON) & self.outside)
        if bad.size:
            slot = int(np.searchsorted(self.offs, bad[0], side="right")) - 1
            raise AssertionError("%s: %d bytes outside the outputs were written, the first at byte %d (slot %d covers "
                                 "[%d, %d))" % (what, bad.size, bad[0], slot, self.offs[max(slot, 0)],
                                                self.offs[max(slot, 0)] + self.slot_bytes[max(slot, 0)]))


def canaried(shape, dtype, residue):
    """(tensor of ``shape`` / torch ``dtype`` that is a view into a 0xFF-filled buffer at byte ``residue`` mod 64, with
    guards; its ``Canaries``)."""
    import torch

    n = int(np.prod(shape))
    c = Canaries([n * torch.empty(0, dtype=dtype).element_size()], [residue])
    return c.tensor(0, dtype, shape), c
