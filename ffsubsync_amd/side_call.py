"""What the side entry points share (host wrappers): the batch check, the plan sizing rule and the prepared
call of a block-wise plan.

Every batch entry point beside the headline aligner -- split, cut, drift, range drift, their reports, fits and
refinements, the cue report and retiming, the quality reports -- runs the same steps around its one native call: check
the arguments and the batch, read the batch as bits, count blocks, size a plan, allocate outputs, call, read back.  The
steps live here once; a module keeps what is its own: its checks, its ``per_pair`` workspace formula, its native call
and its record dtype.  Nothing here knows a plan class or a kernel.
"""
import numpy as np

from . import _native


def empty_error(ref_len: int, sub_len: int) -> ValueError:
    """aligners.py:58-66's wording for empty speech data."""
    return ValueError("cannot align empty speech data (reference length=%d, subtitle length=%d); the reference or subtitles "
                      "may contain no detectable speech" % (ref_len, sub_len))


def check_two_level_batch(batch, name: str, float_ref_message: bool = False, lists: bool = False) -> None:
    """The batch check of the entry point ``name`` (ValueError in its words): one candidate per pair, both vectors of
    one two-level type (bits or 0/1 bytes; with ``lists`` boundary lists too), no empty vector, finite levels.
    ``float_ref_message`` names a multi-level float reference as what it is, and states negative lengths as 0."""
    if batch.n_cand != 1:
        raise ValueError("%s needs one candidate per pair (DeviceBatch.select_candidates)" % name)
    ref_dt = batch.dtype if batch.ref_dtype is None else batch.ref_dtype
    if float_ref_message and ref_dt in (_native.FFS_DTYPE_F32, _native.FFS_DTYPE_F64):
        raise ValueError("%s needs a two-level reference: a multi-level float reference (FFS_DTYPE_%s) is not supported"
                         % (name, "F64" if ref_dt == _native.FFS_DTYPE_F64 else "F32"))
    two_level = (_native.FFS_DTYPE_U1, _native.FFS_DTYPE_U8) + ((_native.FFS_DTYPE_RUNS,) if lists else ())
    if ref_dt != batch.dtype or batch.dtype not in two_level:
        if lists:
            raise ValueError("%s needs two-level vectors of one type: bit-packed (FFS_DTYPE_U1), 0/1 bytes "
                             "(FFS_DTYPE_U8) or boundary lists (FFS_DTYPE_RUNS)" % name)
        raise ValueError("%s needs two-level vectors: bit-packed (FFS_DTYPE_U1) or 0/1 bytes (FFS_DTYPE_U8)" % name)
    lens = np.asarray(batch.lens)
    for p in range(lens.shape[0]):
        if lens[p, 0] <= 0 or lens[p, 1] <= 0:
            ref_len, sub_len = int(lens[p, 0]), int(lens[p, 1])
            raise empty_error(max(ref_len, 0), max(sub_len, 0)) if float_ref_message else empty_error(ref_len, sub_len)
    levels = np.concatenate([np.ravel(batch.lo), np.ravel(batch.hi)])
    if not np.all(np.isfinite(levels)):
        raise ValueError("two-level vectors need finite levels")


def pairs_for_budget(n_pairs: int, per_pair, cap: int = 256, budget: int = 12 << 30) -> int:
    """Pairs in flight of a plan whose workspace takes ``per_pair`` bytes a pair: all of them, up to ``cap`` and to what
    ``budget`` bytes hold, and at least one."""
    return int(max(1, min(n_pairs, cap, budget // per_pair)))


def no_workspace_split_plan(cache, n_pairs: int):
    """A split plan out of the caller's ``cache`` that holds no split workspace: refine and cue calls use its
    sub-batching and descriptors only, so only the cap on the pairs in flight binds."""
    return cache.get(pairs_for_budget(n_pairs, per_pair=1), 1, 2, 1)


def bits_batch(batch):
    """The batch as the side kernels read it: bit-packed vectors as they are, 0/1 bytes through ``to_bits()``."""
    return batch.to_bits() if batch.dtype == _native.FFS_DTYPE_U8 else batch


def block_shape(batch, block_samples: int):
    """(reference lengths, subtitle lengths, blocks of ``block_samples`` subtitle samples) of every pair, int64."""
    k = int(block_samples)
    ref_len, sub_len = batch.lens[:, 0].astype(np.int64), batch.lens[:, 1].astype(np.int64)
    return ref_len, sub_len, (sub_len + k - 1) // k


def pad_rows(n_blocks, what, *paths, clip: bool = False) -> list:
    """A given path on the host: each of ``paths`` is (rows, numpy dtype) with one row of per-block values per pair,
    and comes back as a zero-padded [n_pairs, max_b] array.  Row p needs ``n_blocks[p]`` entries (with ``clip`` at least
    as many: the rest is dropped); the first pair with a wrong row raises ValueError(``what(p, entries, blocks)``)."""
    outs = [np.zeros((len(n_blocks), int(max(n_blocks))), np_dtype) for _, np_dtype in paths]
    for p, nb in enumerate(int(b) for b in n_blocks):
        for (rows, _), out in zip(paths, outs):
            row = np.asarray(rows[p])[:nb] if clip else np.asarray(rows[p])
            if row.size != nb:
                raise ValueError(what(p, row.size, nb))
            out[p, :nb] = row
    return outs


def record_lists(recs, counts, from_record) -> list:
    """Per pair, ``from_record`` of its first ``counts[p]`` records of a [n_pairs, max_b] record array."""
    return [[from_record(x) for x in recs[p, :int(counts[p])]] for p in range(len(counts))]


class BlockCall:
    """One call of a block-wise side plan, prepared after the caller's checks have passed: the batch as bits, its shape
    in blocks of ``block_samples`` subtitle samples, and the output tensors and read-backs of that shape.  Needs a GPU."""

    def __init__(self, batch, block_samples: int) -> None:
        self.torch = _native.require_gpu()
        self.batch = bits_batch(batch)
        self.k, self.n = int(block_samples), batch.n_pairs
        self.ref_len, self.sub_len, self.n_blocks = block_shape(batch, self.k)
        self.max_b = int(self.n_blocks.max())
        self.dev = self.batch.data.device

    def pair_arrays(self):
        """The bits batch's host descriptor arrays, as every native call takes them first."""
        return self.batch.pair_arrays()

    def lag_dims(self, lo, hi):
        """(max_lags, max_samples) of a plan for the per-pair lag ranges [lo, hi]."""
        return int((hi - lo + 1).max()), int(max(self.sub_len.max(), self.ref_len.max()))

    def _empty(self, entries: int, np_dtype):
        return self.torch.empty(entries, dtype=getattr(self.torch, np.dtype(np_dtype).name), device=self.dev)

    def per_block(self, np_dtype):
        """An output tensor of n * max_b entries."""
        return self._empty(self.n * self.max_b, np_dtype)

    def per_pair(self, np_dtype):
        """An output tensor of n entries."""
        return self._empty(self.n, np_dtype)

    def records(self, record_dtype):
        """The output bytes of n * max_b records of the numpy ``record_dtype``."""
        return self._empty(self.n * self.max_b * record_dtype.itemsize, np.uint8)

    def read_blocks(self, tensor) -> np.ndarray:
        """A ``per_block`` tensor on the host, [n, max_b]."""
        return tensor.cpu().numpy().reshape(self.n, self.max_b)

    def read_records(self, tensor, record_dtype) -> np.ndarray:
        """A ``records`` tensor on the host, [n, max_b] of ``record_dtype``."""
        return tensor.cpu().numpy().view(record_dtype).reshape(self.n, self.max_b)

    def upload(self, padded) -> list:
        """The [n, max_b] host arrays of ``pad_rows`` as flat device tensors of n * max_b entries."""
        return [self.torch.from_numpy(rows.reshape(-1)).to(self.dev) for rows in padded]

    def place(self, what, *paths, clip: bool = False) -> list:
        """``upload`` of ``pad_rows``: a given path on the device, or the caller's ValueError."""
        return self.upload(pad_rows(self.n_blocks, what, *paths, clip=clip))
