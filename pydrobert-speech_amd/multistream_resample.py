"""Batched streaming rate conversion: ``pre.Resample`` per stream across ticks, one launch per tick.

``ResampleBatch`` stands in front of ``StreamBatch`` / ``SiStreamBatch``: it takes each stream's chunk at `from_rate`
and returns, back to back in one GPU tensor, the samples at `to_rate` whose whole filter window has arrived --

    d_out, out_lengths = resampler.resample_chunks_packed(ids, d_samples, lengths)
    feats, rows = streams.compute_chunks_packed(ids, d_out, out_lengths)

-- and at a stream's end (:func:`ResampleBatch.finalize`) the rest, with the missing future read as nothing.  The
emission rule (``include/pds_amd_stages.h``): after n samples in all, the outputs k with
``first[p] + u * in_unit + ntaps[p] - 1 <= n - 1`` are due, ``Resample.num_due_samples(n)`` of them; ``finalize``
brings the count to ``Resample.num_output_samples(n)``.  The concatenation of a stream's outputs over its calls and its
``finalize`` is therefore ``Resample.apply`` of its whole signal, bit for bit, whatever the cuts, for float32, float64
and int16 chunks alike.

State: per stream on the device its last ``max_taps - 1`` input samples, one pool ``dtype[capacity][max_taps - 1]``;
on the host the samples seen and the outputs emitted.  There is no CPU path.
"""
from typing import List, Sequence, Tuple

import numpy as np

from . import _native
from .alias import alias_factory_subclass_from_arg
from .pre import PreProcessor, Resample

__all__ = ["ResampleBatch"]

_META_FIELDS = 8  # int64 per entry: stream, chunk offset, chunk length, seen, first output, outputs, output offset, 0


class ResampleBatch:
    """`capacity` streams resampled by `resample` (a ``Resample`` or what configures one), chunks of `dtype`
    (float32, float64 or int16; int16 gives float32 outputs) on `device`"""

    def __init__(self, resample, capacity: int, dtype=np.float32, device=None):
        if not isinstance(resample, Resample):
            if isinstance(resample, PreProcessor) or not isinstance(resample, (str, dict)):
                raise ValueError(f"resample must be a Resample or its configuration, not {resample!r}")
            resample = alias_factory_subclass_from_arg(PreProcessor, resample)
            if not isinstance(resample, Resample):
                raise ValueError(f"resample configures a {type(resample).__name__}, not a Resample")
        if isinstance(capacity, (bool, np.bool_)) or int(capacity) != capacity or capacity < 1:
            raise ValueError("capacity must be a positive integer")
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.int16)):
            raise ValueError("dtype must be float32, float64 or int16")
        self.out_dtype = np.dtype(np.float64) if self.dtype == np.float64 else np.dtype(np.float32)
        self.resample, self.capacity = resample, int(capacity)
        self.seen = np.zeros(self.capacity, dtype=np.int64)  # samples given to each stream since its start
        self.emitted = np.zeros(self.capacity, dtype=np.int64)  # outputs returned for them
        torch = self._torch = _native.require_device()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._tdtype = getattr(torch, self.dtype.name)
        self._tout = getattr(torch, self.out_dtype.name)
        self._hist = torch.zeros((self.capacity, resample.max_taps - 1), dtype=self._tdtype, device=self.device)
        self._fn = None
        if not resample.is_identity:
            lib = _native.stages_lib()
            self._fn = {"float32": lib.pds_multistream_resample_f32, "float64": lib.pds_multistream_resample_f64,
                        "int16": lib.pds_multistream_resample_i16_f32}[self.dtype.name]
            self._tables = resample._tables(self.device)

    # ---- the host side of a tick ----------------------------------------------------------------------------------

    def check_ids(self, ids) -> np.ndarray:
        """`ids` as int64, or ``ValueError`` if any is unknown, negative or repeated"""
        arr = np.asarray(ids)
        if arr.ndim != 1:
            raise ValueError("ids must be a 1-D sequence of stream indices")
        if arr.size == 0:
            return np.zeros(0, dtype=np.int64)
        if not np.issubdtype(arr.dtype, np.integer):
            raise ValueError("stream ids must be integers")
        arr = arr.astype(np.int64, copy=False)
        if arr.min() < 0 or arr.max() >= self.capacity:
            raise ValueError(f"stream ids must lie in [0, {self.capacity})")
        if np.unique(arr).size != arr.size:
            raise ValueError("a tick names each stream at most once")
        return arr

    def step(self, ids: np.ndarray, lengths: np.ndarray, final: bool = False) -> dict:
        """What a tick that brings streams `ids` chunks of `lengths` computes: per stream the samples seen before, the
        first output and the number of outputs.  Changes nothing."""
        n0 = self.seen[ids]
        n1 = n0 + lengths
        k0 = self.emitted[ids]
        if final or self.resample.is_identity:  # (equal rates: a sample is its own output)
            upto = self.resample.num_output_samples(n1)
        else:
            upto = self.resample.num_due_samples(n1)
        return {"seen": n0, "after": n1, "first": k0, "count": np.asarray(upto, dtype=np.int64).reshape(-1) - k0}

    def commit(self, ids: np.ndarray, step: dict, final: bool = False) -> None:
        if final:
            self.seen[ids] = 0
            self.emitted[ids] = 0
        else:
            self.seen[ids] = step["after"]
            self.emitted[ids] = step["first"] + step["count"]

    @staticmethod
    def fill_meta(meta: np.ndarray, ids: np.ndarray, lengths: np.ndarray, step: dict) -> np.ndarray:
        """the ``(n, 8)`` int64 table of ``pds_multistream_resample_*``; returns the output offsets, ``n + 1`` of them"""
        out_offs = np.concatenate([[0], np.cumsum(step["count"])]).astype(np.int64)
        meta[:, 0] = ids
        meta[:, 1] = np.cumsum(lengths) - lengths
        meta[:, 2] = lengths
        meta[:, 3] = step["seen"]
        meta[:, 4] = step["first"]
        meta[:, 5] = step["count"]
        meta[:, 6] = out_offs[:-1]
        meta[:, 7] = 0
        return out_offs

    def pending(self, ids) -> Tuple[np.ndarray, np.ndarray]:
        """``(seen, emitted)`` of streams `ids`: the samples each has been given since its start and the outputs it
        has returned (``finalize`` would return ``num_output_samples(seen) - emitted`` more)"""
        self._check_open()
        ids = self.check_ids(ids)
        return self.seen[ids].copy(), self.emitted[ids].copy()

    # ---- the calls ------------------------------------------------------------------------------------------------

    def resample_chunks_packed(self, ids, d_samples, lengths) -> Tuple[object, np.ndarray]:
        """Chunks already on the GPU: `d_samples` holds them back to back (1-D contiguous tensor of this object's dtype
        on its device), ``lengths[i]`` samples for stream ``ids[i]`` (0 is legal).  Returns ``(d_out, out_lengths)``:
        the due outputs of the streams back to back, and how many each has -- what
        ``StreamBatch.compute_chunks_packed(ids, d_out, out_lengths)`` takes"""
        self._check_open()
        torch = self._torch
        ids = self.check_ids(ids)
        lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        if len(lengths) != len(ids):
            raise ValueError("one length per stream id")
        if len(lengths) and lengths.min() < 0:
            raise ValueError("negative chunk length")
        if (not isinstance(d_samples, torch.Tensor) or d_samples.device != self.device or d_samples.dim() != 1
                or not d_samples.is_contiguous() or d_samples.dtype != self._tdtype):
            raise ValueError(f"d_samples must be a contiguous 1-D {self.dtype} tensor on {self.device}")
        if int(lengths.sum()) > d_samples.numel():
            raise ValueError("the chunks lie outside d_samples")
        return self._tick(ids, lengths, d_samples, False)

    def finalize_packed(self, ids) -> Tuple[object, np.ndarray]:
        """The streams' last outputs, ``(d_out, out_lengths)`` as :func:`resample_chunks_packed`; the streams are fresh
        afterwards and may be used again.  A fresh stream gives nothing."""
        self._check_open()
        ids = self.check_ids(ids)
        return self._tick(ids, np.zeros(len(ids), dtype=np.int64), None, True)

    def resample_chunks(self, ids, chunks: Sequence) -> List[np.ndarray]:
        """:func:`resample_chunks_packed` of host chunks (``chunks[i]``, a 1-D array, for stream ``ids[i]``); returns
        the list of output arrays in the order of `ids`"""
        self._check_open()
        torch = self._torch
        ids = self.check_ids(ids)
        if len(chunks) != len(ids):
            raise ValueError("one chunk per stream id")
        arrs = [np.asarray(c) for c in chunks]
        if any(a.ndim != 1 for a in arrs):
            raise ValueError("chunks must be 1-dimensional")
        if any(a.dtype != self.dtype for a in arrs):
            raise ValueError(f"chunks must be {self.dtype}")
        lengths = np.fromiter(map(len, arrs), dtype=np.int64, count=len(arrs))
        host = np.concatenate(arrs) if len(arrs) else np.zeros(0, self.dtype)
        d_out, out_lengths = self._tick(ids, lengths, torch.from_numpy(host).to(self.device), False)
        return self._to_host(d_out, out_lengths)

    def finalize(self, ids) -> List[np.ndarray]:
        """:func:`finalize_packed` with the outputs as a list of host arrays"""
        return self._to_host(*self.finalize_packed(ids))

    def close(self) -> None:
        """Release the pool; the object cannot be used afterwards"""
        self._hist = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- a tick -----------------------------------------------------------------------------------------------------

    def _check_open(self):
        if self._hist is None:
            raise ValueError("ResampleBatch is closed")

    def _to_host(self, d_out, out_lengths) -> List[np.ndarray]:
        host = d_out.cpu().numpy()
        ends = np.cumsum(out_lengths)
        return [host[e - n : e].copy() for e, n in zip(ends.tolist(), out_lengths.tolist())]

    def _tick(self, ids, lengths, d_samples, final):
        torch = self._torch
        n = len(ids)
        step = self.step(ids, lengths, final)
        if self._fn is None:  # equal rates: the chunks themselves (widened), no launch and no history
            total = int(lengths.sum())
            d_out = (d_samples[:total].to(self._tout, copy=True) if total
                     else torch.empty(0, dtype=self._tout, device=self.device))
            self.commit(ids, step, final)
            return d_out, step["count"].copy()
        meta = np.empty((n, _META_FIELDS), dtype=np.int64)
        out_offs = self.fill_meta(meta, ids, lengths, step)
        d_out = torch.empty(int(out_offs[-1]), dtype=self._tout, device=self.device)
        if n:
            rs = self.resample
            first, ntaps, weights = self._tables
            d_meta = torch.from_numpy(meta).to(self.device)
            with torch.cuda.device(self.device):
                rc = self._fn(d_samples.data_ptr() if d_samples is not None and d_samples.numel() else None,
                              self._hist.data_ptr(), self.capacity, rs.in_unit, rs.out_unit, rs.max_taps,
                              first.data_ptr(), ntaps.data_ptr(), weights.data_ptr(), d_meta.data_ptr(), n,
                              d_out.data_ptr() if d_out.numel() else None,
                              torch.cuda.current_stream(self.device).cuda_stream)
            _native.check_stages(rc, "pds_multistream_resample")
        self.commit(ids, step, final)
        return d_out, step["count"].copy()
