"""Pre-processors: ``Preemphasize`` and ``Dither`` (reference pre.py:39-149), on the GPU.

These sit immediately before the hot path in the reference's drivers
(command_line.py:127-128, 346-348).  Both are one element-wise pass over the signal;
pre-emphasis can instead be fused into the STFT kernels' frame load
(``STFTFrameComputer.compute_full_batch(signals, preemphasis=0.97)``), which saves the pass.
Intermediate arithmetic is float64 and the result is cast back to the input dtype, as in the
reference.  ``Dither`` draws its noise from a counter-based generator on the device (Philox),
so it matches the reference statistically, not sample for sample (the reference's own test
checks the standard deviation only, tests/test_pre.py:6-12).
"""
import abc
import warnings
from typing import Optional

import numpy as np

from . import _native
from .alias import AliasedFactory

__all__ = ["Dither", "PreProcessor", "Preemphasize", "dither_keys"]

_AXIS_DEP_MSG = (
    "Specifying axis in preprocessor.apply is deprecated. "
    "Preprocessors should be applied to 1D signals only."
)


class PreProcessor(AliasedFactory):
    """A transform applied to a signal before framing (reference pre.py:39-64)"""

    @abc.abstractmethod
    def apply(self, signal, axis: Optional[int] = None, in_place: bool = False):
        pass


def _device_copy(signal):
    """(tensor on the GPU in float32/float64, was_gpu, original numpy dtype or None)"""
    torch = _native.require_device()
    if getattr(signal, "is_cuda", False):
        t = signal if signal.dtype in (torch.float32, torch.float64) else signal.to(torch.float64)
        return t.contiguous(), True, None
    arr = np.asarray(signal)
    work = arr if arr.dtype in (np.float32, np.float64) else arr.astype(np.float64)
    return torch.from_numpy(np.array(work, order="C", copy=True)).to("cuda"), False, arr.dtype


def _finish(t, was_gpu, dtype, original, in_place):
    if was_gpu:
        return t
    res = t.cpu().numpy()
    if res.dtype != dtype:
        res = res.astype(dtype)
    if in_place and isinstance(original, np.ndarray) and original.flags.writeable:
        original[...] = res
        return original
    return res


def _seed_state(seed: Optional[int]) -> int:
    """the 64-bit state a ``Dither(seed=seed)`` starts from (fresh entropy for ``None``)"""
    return int(np.random.SeedSequence(seed).generate_state(1, np.uint64)[0])


def _next_key(state: int) -> int:
    """one step of the state: the generator key of the next launch (and the state after it)"""
    return (state * 6364136223846793005 + 1442695040888963407) % (1 << 64)


def dither_keys(seeds) -> np.ndarray:
    """uint64 per seed: the generator key of the first ``apply`` of ``Dither(seed=s)`` -- the one rule by which
    ``Dither``, :func:`Dither.apply_packed` and the batched streaming (``StreamBatch(dither=...)``) turn a seed into a
    key"""
    return np.fromiter((_next_key(_seed_state(int(s))) for s in seeds), dtype=np.uint64, count=len(seeds))


class Dither(PreProcessor):
    """Add Gaussian noise of standard deviation `coeff` (aliases ``dither``, ``dithering``)

    `seed` makes the noise reproducible; each :func:`apply` advances it.  The noise of sample t of a signal depends on
    the launch's key and t alone (``csrc/dither_noise.h``), so a signal may be dithered in pieces:
    :func:`apply_packed` does many utterances in one launch, ``StreamBatch(dither=...)`` a stream chunk by chunk.
    """

    aliases = {"dither", "dithering"}

    def __init__(self, coeff: float = 1.0, seed: Optional[int] = None):
        super().__init__()
        self.coeff = coeff
        self._given_seed = seed
        self._seed = _seed_state(seed)

    @property
    def seed(self) -> Optional[int]:
        """the `seed` this object was built with"""
        return self._given_seed

    def __repr__(self) -> str:
        # (what the object was built with and nothing of where it lies: a test id made of it is the same in every run)
        return f"Dither(coeff={self.coeff!r}, seed={self._given_seed!r})"

    def apply(self, signal, axis: Optional[int] = None, in_place: bool = False):
        if axis is not None:
            warnings.warn(_AXIS_DEP_MSG, DeprecationWarning)
        torch = _native.require_device()
        t, was_gpu, dtype = _device_copy(signal)
        shape = tuple(t.shape)
        if axis is not None and len(shape) > 1:
            # one noise value per position along `axis`, shared by the other axes
            # (reference pre.py:96-99): dither a vector of that length and broadcast-add
            noise = torch.zeros(shape[axis], dtype=t.dtype, device=t.device)
            noise = self._launch(noise, noise)
            view = [1] * len(shape)
            view[axis] = shape[axis]
            out = t + noise.reshape(view)
        else:
            out = self._launch(t, t if (was_gpu and in_place) else torch.empty_like(t))
        return _finish(out, was_gpu, dtype, signal, in_place)

    def _launch(self, src, dst):
        torch = _native.require_device()
        lib = _native.lib()
        fn = lib.pds_dither_f32 if src.dtype == torch.float32 else lib.pds_dither_f64
        self._seed = _next_key(self._seed)
        with torch.cuda.device(src.device):
            rc = fn(src.data_ptr(), src.numel(), float(self.coeff), self._seed, dst.data_ptr(),
                    torch.cuda.current_stream(src.device).cuda_stream)
        _native.check(rc, "pds_dither")
        return dst

    def apply_packed(self, signal, offsets, lengths, seeds=None):
        """Dither every utterance of a packed GPU buffer in one launch (see ``compute_packed``)

        `signal`: a 1-D GPU tensor of float32, float64 or int16 (16-bit PCM is widened on the device, exactly, and
        gives a float32 result); utterance b is ``signal[offsets[b] : offsets[b] + lengths[b]]``.  With `seeds`, one
        integer per utterance, utterance b receives exactly what the first ``apply`` of ``Dither(self.coeff,
        seed=seeds[b])`` gives it alone, and this object's own seed sequence is not touched.  With ``seeds=None`` the
        result is that of ``self.apply`` called once per utterance, in order: the seed sequence advances
        ``len(lengths)`` times.  Returns a new tensor of `signal`'s length.  For float input, samples outside every
        utterance keep their values; for int16 input only the utterance spans are defined.
        """
        torch = _native.require_device()
        lib = _native.lib()
        if not getattr(signal, "is_cuda", False) or signal.dim() != 1:
            raise ValueError("signal must be a 1-D GPU tensor")
        if signal.dtype not in (torch.float32, torch.float64, torch.int16):
            raise ValueError("signal must be float32, float64 or int16")
        offs_h = np.asarray(offsets, dtype=np.int64).reshape(-1)
        lens_h = np.asarray(lengths, dtype=np.int64).reshape(-1)
        B = len(lens_h)
        if len(offs_h) != B:
            raise ValueError("one offset per length")
        if B and (offs_h.min() < 0 or lens_h.min() < 0 or int((offs_h + lens_h).max()) > signal.numel()):
            raise ValueError("the utterances lie outside signal")
        if seeds is None:
            keys = np.empty(B, dtype=np.uint64)
            for b in range(B):
                self._seed = keys[b] = _next_key(self._seed)
        else:
            if len(seeds) != B:
                raise ValueError("one seed per utterance")
            keys = dither_keys(seeds)
        signal = signal.contiguous()
        if signal.dtype == torch.int16:
            fn = lib.pds_dither_packed_i16_f32
            out = torch.empty(signal.shape, dtype=torch.float32, device=signal.device)
        else:
            fn = lib.pds_dither_packed_f32 if signal.dtype == torch.float32 else lib.pds_dither_packed_f64
            out = signal.clone()  # gaps between utterances keep their contents
        # offsets, lengths and keys go up in one copy (a key's bits travel as int64)
        table = torch.as_tensor(np.stack([offs_h, lens_h, keys.view(np.int64)])).to(signal.device)
        with torch.cuda.device(signal.device):
            for lo in range(0, B, 65535):
                hi = min(B, lo + 65535)
                rc = fn(signal.data_ptr(), table[0, lo:].data_ptr(), table[1, lo:].data_ptr(),
                        table[2, lo:].data_ptr(), hi - lo, int(lens_h[lo:hi].max()), float(self.coeff),
                        out.data_ptr(), torch.cuda.current_stream(signal.device).cuda_stream)
                _native.check(rc, "pds_dither_packed")
        return out


class Preemphasize(PreProcessor):
    """``new[i] = old[i] - coeff * old[i-1]``, ``new[0] = old[0]`` (aliases ``preemphasize``,
    ``preemphasis``, ``preemph``)"""

    aliases = {"preemphasize", "preemphasis", "preemph"}

    def __init__(self, coeff: float = 0.97):
        super().__init__()
        self.coeff = coeff

    def __repr__(self) -> str:
        return f"Preemphasize(coeff={self.coeff!r})"

    def apply(self, signal, axis: Optional[int] = None, in_place: bool = False):
        if axis is not None:
            warnings.warn(_AXIS_DEP_MSG, DeprecationWarning)
        torch = _native.require_device()
        lib = _native.lib()
        t, was_gpu, dtype = _device_copy(signal)
        if t.dim() == 0 or t.numel() == 0:
            return _finish(t.clone(), was_gpu, dtype, signal, in_place)
        moved = axis not in (-1, None) and t.dim() > 1
        if moved:
            t = t.movedim(axis, -1).contiguous()
        rows, n = t.numel() // t.shape[-1], t.shape[-1]
        out = torch.empty_like(t)
        offs = torch.arange(rows, dtype=torch.int64, device=t.device) * n
        lens = torch.full((rows,), n, dtype=torch.int64, device=t.device)
        fn = lib.pds_preemphasize_f32 if t.dtype == torch.float32 else lib.pds_preemphasize_f64
        with torch.cuda.device(t.device):
            for lo in range(0, rows, 65535):
                hi = min(rows, lo + 65535)
                rc = fn(t.data_ptr(), offs[lo:].data_ptr(), lens[lo:].data_ptr(), hi - lo, n,
                        float(self.coeff), out.data_ptr(),
                        torch.cuda.current_stream(t.device).cuda_stream)
                _native.check(rc, "pds_preemphasize")
        if moved:
            out = out.movedim(-1, axis)
        return _finish(out, was_gpu, dtype, signal, in_place)

    def apply_packed(self, signal, offsets, lengths):
        """Pre-emphasise every utterance of a packed GPU buffer (see ``compute_packed``)

        `signal`: a 1-D GPU tensor of float32 or float64; utterance b is ``signal[offsets[b] : offsets[b] +
        lengths[b]]``.  Returns a new tensor of `signal`'s length and dtype; samples outside every utterance keep their
        values.
        """
        torch = _native.require_device()
        lib = _native.lib()
        if not getattr(signal, "is_cuda", False) or signal.dim() != 1:
            raise ValueError("signal must be a 1-D GPU tensor")
        if signal.dtype not in (torch.float32, torch.float64):
            raise ValueError("signal must be float32 or float64")
        offs_h = np.asarray(offsets, dtype=np.int64).reshape(-1)
        lens_h = np.asarray(lengths, dtype=np.int64).reshape(-1)
        B = len(lens_h)
        if len(offs_h) != B:
            raise ValueError("one offset per length")
        if B and (offs_h.min() < 0 or lens_h.min() < 0 or int((offs_h + lens_h).max()) > signal.numel()):
            raise ValueError("the utterances lie outside signal")
        signal = signal.contiguous()
        offs = torch.as_tensor(offs_h).to(signal.device)
        lens = torch.as_tensor(lens_h).to(signal.device)
        out = signal.clone()  # gaps between utterances keep their contents
        fn = lib.pds_preemphasize_f32 if signal.dtype == torch.float32 else lib.pds_preemphasize_f64
        with torch.cuda.device(signal.device):
            for lo in range(0, B, 65535):
                hi = min(B, lo + 65535)
                rc = fn(signal.data_ptr(), offs[lo:].data_ptr(), lens[lo:].data_ptr(), hi - lo,
                        int(lens_h[lo:hi].max()) if hi > lo else 0, float(self.coeff),
                        out.data_ptr(), torch.cuda.current_stream(signal.device).cuda_stream)
                _native.check(rc, "pds_preemphasize")
        return out
