"""Pre-processors: ``Preemphasize`` and ``Dither`` (reference pre.py:39-149) and ``Resample``, on the GPU.

These sit immediately before the hot path in the reference's drivers
(command_line.py:127-128, 346-348).  Both are one element-wise pass over the signal;
pre-emphasis can instead be fused into the STFT kernels' frame load
(``STFTFrameComputer.compute_full_batch(signals, preemphasis=0.97)``), which saves the pass.
Intermediate arithmetic is float64 and the result is cast back to the input dtype, as in the
reference.  ``Dither`` draws its noise from a counter-based generator on the device (Philox),
so it matches the reference statistically, not sample for sample (the reference's own test
checks the standard deviation only, tests/test_pre.py:6-12).

``Resample`` goes beyond the reference, towards what a Kaldi or torchaudio user expects in front of a filter bank built
for one sampling rate: a windowed-sinc rate conversion (Kaldi's ``LinearResample``) between integer rates, defined
exactly, so that one signal (:func:`Resample.apply`), a packed batch in one launch (:func:`Resample.apply_packed`) and
a stream cut into chunks (``multistream_resample.ResampleBatch``) give the same bits.  It is the one pre-processor that
changes a signal's length.
"""
import abc
import math
import numbers
import warnings
from typing import Optional

import numpy as np

from . import _native
from .alias import AliasedFactory

__all__ = ["Dither", "PreProcessor", "Preemphasize", "Resample", "dither_keys"]

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


def _positive_int(value, what: str, limit: int = (1 << 31) - 1) -> int:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, numbers.Integral):
        raise ValueError(f"{what} must be a positive integer, not {value!r}")
    if not 1 <= int(value) <= limit:
        raise ValueError(f"{what} must lie in [1, {limit}], not {value!r}")
    return int(value)


class Resample(PreProcessor):
    """Convert a signal from `from_rate` to `to_rate` samples per second with a windowed-sinc filter: Kaldi's
    ``LinearResample`` with its feature-extraction defaults (aliases ``resample``, ``resampling``)

    The definition.  from_rate and to_rate are positive integers, num_zeros >= 1, 0 < rolloff <= 1.

        g = gcd(from_rate, to_rate);  in_unit = from_rate / g;  out_unit = to_rate / g
        cutoff = rolloff * 0.5 * min(from_rate, to_rate);  width = num_zeros / (2 * cutoff)
        for phase p in [0, out_unit):  t = p / to_rate
            first[p] = ceil((t - width) * from_rate);  last[p] = floor((t + width) * from_rate)
            ntaps[p] = last[p] - first[p] + 1
            for j in [0, ntaps[p]):  d = (first[p] + j) / from_rate - t
                w[p][j] = f(d) * h(d) / from_rate
                f(d) = sin(2 pi cutoff d) / (pi d), and 2 cutoff at d == 0
                h(d) = 0.5 (1 + cos(2 pi cutoff / num_zeros d)) for |d| < width, else 0

    The table is built on the host in float64: first and ntaps as int32, w as float64 padded with zeros to max_taps,
    the largest ntaps[p].  An utterance of n samples gives m = ceil(n * to_rate / from_rate) output samples (Kaldi's
    flush form), and output k = u * out_unit + p, 0 <= p < out_unit, is

        y[k] = sum over j in [0, ntaps[p]) of w[p][j] * x[first[p] + u * in_unit + j]

    in float64, over j in ascending order, starting from +0.0, with x widened first and each product and each sum
    rounded separately; a tap whose index falls outside [0, n) contributes nothing; y[k] is rounded once to the output
    type: float32 for float32 and int16 input (int16 is widened exactly), float64 for float64 input.  NaN and infinite
    samples reach exactly the outputs whose windows hold them.

    ``from_rate == to_rate`` is the identity: a copy without a launch (int16 still becomes float32).  The table is
    uploaded once per object and device.  A table of more than ``Resample.MAX_TABLE`` = 1048576 entries
    (``out_unit * max_taps``) is refused: the kernels index it in 32 bits.
    """

    aliases = {"resample", "resampling"}
    MAX_TABLE = 1 << 20  # entries, out_unit * max_taps (csrc/resample_index.h)

    def __init__(self, from_rate: int, to_rate: int, num_zeros: int = 6, rolloff: float = 0.99):
        super().__init__()
        self.from_rate = _positive_int(from_rate, "from_rate")
        self.to_rate = _positive_int(to_rate, "to_rate")
        self.num_zeros = _positive_int(num_zeros, "num_zeros")
        if isinstance(rolloff, (bool, np.bool_)) or not isinstance(rolloff, numbers.Real) or not 0 < rolloff <= 1:
            raise ValueError(f"rolloff must lie in (0, 1], not {rolloff!r}")
        self.rolloff = float(rolloff)
        g = math.gcd(self.from_rate, self.to_rate)
        self.in_unit, self.out_unit = self.from_rate // g, self.to_rate // g
        limit = f"the weight table would have more than Resample.MAX_TABLE = {self.MAX_TABLE} entries (out_unit * max_taps)"
        if 2 * self.out_unit > self.MAX_TABLE:  # (every phase has at least two taps)
            raise ValueError(limit)
        cutoff = self.rolloff * 0.5 * min(self.from_rate, self.to_rate)
        width = self.num_zeros / (2 * cutoff)
        t = np.arange(self.out_unit, dtype=np.float64) / self.to_rate
        first = np.ceil((t - width) * self.from_rate).astype(np.int64)
        last = np.floor((t + width) * self.from_rate).astype(np.int64)
        ntaps = last - first + 1
        self.max_taps = int(ntaps.max())
        if self.out_unit * self.max_taps > self.MAX_TABLE:
            raise ValueError(limit)
        if (np.diff(last) < 0).any() or last[-1] > last[0] + self.in_unit or max(-first.min(), last.max()) >= 1 << 31:
            raise ValueError("the last input index of an output does not grow with the output: rates beyond float64")
        j = np.arange(self.max_taps, dtype=np.int64)
        d = (first[:, None] + j[None, :]) / self.from_rate - t[:, None]
        # sin and cos from the C library, value by value (numpy's vectorised ones differ from it, and from machine to
        # machine, in the last bit): the table is the same wherever it is built
        sin = np.fromiter(map(math.sin, (2 * np.pi * cutoff * d).ravel()), dtype=np.float64, count=d.size).reshape(d.shape)
        cos = np.fromiter(map(math.cos, (2 * np.pi * cutoff / self.num_zeros * d).ravel()), dtype=np.float64,
                          count=d.size).reshape(d.shape)
        with np.errstate(all="ignore"):
            f = np.where(d == 0, 2 * cutoff, sin / (np.pi * d))
        h = np.where(np.abs(d) < width, 0.5 * (1 + cos), 0.0)
        w = np.where(j[None, :] < ntaps[:, None], f * h / self.from_rate, 0.0)
        self._first, self._ntaps = first.astype(np.int32), ntaps.astype(np.int32)
        self._last = last.astype(np.int32)
        self._weights = np.ascontiguousarray(w, dtype=np.float64)
        for table in (self._first, self._ntaps, self._last, self._weights):
            table.flags.writeable = False
        self._device_tables = {}  # device index -> (first, ntaps, weights tap-major)

    first = property(lambda self: self._first, doc="int32 per phase: the first input index of the phase's unit-0 output")
    ntaps = property(lambda self: self._ntaps, doc="int32 per phase: its number of taps")
    last = property(lambda self: self._last, doc="int32 per phase: ``first + ntaps - 1``")
    weights = property(lambda self: self._weights, doc="float64 ``(out_unit, max_taps)``, zero behind a phase's taps")

    def __repr__(self) -> str:
        return (f"Resample(from_rate={self.from_rate!r}, to_rate={self.to_rate!r}, num_zeros={self.num_zeros!r}, "
                f"rolloff={self.rolloff!r})")

    @property
    def is_identity(self) -> bool:
        return self.from_rate == self.to_rate

    def num_output_samples(self, n):
        """``ceil(n * to_rate / from_rate)``: the output samples of an utterance of `n` (an integer or an array)"""
        n = np.asarray(n, dtype=np.int64)
        q, r = np.divmod(n, self.in_unit)
        m = q * self.out_unit + -(-(r * self.out_unit) // self.in_unit)
        return int(m) if m.ndim == 0 else m

    def num_due_samples(self, n):
        """The outputs whose whole window lies within the first `n` samples of a stream (an integer or an array): what
        a stream has emitted once it has been given `n` samples and not been finalized"""
        n = np.asarray(n, dtype=np.int64)
        q = n - 1
        u0 = np.floor_divide(q - int(self._last[-1]), self.in_unit)  # the last unit all of whose phases are due
        part = np.searchsorted(self._last, q - (u0 + 1) * self.in_unit, side="right")
        due = np.where((n <= 0) | (u0 < -1), 0, (u0 + 1) * self.out_unit + part).astype(np.int64)
        return int(due) if due.ndim == 0 else due

    def _tables(self, device):
        torch = _native.require_device()
        key = torch.device(device).index
        if key is None:
            key = torch.cuda.current_device()
        got = self._device_tables.get(key)
        if got is None:
            dev = torch.device("cuda", key)
            got = self._device_tables[key] = (
                torch.from_numpy(self._first.copy()).to(dev), torch.from_numpy(self._ntaps.copy()).to(dev),
                torch.from_numpy(self._weights.T.copy()).to(dev))  # tap-major
        return got

    def apply(self, signal, axis: Optional[int] = None, in_place: bool = False):
        """The resampled signal: a new 1-D array or tensor of ``num_output_samples(len(signal))`` samples, on the side
        `signal` came from

        float32, float64 and int16 (numpy arrays and GPU tensors) are taken as they are; any other dtype is widened to
        float64 first and gives a float64 result.  ``in_place=True`` is refused unless the rates are equal, because
        the length changes.
        """
        if axis is not None:
            warnings.warn(_AXIS_DEP_MSG, DeprecationWarning)
        if in_place and not self.is_identity:
            raise ValueError("Resample changes the signal's length: in_place=True needs from_rate == to_rate")
        # (the refusals, and equal rates in place, come before anything needs a device)
        was_gpu = bool(getattr(signal, "is_cuda", False))
        t = signal if was_gpu else np.asarray(signal)
        if t.ndim != 1:
            raise ValueError(f"Resample applies to 1-D signals, not to shape {tuple(t.shape)}")
        torch = _native.require_device() if was_gpu else None
        taken = (torch.float32, torch.float64, torch.int16) if was_gpu else (np.float32, np.float64, np.int16)
        if t.dtype not in taken:
            t = t.to(torch.float64) if was_gpu else t.astype(np.float64)
        if self.is_identity and in_place and t is signal and t.dtype != taken[2]:
            return signal
        if not was_gpu:
            torch = _native.require_device()
            t = torch.from_numpy(np.array(t, order="C", copy=True)).to("cuda")
        out, _, _ = self.apply_packed(t, [0], [t.numel()])
        return out if was_gpu else out.cpu().numpy()

    def apply_packed(self, signal, offsets, lengths):
        """Resample every utterance of a packed GPU buffer in one launch (see ``compute_packed``)

        `signal`: a 1-D GPU tensor of float32, float64 or int16 (16-bit PCM is widened on the device, exactly, and
        gives a float32 result); utterance b is ``signal[offsets[b] : offsets[b] + lengths[b]]``.  Returns
        ``(out, out_offsets, out_lengths)``: a new tensor that holds the resampled utterances back to back in order,
        and host int64 arrays such that utterance b is ``out[out_offsets[b] : out_offsets[b] + out_lengths[b]]``.
        """
        torch = _native.require_device()
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
        out_lens = np.asarray(self.num_output_samples(lens_h), dtype=np.int64).reshape(-1)
        ends = np.cumsum(out_lens)
        out_offs = (ends - out_lens).astype(np.int64)
        total = int(ends[-1]) if B else 0
        out_dtype = torch.float64 if signal.dtype == torch.float64 else torch.float32
        signal = signal.contiguous()
        if self.is_identity:  # a copy, no launch
            if B and (offs_h == out_offs).all():
                return signal[:total].to(out_dtype, copy=True), out_offs, out_lens
            pieces = [signal[o : o + n] for o, n in zip(offs_h.tolist(), lens_h.tolist())]
            out = torch.cat(pieces).to(out_dtype, copy=True) if pieces else signal[:0].to(out_dtype, copy=True)
            return out, out_offs, out_lens
        out = torch.empty(total, dtype=out_dtype, device=signal.device)
        if not total:
            return out, out_offs, out_lens
        lib = _native.stages_lib()
        fn = {torch.float32: lib.pds_resample_packed_f32, torch.float64: lib.pds_resample_packed_f64,
              torch.int16: lib.pds_resample_packed_i16_f32}[signal.dtype]
        first, ntaps, weights = self._tables(signal.device)
        # offsets, lengths and output offsets go up in one copy
        table = torch.as_tensor(np.stack([offs_h, lens_h, out_offs])).to(signal.device)
        # a call takes 2^31 - 1 blocks of 256 outputs, every utterance counted as the longest of its call
        tiles = -(-int(out_lens.max()) // 256)
        step = max(1, ((1 << 31) - 1) // tiles)
        with torch.cuda.device(signal.device):
            for lo in range(0, B, step):
                hi = min(B, lo + step)
                rc = fn(signal.data_ptr(), table[0, lo:].data_ptr(), table[1, lo:].data_ptr(),
                        table[2, lo:].data_ptr(), hi - lo, int(lens_h[lo:hi].max()), self.in_unit, self.out_unit,
                        self.max_taps, first.data_ptr(), ntaps.data_ptr(), weights.data_ptr(), out.data_ptr(),
                        torch.cuda.current_stream(signal.device).cuda_stream)
                _native.check_stages(rc, "pds_resample_packed")
        return out, out_offs, out_lens
