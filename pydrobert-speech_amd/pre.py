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

``AddNoise`` goes beyond the reference too: the waveform augmentation of Kaldi's multi-condition recipes
(``wav-reverberate --additive-signals --snrs``), a clip of a noise bank added to every utterance of a packed batch at a
signal-to-noise ratio drawn per utterance, defined exactly so that a numpy model reproduces it.

``Reverb`` is the other half of that tool (``--impulse-response --shift-output --normalize-output``): a room impulse
response of a bank convolved with every utterance of a packed batch by partitioned overlap-save on the device.
"""
import abc
import math
import numbers
import os
import warnings
from typing import NamedTuple, Optional

import numpy as np

from . import _native
from .alias import AliasedFactory

__all__ = ["AddNoise", "Dither", "NoisePlan", "PreProcessor", "Preemphasize", "Resample", "Reverb", "ReverbPlan",
           "dither_keys"]

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


class _Seeded:
    """The seed of a stage that draws: `seed` as given, the state of the object's own sequence, and the one rule that
    gives every utterance of a batch its key"""

    _SEEDS_ERROR = "one seed per utterance"

    def _start_seed(self, seed: Optional[int]) -> None:
        self._given_seed = seed
        self._seed = _seed_state(seed)

    @property
    def seed(self) -> Optional[int]:
        """the `seed` this object was built with"""
        return self._given_seed

    def _keys(self, B: int, seeds) -> np.ndarray:
        """uint64 per utterance: from `seeds` by :func:`dither_keys`, else the next `B` keys of the object's sequence"""
        if seeds is None:
            keys = np.empty(B, dtype=np.uint64)
            for b in range(B):
                self._seed = keys[b] = _next_key(self._seed)
            return keys
        if len(seeds) != B:
            raise ValueError(self._SEEDS_ERROR)
        return dither_keys(seeds)


_U32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _philox_draws(keys: np.ndarray, counter):
    """x0..x3 of one Philox4x32-10 block on `counter` under every key of `keys` (uint64): four uint64 arrays of 32-bit
    values (csrc/mix_rule.h: mix_draw, csrc/reverb_rule.h)"""
    keys = np.asarray(keys, dtype=np.uint64)
    k0, k1 = keys & _U32, keys >> _S32
    c = [np.full(keys.shape, word, dtype=np.uint64) for word in counter]
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _U32, (p0 >> _S32) ^ c[3] ^ k1, p0 & _U32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & _U32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _U32
    return c


def _is_gpu_tensor(x) -> bool:
    return bool(getattr(x, "is_cuda", False))


def _check_packed(signal, offsets, lengths):
    """What every packed waveform stage checks (Dither, AddNoise and Reverb): (offsets, lengths, B) on the host, or the
    ``ValueError`` -- nothing here needs a device"""
    import torch

    if not _is_gpu_tensor(signal) or signal.dim() != 1:
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
    return offs_h, lens_h, B


class Dither(_Seeded, PreProcessor):
    """Add Gaussian noise of standard deviation `coeff` (aliases ``dither``, ``dithering``)

    `seed` makes the noise reproducible; each :func:`apply` advances it.  The noise of sample t of a signal depends on
    the launch's key and t alone (``csrc/dither_noise.h``), so a signal may be dithered in pieces:
    :func:`apply_packed` does many utterances in one launch, ``StreamBatch(dither=...)`` a stream chunk by chunk.
    """

    aliases = {"dither", "dithering"}

    def __init__(self, coeff: float = 1.0, seed: Optional[int] = None):
        super().__init__()
        self.coeff = coeff
        self._start_seed(seed)

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
        offs_h, lens_h, B = _check_packed(signal, offsets, lengths)
        keys = self._keys(B, seeds)
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


# ---- AddNoise ---------------------------------------------------------------------------------------------------------

_MIX_CHUNK = 16384  # samples of a chunk of the segment energy (csrc/mix_rule.h: MIX_CHUNK)
_MIX_VEC, _MIX_TILE = 4, 4096  # samples of a lane's group and of a block of the apply kernel (MIX_VEC, MIX_TILE)
_MIX_ENERGY_WAVES = 4  # chunks of a block of the energy kernel (MIX_ENERGY_WAVES)
_MIX_MAX_BLOCKS = (1 << 31) - 1  # blocks of one launch (MIX_MAX_BLOCKS)
_MIX_MAX_UTTS = 65535  # utterances of one launch of the apply kernel (MIX_MAX_UTTS)
_MIX_COUNTER = (0, 0, 0, 0x4D495831)  # the counter of the plan's Philox block (MIX_COUNTER_0 .. MIX_COUNTER_3)


def _mix_pick(x: np.ndarray, n: np.ndarray) -> np.ndarray:
    """``(x * n) >> 32`` for 32-bit `x` and ``0 <= n < 2^63``, the product taken in two halves (mix_pick)"""
    n = np.asarray(n, dtype=np.uint64)
    return ((x * (n >> _S32)) + ((x * (n & _U32)) >> _S32)).astype(np.int64)


def _mix_chunks(n):
    """chunks of segments of `n` samples (an integer or an array)"""
    n = np.asarray(n, dtype=np.int64)
    return np.where(n > 0, (n + (_MIX_CHUNK - 1)) // _MIX_CHUNK, 0)


def _chunk_bases(lens_h):
    """(chunk base per segment, chunks in all), refusing more than 2^31 - 1 blocks of the energy kernel"""
    chunks = _mix_chunks(lens_h).astype(np.int64).reshape(-1)
    ends = np.cumsum(chunks)
    total = int(ends[-1]) if len(chunks) else 0
    if -(-total // _MIX_ENERGY_WAVES) > _MIX_MAX_BLOCKS:
        raise ValueError("the batch needs more than 2^31 - 1 blocks in one launch of the energy kernel: split it")
    return (ends - chunks).astype(np.int64), total


def _apply_calls(lens_h):
    """[(lo, hi, longest)] of the apply kernel's launches, refusing one of more than 2^31 - 1 blocks"""
    calls = []
    for lo in range(0, len(lens_h), _MIX_MAX_UTTS):
        hi = min(len(lens_h), lo + _MIX_MAX_UTTS)
        longest = int(lens_h[lo:hi].max())
        blocks_x = -(-(longest + _MIX_VEC - 1) // _MIX_TILE) if longest else 0
        if blocks_x * (hi - lo) > _MIX_MAX_BLOCKS:
            raise ValueError("the batch needs more than 2^31 - 1 blocks in one launch of the apply kernel: split it")
        calls.append((lo, hi, longest))
    return calls


def _suffix(dtype) -> str:
    return {"float32": "f32", "float64": "f64", "int16": "i16"}[str(dtype).replace("torch.", "")]


class NoisePlan(NamedTuple):
    """What :func:`AddNoise.plan` draws, one entry per utterance"""

    clip: np.ndarray  #: int64, the clip of the bank
    start: np.ndarray  #: int64, the first sample read of that clip
    snr_db: np.ndarray  #: float64, the signal-to-noise ratio in dB
    ratio: np.ndarray  #: float64, ``10 ** (snr_db / 10)``
    applied: np.ndarray  #: bool, whether the utterance gets noise at all


class AddNoise(_Seeded, PreProcessor):
    """Add a clip of a noise bank to every utterance at a signal-to-noise ratio drawn per utterance: the additive half
    of Kaldi's ``wav-reverberate --additive-signals --snrs`` (aliases ``add_noise``, ``additive_noise``, ``mix_noise``)

    `clips` is a non-empty sequence of noise clips, each a 1-D array, a 1-D tensor or a path that the readers of
    ``util.read_signal`` take (wav, npy, npz, pt); all of one dtype, float32, float64 or int16.  They are packed into
    one bank, uploaded once per device in that dtype (16-bit PCM stays at two bytes a sample and is widened exactly in
    the kernel).  `snr_db` is a number or a pair ``(lo, hi)``, ``lo <= hi``; `prob` in ``[0, 1]`` is the share of
    utterances that get noise at all; `seed` is as ``Dither``'s: an utterance's key comes from :func:`dither_keys`, and
    with ``seeds=None`` the object's own sequence advances once per utterance.  An utterance's result depends on its
    key, its samples, the bank and the parameters, not on the batch it stands in, its position there, or the launch.

    The definition.

    Segment energy `E(x, n)` of `n` samples, float64:

    - Chunk `c` covers samples `[c·16384, min(n, (c+1)·16384))`.
    - In a chunk, lane `l` of 64 starts at `p_l = +0.0`. For `i = l, l+64, …` inside the chunk, in that order, it takes
      `v = float64(x[i])` and `p_l = p_l + v·v`. The product is rounded by itself, and it is exact for float32 and int16
      samples.
    - The chunk sum is the fixed tree: for `s = 32, 16, 8, 4, 2, 1`, `p_l = p_l + p_{l+s}` for all `l < s`. The result
      is `p_0`.
    - `E` starts at `+0.0` and takes the chunk sums in ascending order.
    - `E(x, 0) = 0.0`.
    - Mean power is `P = E / float64(n)` for `n > 0`, else `0.0`.

    Plan of utterance `b`, built on the host in integers and float64:

    - One Philox4x32-10 block: key = the utterance's 64-bit key (low word, high word, as `dither_noise.h` splits it),
      counter = `(0, 0, 0, 0x4D495831)`. `dither_noise.h` and `specaug_rule.h` leave the fourth counter word zero, so
      this counter differs from every one of theirs.
    - Output words `x0..x3`, with `K` clips and `L_j` the length of clip `j`:
      - clip `j = (uint64(x0) · K) >> 32`
      - start `s = (uint64(x1) · L_j) >> 32`
      - `snr = lo + (hi − lo) · (float64(x2) · 2⁻³²)`, each operation rounded by itself. It is exactly `lo` when
        `lo == hi`.
      - `applied = float64(x3) · 2⁻³² < prob`
      - ratio `r = math.pow(10.0, snr / 10.0)`, one scalar call per utterance.

    Gain, on the device, float64, one lane per utterance:

    - `Ps` is the mean power of the utterance's samples. `Pn` is that of the whole clip `j`.
    - If `applied`, `Ps > 0` and `Pn > 0`, then `g = sqrt(Ps / (Pn · r))`. The product, the quotient and the root are
      each rounded by itself.
    - Otherwise `g = 0.0`. The comparisons are false for NaN.

    Mix:

    - For `0 ≤ t < n`: `y[t] = T(float64(x[t]) + g · float64(z[o_j + ((s + t) mod L_j)]))`. `z` is the noise bank;
      `o_j` and `L_j` are clip `j`'s offset and length in it. Product and sum are rounded separately, and there is one
      rounding to `T`.
    - `T` is float32 for float32 and int16 signals, and float64 for float64 signals.
    - When `g` is exactly `0.0` the utterance is copied. Float input goes byte for byte. int16 is widened.
    - A clip shorter than the utterance wraps as often as needed.
    - Float samples outside every utterance keep their values. For int16 input only the utterance spans are defined.
    - `+inf` anywhere is only promised not to disturb other utterances.

    So a silent or NaN utterance, a silent or NaN clip and an utterance not chosen are all copied.  `Pn` is the power of
    the whole clip (Kaldi's rule), computed once per device (:func:`clip_power`).  Refused with ``ValueError`` before
    any device work: a bad `snr_db` or `prob`, an empty bank or clip, mixed clip dtypes, a signal that is not a 1-D GPU
    tensor of the three dtypes, utterances outside the signal, a plan of the wrong length or with `clip` or `start`
    out of range, a batch needing more than 2^31 - 1 blocks.  Reverberation and speed perturbation are other stages;
    there is no streaming form, because the gain needs the whole utterance's energy.
    """

    aliases = {"add_noise", "additive_noise", "mix_noise"}

    def __init__(self, clips, snr_db=(5.0, 20.0), prob: float = 1.0, seed: Optional[int] = None):
        super().__init__()
        self.snr_db = self._check_snr(snr_db)
        if isinstance(prob, (bool, np.bool_)) or not isinstance(prob, numbers.Real) or not 0.0 <= float(prob) <= 1.0:
            raise ValueError(f"prob must lie in [0, 1], not {prob!r}")
        self.prob = float(prob)
        if isinstance(clips, (str, bytes, os.PathLike)) or not hasattr(clips, "__len__") or hasattr(clips, "dtype"):
            raise ValueError("clips must be a sequence of 1-D arrays, 1-D tensors or paths")
        if len(clips) == 0:
            raise ValueError("the noise bank is empty: clips must hold at least one clip")
        read = [self._read_clip(k, clip) for k, clip in enumerate(clips)]
        kinds = {clip.dtype for clip in read}
        if len(kinds) > 1:
            raise ValueError(f"the clips have mixed dtypes ({', '.join(sorted(str(kind) for kind in kinds))}): one of "
                             "float32, float64 or int16 for all")
        lengths = np.asarray([len(clip) for clip in read], dtype=np.int64)
        self._bank = np.ascontiguousarray(np.concatenate(read))
        self._clip_lengths = lengths
        self._clip_offsets = (np.cumsum(lengths) - lengths).astype(np.int64)
        for table in (self._bank, self._clip_lengths, self._clip_offsets):
            table.flags.writeable = False
        self._start_seed(seed)
        self._on_device = {}  # device index -> [bank, its table (offsets, lengths, chunk bases), Pn or None]

    @staticmethod
    def _check_snr(snr_db):
        def number(v):
            return isinstance(v, numbers.Real) and not isinstance(v, (bool, np.bool_)) and math.isfinite(float(v))

        if number(snr_db):
            return (float(snr_db), float(snr_db))
        try:
            lo, hi = snr_db
        except (TypeError, ValueError):
            raise ValueError(f"snr_db must be a finite number or a pair (lo, hi), not {snr_db!r}") from None
        if not (number(lo) and number(hi)) or float(lo) > float(hi):
            raise ValueError(f"snr_db must be a finite number or a pair (lo, hi) with lo <= hi, not {snr_db!r}")
        return (float(lo), float(hi))

    @staticmethod
    def _read_clip(k, clip):
        if isinstance(clip, (str, os.PathLike)):
            from .util import read_signal

            clip = read_signal(os.fspath(clip), dtype=None)
        elif hasattr(clip, "detach") and hasattr(clip, "cpu"):  # a tensor, wherever it lies
            clip = clip.detach().cpu().numpy()
        clip = np.asarray(clip)
        if clip.ndim != 1:
            raise ValueError(f"clip {k} has shape {tuple(clip.shape)}: a clip is 1-D")
        if clip.size == 0:
            raise ValueError(f"clip {k} is empty")
        if clip.dtype not in (np.float32, np.float64, np.int16):
            raise ValueError(f"clip {k} is {clip.dtype}: a clip is float32, float64 or int16")
        return clip

    num_clips = property(lambda self: len(self._clip_lengths), doc="K, the clips of the bank")
    clip_offsets = property(lambda self: self._clip_offsets, doc="int64 per clip: its first sample in the bank")
    clip_lengths = property(lambda self: self._clip_lengths, doc="int64 per clip: its samples")
    bank = property(lambda self: self._bank, doc="the clips back to back, in their dtype (host copy, read-only)")

    def __repr__(self) -> str:
        # (what the object was built with and nothing of where it lies: a test id made of it is the same in every run)
        return (f"AddNoise(clips=<{self.num_clips} of {self._bank.dtype}>, snr_db={self.snr_db!r}, prob={self.prob!r}, "
                f"seed={self._given_seed!r})")

    # -- the plan ---------------------------------------------------------------------------------------------------

    def plan(self, B: int, seeds=None, clips=None, snr_db=None) -> NoisePlan:
        """The plan of `B` utterances as numpy arrays: ``clip``, ``start``, ``snr_db``, ``ratio``, ``applied``

        With `seeds`, one integer per utterance, utterance b's plan is that of the first call of ``AddNoise(...,
        seed=seeds[b])`` and this object's sequence is not touched; with ``seeds=None`` the sequence advances `B`
        times.  `clips` and `snr_db`, one value per utterance, take the place of those draws (``start`` is still drawn,
        against the chosen clip's length).  :func:`apply_packed` applies a plan as given (``plan=``), so one plan can
        go on two views.
        """
        if isinstance(B, (bool, np.bool_)) or not isinstance(B, numbers.Integral) or B < 0:
            raise ValueError(f"B must be a non-negative integer, not {B!r}")
        B = int(B)
        given_clips = given_snr = None
        if clips is not None:
            given_clips = np.asarray(clips).reshape(-1)
            if len(given_clips) != B or (B and given_clips.dtype.kind not in "iu"):
                raise ValueError("clips: one clip index per utterance")
            given_clips = given_clips.astype(np.int64)
            if B and (given_clips.min() < 0 or given_clips.max() >= self.num_clips):
                raise ValueError(f"clips: an index outside [0, {self.num_clips})")
        if snr_db is not None:
            given_snr = np.asarray(snr_db, dtype=np.float64).reshape(-1)
            if len(given_snr) != B or not np.isfinite(given_snr).all():
                raise ValueError("snr_db: one finite value per utterance")
        x0, x1, x2, x3 = _philox_draws(self._keys(B, seeds), _MIX_COUNTER)
        clip = _mix_pick(x0, np.uint64(self.num_clips)) if given_clips is None else given_clips
        start = _mix_pick(x1, self._clip_lengths[clip].astype(np.uint64))
        lo, hi = self.snr_db
        # (every operation on float64 arrays rounds by itself; (hi - lo) is +0.0 where lo == hi, so snr is lo there)
        snr = (lo + (hi - lo) * (x2.astype(np.float64) * 2.0 ** -32)) if given_snr is None else given_snr
        applied = x3.astype(np.float64) * 2.0 ** -32 < self.prob
        # one scalar call per utterance: an array call may round differently
        ratio = np.fromiter((math.pow(10.0, float(v) / 10.0) for v in snr), dtype=np.float64, count=B)
        return NoisePlan(clip.astype(np.int64), start, np.asarray(snr, dtype=np.float64), ratio, applied)

    def _check_plan(self, plan, B: int) -> NoisePlan:
        try:
            clip, start, snr, ratio, applied = (np.asarray(v).reshape(-1) for v in plan)
        except (TypeError, ValueError):
            raise ValueError("plan must hold clip, start, snr_db, ratio and applied, as plan() returns them") from None
        if any(len(v) != B for v in (clip, start, snr, ratio, applied)):
            raise ValueError(f"the plan is not one of {B} utterances")
        if B and (clip.dtype.kind not in "iu" or start.dtype.kind not in "iu"):
            raise ValueError("the plan's clip and start are integers")
        clip, start = clip.astype(np.int64), start.astype(np.int64)
        if B and (clip.min() < 0 or clip.max() >= self.num_clips):
            raise ValueError(f"the plan names a clip outside [0, {self.num_clips})")
        if B and (start.min() < 0 or (start >= self._clip_lengths[clip]).any()):
            raise ValueError("the plan has a start outside its clip")
        return NoisePlan(clip, start, snr.astype(np.float64), ratio.astype(np.float64), applied.astype(bool))

    # -- the device side ----------------------------------------------------------------------------------------------

    _chunk_bases = staticmethod(_chunk_bases)  # (a module-level helper; tools/mix_rate.py calls it on the object)

    def _chunk_sums(self, torch, lib, signal, table, B, total):
        """the chunk sums of the B segments of `signal` that rows 0..2 of `table` (offsets, lengths, chunk bases) name"""
        partials = torch.empty((total,), dtype=torch.float64, device=signal.device)
        fn = getattr(lib, "pds_mix_chunk_energy_" + _suffix(signal.dtype))
        rc = fn(signal.data_ptr(), table[0].data_ptr(), table[1].data_ptr(), table[2].data_ptr(), B, total,
                partials.data_ptr(), torch.cuda.current_stream(signal.device).cuda_stream)
        _native.check_stages5(rc, "pds_mix_chunk_energy")
        return partials

    def _bank_on(self, device):
        torch = _native.require_device()
        key = torch.device(device).index if device is not None else None
        if key is None:
            key = torch.cuda.current_device()
        got = self._on_device.get(key)
        if got is None:
            dev = torch.device("cuda", key)
            bases, _ = self._chunk_bases(self._clip_lengths)
            table = np.stack([self._clip_offsets, self._clip_lengths, bases])
            got = self._on_device[key] = [torch.from_numpy(self._bank.copy()).to(dev), torch.from_numpy(table).to(dev),
                                          None]
        return got

    def clip_power(self, device=None):
        """float64 GPU tensor ``[K]``: the mean power `Pn` of every clip of the bank, computed once per device"""
        torch = _native.require_device()
        entry = self._bank_on(device)
        if entry[2] is None:
            lib = _native.stages5_lib()
            bank, table, _ = entry
            K = self.num_clips
            _, total = self._chunk_bases(self._clip_lengths)
            with torch.cuda.device(bank.device):
                partials = self._chunk_sums(torch, lib, bank, table, K, total)
                pn = torch.empty((K,), dtype=torch.float64, device=bank.device)
                rc = lib.pds_mix_gain(partials.data_ptr(), table[2].data_ptr(), table[1].data_ptr(), K, 1, None, None,
                                      None, None, 0, pn.data_ptr(), torch.cuda.current_stream(bank.device).cuda_stream)
                _native.check_stages5(rc, "pds_mix_gain")
            entry[2] = pn
        return entry[2]

    def energy_packed(self, signal, offsets, lengths):
        """float64 GPU tensor ``[B]``: the segment energy `E` of every utterance of a packed GPU buffer, as the
        definition sums it (utterance b is ``signal[offsets[b] : offsets[b] + lengths[b]]``)"""
        offs_h, lens_h, B = _check_packed(signal, offsets, lengths)
        bases, total = self._chunk_bases(lens_h)
        torch = _native.require_device()
        lib = _native.stages5_lib()
        signal = signal.contiguous()
        out = torch.empty((B,), dtype=torch.float64, device=signal.device)
        if not B:
            return out
        table = torch.as_tensor(np.stack([offs_h, lens_h, bases])).to(signal.device)
        with torch.cuda.device(signal.device):
            partials = self._chunk_sums(torch, lib, signal, table, B, total)
            rc = lib.pds_mix_gain(partials.data_ptr(), table[2].data_ptr(), table[1].data_ptr(), B, 0, None, None, None,
                                  None, 0, out.data_ptr(), torch.cuda.current_stream(signal.device).cuda_stream)
            _native.check_stages5(rc, "pds_mix_gain")
        return out

    def apply_packed(self, signal, offsets, lengths, seeds=None, plan=None, return_gains: bool = False):
        """Mix noise into every utterance of a packed GPU buffer (see ``compute_packed``): three launches, one upload,
        no synchronisation

        `signal`: a 1-D GPU tensor of float32, float64 or int16 (16-bit PCM is widened on the device, exactly, and
        gives a float32 result); utterance b is ``signal[offsets[b] : offsets[b] + lengths[b]]``.  `seeds` as for
        :func:`plan`; a `plan` is applied as given (and no seed is used).  Returns a new tensor of `signal`'s length;
        with `return_gains` also the float64 gains ``[B]`` on the device.  For float input, samples outside every
        utterance keep their values; for int16 input only the utterance spans are defined.
        """
        import torch

        offs_h, lens_h, B = _check_packed(signal, offsets, lengths)
        if plan is None:
            if seeds is not None and len(seeds) != B:
                raise ValueError("one seed per utterance")
        else:
            plan = self._check_plan(plan, B)
        bases, total = self._chunk_bases(lens_h)
        calls = _apply_calls(lens_h)
        if plan is None:
            plan = self.plan(B, seeds=seeds)
        torch = _native.require_device()
        lib = _native.stages5_lib()
        signal = signal.contiguous()
        if signal.dtype == torch.int16:
            out = torch.empty(signal.shape, dtype=torch.float32, device=signal.device)
        elif B and np.array_equal(offs_h, np.cumsum(lens_h) - lens_h) and int(lens_h.sum()) == signal.numel():
            out = torch.empty_like(signal)  # (the utterances cover the buffer: every sample is written)
        else:
            out = signal.clone()  # gaps between utterances keep their contents
        gains = torch.empty((B,), dtype=torch.float64, device=signal.device)
        if not B:
            return (out, gains) if return_gains else out
        bank, bank_table, _ = self._bank_on(signal.device)
        pn = self.clip_power(signal.device)
        # everything the kernels need of the batch goes up in one copy (a ratio's bits travel as int64)
        table = torch.as_tensor(np.stack([
            offs_h, lens_h, bases, self._clip_offsets[plan.clip], self._clip_lengths[plan.clip], plan.start,
            np.ascontiguousarray(plan.ratio).view(np.int64), plan.applied.astype(np.int64), plan.clip,
        ])).to(signal.device)
        fn = getattr(lib, f"pds_mix_apply_{_suffix(signal.dtype)}_{_suffix(bank.dtype)}")
        with torch.cuda.device(signal.device):
            stream = torch.cuda.current_stream(signal.device).cuda_stream
            partials = self._chunk_sums(torch, lib, signal, table, B, total)
            rc = lib.pds_mix_gain(partials.data_ptr(), table[2].data_ptr(), table[1].data_ptr(), B, 2, table[8].data_ptr(),
                                  table[6].data_ptr(), table[7].data_ptr(), pn.data_ptr(), self.num_clips,
                                  gains.data_ptr(), stream)
            _native.check_stages5(rc, "pds_mix_gain")
            for lo, hi, longest in calls:
                rc = fn(signal.data_ptr(), table[0, lo:].data_ptr(), table[1, lo:].data_ptr(), bank.data_ptr(),
                        table[3, lo:].data_ptr(), table[4, lo:].data_ptr(), table[5, lo:].data_ptr(),
                        gains[lo:].data_ptr(), hi - lo, longest, out.data_ptr(), stream)
                _native.check_stages5(rc, "pds_mix_apply")
        return (out, gains) if return_gains else out

    def apply(self, signal, axis: Optional[int] = None, in_place: bool = False):
        """Noise on a signal, or on every vector along `axis` (default: the last) of an array of more dimensions

        A 1-D signal is one utterance; with more dimensions every vector along `axis` is an utterance of its own draw,
        and the seed sequence advances once per vector, in C order of the other axes.  numpy arrays go to the device
        and come back in their dtype; GPU tensors stay (float32 and float64 as they are, any other dtype through
        float64).
        """
        t, was_gpu, dtype = _device_copy(signal)
        if t.dim() == 0:
            raise ValueError("AddNoise applies to signals of at least one dimension")
        if t.numel() == 0:
            return _finish(t.clone(), was_gpu, dtype, signal, in_place)
        ax = t.dim() - 1 if axis is None else int(axis) % t.dim()
        work = t.movedim(ax, -1).contiguous()
        n = work.shape[-1]
        rows = work.numel() // n
        out = self.apply_packed(work.reshape(-1), np.arange(rows, dtype=np.int64) * n, np.full(rows, n, dtype=np.int64))
        out = out.reshape(work.shape).movedim(-1, ax)
        if was_gpu and in_place and out.dtype == signal.dtype:
            signal.copy_(out)
            return signal
        return _finish(out.contiguous(), was_gpu, dtype, signal, in_place)


# ---- Reverb -----------------------------------------------------------------------------------------------------------

_REVERB_BLOCK, _REVERB_FFT = 512, 1024  # taps of a partition, points of a transform (csrc/reverb_rule.h)
_REVERB_MAX_TAPS = 1 << 20  # taps of a room impulse response (REVERB_MAX_TAPS)
_REVERB_HALVES = 8  # units of a block of the transform kernels (REVERB_HALVES)
_REVERB_MAX_BLOCKS = (1 << 31) - 1  # blocks of one launch (REVERB_MAX_BLOCKS)
_REVERB_COUNTER = (0, 0, 0, 0x52495231)  # the counter of the plan's Philox block (REVERB_COUNTER_0 .. REVERB_COUNTER_3)


def _reverb_even(units):
    return (units + 1) & ~np.int64(1)


class ReverbPlan(NamedTuple):
    """What :func:`Reverb.plan` draws, one entry per utterance"""

    rir: np.ndarray  #: int64, the room impulse response of the bank
    applied: np.ndarray  #: bool, whether the utterance is reverberated at all


class Reverb(_Seeded, PreProcessor):
    """Convolve a room impulse response of a bank with every utterance: the reverberation half of Kaldi's
    ``wav-reverberate --impulse-response --shift-output --normalize-output`` (aliases ``reverb``, ``reverberate``,
    ``rir``)

    `rirs` is a non-empty sequence of room impulse responses, each a 1-D array, a 1-D tensor or a path that the readers
    of ``util.read_signal`` take (wav, npy, npz, pt), float32, float64 or int16.  `prob` in ``[0, 1]`` is the share of
    utterances that are reverberated at all; `seed` is as ``Dither``'s: an utterance's key comes from
    :func:`dither_keys`, and with ``seeds=None`` the object's own sequence advances once per utterance.

    The definition.

    Bank:

    - `K` room impulse responses (RIRs), each one channel of `1 ≤ L_j ≤ 2²⁰` taps, float32, float64 or int16.
    - Partition size is `B = 512` taps and transform size is `N = 1024`, so `P_j = ceil(L_j / 512)`.
    - The partition spectra are built on the host in float64: `H_{j,p} = fft(taps[512p : 512p+512]` zero-padded to
      1024`)`. Each spectrum is rounded once to complex64, uploaded once per device and cached.
    - The peak is `d_j = ` the first index of `max |h_j[k]|` when `shift_output` is set, else `0`. The taps are compared
      as float64.

    Plan of utterance `b`, built on the host in integers and float64:

    - One Philox4x32-10 block: key = the utterance's 64-bit key from `pre.dither_keys` (low word, high word), counter =
      `(0, 0, 0, 0x52495231)`. The fourth word differs from `dither_noise.h`, `specaug_rule.h` and `mix_rule.h`.
    - RIR `j = (uint64(x0) · K) >> 32`.
    - `applied = float64(x3) · 2⁻³² < prob`.

    Wet signal, float32 whatever the sample dtype:

    - With `x` zero outside `[0, n)`, `y_full[τ] = Σ_k h[k]·x[τ−k]` and `wet[t] = y_full[t + d]` for `0 ≤ t < n`. The
      reverberant tail past the last sample is dropped.
    - It is evaluated by uniformly partitioned overlap-save in float32. The blocks of `y_full` stand on multiples of 512
      of `τ`, anchored at the utterance's own first sample, not at the buffer's.
    - float64 samples are rounded to float32 at the load. int16 samples are widened.
    - A RIR with exactly one non-zero tap `g` at `k0` is a delay and a gain. No transform is taken:
      `wet[t] = float32(g)·x[t + d − k0]`, one float32 product, `+0.0` where `t + d − k0` lies outside `[0, n)`. A unit
      impulse therefore returns the samples as loaded.
    - Independence: an utterance's wet bytes depend on its samples, the RIR and the parameters alone, not on the batch it
      stands in, its offset in the buffer (aligned or not), its neighbours or the launch. The summation order over `p` is
      fixed and there are no atomics.
    - Locality: take `τ` in the block beginning at `b0 = 512·floor(τ/512)`. `wet` at `τ − d` depends, round-off
      included, only on input samples `b0 − 512·(P+2) ≤ i < b0 + 1536`. Two adjacent real blocks are packed into one
      complex transform: `ifft(fft(a + i·b)·H) = a⊛h + i·(b⊛h)`. Where that window holds no non-zero sample, the output
      is exactly `±0.0`.

    Normalisation (`normalize_output`):

    - `Ps` is the mean power of the utterance's samples in their own dtype, `Py` that of the float32 wet signal. Both are
      the segment energy `E(·, n) / n` of `pds_amd_stages5.h`: the same chunks, lanes and tree.
    - If `Ps > 0` and `Py > 0`, then `out[t] = float32(float64(wet[t]) · c)` with `c = sqrt(Ps / Py)`. The quotient, the
      root and the product are each rounded by themselves.
    - Otherwise the wet signal stands as it is. The comparisons are false for NaN.

    Not applied: a float32 utterance is copied byte for byte, with NaN payloads and signed zeros intact. int16 is widened.
    float64 is rounded once.

    Gaps and bad samples:

    - Float32 samples outside every utterance keep their bytes. For int16 and float64 input only the utterance spans are
      defined.
    - A NaN or infinite sample spoils only the outputs whose window holds it. With `normalize_output` it spoils its own
      utterance's scale. It never spoils another utterance.

    In a chain with :class:`AddNoise`, ``Reverb`` goes first: ``AddNoise``'s `Ps` is then the reverberated signal's
    power (Kaldi's early-reverberation energy rule for the SNR is not implemented).  There is no streaming form, because
    the scale needs the whole utterance; a ``StreamBatch`` handed a ``Reverb`` raises ``TypeError``.  Refused with
    ``ValueError`` before any device work: a bad `prob`, an empty bank, an empty, multi-channel or too long RIR, a signal
    that is not a 1-D GPU tensor of the three dtypes, utterances outside the signal, a plan of the wrong length or with
    `rir` out of range, a batch needing more than 2^31 - 1 blocks.
    """

    aliases = {"reverb", "reverberate", "rir"}

    def __init__(self, rirs, prob: float = 1.0, shift_output: bool = True, normalize_output: bool = True,
                 seed: Optional[int] = None):
        super().__init__()
        if isinstance(prob, (bool, np.bool_)) or not isinstance(prob, numbers.Real) or not 0.0 <= float(prob) <= 1.0:
            raise ValueError(f"prob must lie in [0, 1], not {prob!r}")
        self.prob = float(prob)
        self.shift_output = bool(shift_output)
        self.normalize_output = bool(normalize_output)
        if isinstance(rirs, (str, bytes, os.PathLike)) or not hasattr(rirs, "__len__") or hasattr(rirs, "dtype"):
            raise ValueError("rirs must be a sequence of 1-D arrays, 1-D tensors or paths")
        if len(rirs) == 0:
            raise ValueError("the bank is empty: rirs must hold at least one room impulse response")
        self._taps = [self._read_rir(k, rir) for k, rir in enumerate(rirs)]
        self._rir_lengths = np.asarray([len(t) for t in self._taps], dtype=np.int64)
        self._rir_peaks = np.asarray([self.peak_of(t) if self.shift_output else 0 for t in self._taps], dtype=np.int64)
        self._rir_parts = -(-self._rir_lengths // _REVERB_BLOCK)
        self._rir_bases = (np.cumsum(self._rir_parts) - self._rir_parts).astype(np.int64)
        # a response of one non-zero tap is a delay and a gain: its index (else -1) and the tap as float32
        single = [np.flatnonzero(t) if np.count_nonzero(t) == 1 else None for t in self._taps]
        self._rir_taps = np.asarray([-1 if k is None else int(k[0]) for k in single], dtype=np.int64)
        self._rir_gains = np.asarray([0.0 if k is None else t[int(k[0])] for k, t in zip(single, self._taps)],
                                     dtype=np.float32)
        for table in (self._rir_lengths, self._rir_peaks, self._rir_parts, self._rir_bases, self._rir_taps,
                      self._rir_gains, *self._taps):
            table.flags.writeable = False
        self._spectra = None  # complex64 [sum of P_j, 1024], built at the first use
        self._start_seed(seed)
        self._on_device = {}  # device index -> (spectra, table (bases, partitions, peaks), twiddles)

    @staticmethod
    def _read_rir(k, rir):
        if isinstance(rir, (str, os.PathLike)):
            from .util import read_signal

            rir = read_signal(os.fspath(rir), dtype=None)
        elif hasattr(rir, "detach") and hasattr(rir, "cpu"):  # a tensor, wherever it lies
            rir = rir.detach().cpu().numpy()
        rir = np.asarray(rir)
        if rir.ndim != 1:
            raise ValueError(f"RIR {k} has shape {tuple(rir.shape)}: a room impulse response is one channel, 1-D")
        if rir.size == 0:
            raise ValueError(f"RIR {k} is empty")
        if rir.size > _REVERB_MAX_TAPS:
            raise ValueError(f"RIR {k} has {rir.size} taps: at most 2^20")
        if rir.dtype not in (np.float32, np.float64, np.int16):
            raise ValueError(f"RIR {k} is {rir.dtype}: a room impulse response is float32, float64 or int16")
        return np.array(rir, dtype=np.float64)

    @staticmethod
    def peak_of(taps) -> int:
        """the first index of ``max |h[k]|``, the taps compared as float64"""
        return int(np.argmax(np.abs(np.asarray(taps, dtype=np.float64))))

    @staticmethod
    def partition_spectra(taps) -> np.ndarray:
        """complex64 ``[P, 1024]``: the spectra of the partitions of 512 taps, formed in float64, rounded once"""
        taps = np.asarray(taps, dtype=np.float64)
        parts = -(-len(taps) // _REVERB_BLOCK)
        padded = np.zeros(parts * _REVERB_BLOCK, dtype=np.float64)
        padded[: len(taps)] = taps
        return np.fft.fft(padded.reshape(parts, _REVERB_BLOCK), n=_REVERB_FFT, axis=1).astype(np.complex64)

    num_rirs = property(lambda self: len(self._rir_lengths), doc="K, the room impulse responses of the bank")
    rir_lengths = property(lambda self: self._rir_lengths, doc="int64 per RIR: its taps")
    rir_peaks = property(lambda self: self._rir_peaks, doc="int64 per RIR: d, the shift of the output (0 without it)")
    rir_partitions = property(lambda self: self._rir_parts, doc="int64 per RIR: P, its partitions of 512 taps")

    def __repr__(self) -> str:
        # (what the object was built with and nothing of where it lies: a test id made of it is the same in every run)
        return (f"Reverb(rirs=<{self.num_rirs}>, prob={self.prob!r}, shift_output={self.shift_output!r}, "
                f"normalize_output={self.normalize_output!r}, seed={self._given_seed!r})")

    # -- the plan ---------------------------------------------------------------------------------------------------

    def plan(self, B: int, seeds=None, rirs=None) -> ReverbPlan:
        """The plan of `B` utterances as numpy arrays: ``rir`` and ``applied``

        With `seeds`, one integer per utterance, utterance b's plan is that of the first call of ``Reverb(...,
        seed=seeds[b])`` and this object's sequence is not touched; with ``seeds=None`` the sequence advances `B` times.
        `rirs`, one index per utterance, takes the place of that draw.  :func:`apply_packed` applies a plan as given
        (``plan=``), so one plan can go on two views.
        """
        if isinstance(B, (bool, np.bool_)) or not isinstance(B, numbers.Integral) or B < 0:
            raise ValueError(f"B must be a non-negative integer, not {B!r}")
        B = int(B)
        given = None
        if rirs is not None:
            given = np.asarray(rirs).reshape(-1)
            if len(given) != B or (B and given.dtype.kind not in "iu"):
                raise ValueError("rirs: one index per utterance")
            given = given.astype(np.int64)
            if B and (given.min() < 0 or given.max() >= self.num_rirs):
                raise ValueError(f"rirs: an index outside [0, {self.num_rirs})")
        x0, _, _, x3 = _philox_draws(self._keys(B, seeds), _REVERB_COUNTER)
        rir = ((x0 * np.uint64(self.num_rirs)) >> _S32).astype(np.int64) if given is None else given
        applied = x3.astype(np.float64) * 2.0 ** -32 < self.prob
        return ReverbPlan(rir, applied)

    def _check_plan(self, plan, B: int) -> ReverbPlan:
        try:
            rir, applied = (np.asarray(v).reshape(-1) for v in plan)
        except (TypeError, ValueError):
            raise ValueError("plan must hold rir and applied, as plan() returns them") from None
        if len(rir) != B or len(applied) != B:
            raise ValueError(f"the plan is not one of {B} utterances")
        if B and rir.dtype.kind not in "iu":
            raise ValueError("the plan's rir is an integer")
        rir = rir.astype(np.int64)
        if B and (rir.min() < 0 or rir.max() >= self.num_rirs):
            raise ValueError(f"the plan names a RIR outside [0, {self.num_rirs})")
        return ReverbPlan(rir, applied.astype(bool))

    # -- the device side ----------------------------------------------------------------------------------------------

    def layout(self, lengths, plan):
        """(spectra base per utterance, spectra slots in all, convolve unit base, convolve units in all) of a batch, as
        csrc/reverb_rule.h counts them; ``ValueError`` where a launch would need more than 2^31 - 1 blocks"""
        n = np.asarray(lengths, dtype=np.int64).reshape(-1)
        applied = np.asarray(plan.applied, dtype=bool) & (self._rir_taps[plan.rir] < 0)  # (transformed)
        d = self._rir_peaks[plan.rir] if len(n) else np.zeros(0, np.int64)
        some = n > 0
        last = np.where(some, (n - 1) // _REVERB_BLOCK + 1, 0)
        spec = np.where(some & applied, _reverb_even(last + 2), 0).astype(np.int64)
        pairs = np.where(some, (d + n - 1) // _REVERB_FFT - d // _REVERB_FFT + 1, 0)
        copies = -(-n // _REVERB_FFT)
        units = np.where(some, _reverb_even(np.where(applied, pairs, copies)), 0).astype(np.int64)
        spec_total, unit_total = int(spec.sum()), int(units.sum())
        if max(spec_total, unit_total) > _REVERB_MAX_BLOCKS * _REVERB_HALVES:
            raise ValueError("the batch needs more than 2^31 - 1 blocks in one launch: split it")
        return (np.cumsum(spec) - spec).astype(np.int64), spec_total, (np.cumsum(units) - units).astype(np.int64), unit_total

    def spectra(self) -> np.ndarray:
        """complex64 ``[sum of P_j, 1024]``: the bank's partition spectra, RIR j's from row ``cumsum(P)[j] - P[j]``"""
        if self._spectra is None:
            self._spectra = np.concatenate([self.partition_spectra(t) for t in self._taps])
            self._spectra.flags.writeable = False
        return self._spectra

    def _bank_on(self, device):
        torch = _native.require_device()
        key = torch.device(device).index if device is not None else None
        if key is None:
            key = torch.cuda.current_device()
        got = self._on_device.get(key)
        if got is None:
            dev = torch.device("cuda", key)
            lib = _native.stages6_lib()
            tw = np.empty(2 * _REVERB_FFT, dtype=np.float32)
            _native.check_stages6(lib.pds_reverb_twiddles(tw.ctypes.data), "pds_reverb_twiddles")
            table = np.stack([self._rir_bases, self._rir_parts, self._rir_peaks, self._rir_taps])
            spectra = torch.from_numpy(np.ascontiguousarray(self.spectra()).view(np.float32).copy())
            got = self._on_device[key] = (spectra.to(dev), torch.from_numpy(table).to(dev), torch.from_numpy(tw).to(dev),
                                          torch.from_numpy(self._rir_gains.copy()).to(dev))
        return got

    def workspace_bytes(self, lengths, plan) -> int:
        """bytes of the spectra workspace :func:`apply_packed` allocates for a batch"""
        return self.layout(lengths, plan)[1] * _REVERB_FFT * 8

    def apply_packed(self, signal, offsets, lengths, seeds=None, plan=None, return_wet: bool = False):
        """Reverberate every utterance of a packed GPU buffer (see ``compute_packed``): one upload of one table, no
        synchronisation

        `signal`: a 1-D GPU tensor of float32, float64 or int16; utterance b is ``signal[offsets[b] : offsets[b] +
        lengths[b]]``.  `seeds` as for :func:`plan`; a `plan` is applied as given (and no seed is used).  Returns a new
        float32 tensor of `signal`'s length; with `return_wet` also the wet signal before the normalisation (the same
        layout; the output itself without `normalize_output`).  For float32 input, samples outside every utterance keep
        their bytes; for int16 and float64 input only the utterance spans are defined.
        """
        import torch

        offs_h, lens_h, B = _check_packed(signal, offsets, lengths)
        if plan is None:
            if seeds is not None and len(seeds) != B:
                raise ValueError("one seed per utterance")
        else:
            plan = self._check_plan(plan, B)
        chunk_bases, chunk_total = _chunk_bases(lens_h)
        scale_calls = _apply_calls(lens_h) if B else []
        if plan is None:
            plan = self.plan(B, seeds=seeds)
        spec_base, spec_total, unit_base, unit_total = self.layout(lens_h, plan)
        torch = _native.require_device()
        lib = _native.stages6_lib()
        signal = signal.contiguous()
        if signal.dtype != torch.float32:
            out = torch.empty(signal.shape, dtype=torch.float32, device=signal.device)
        elif B and np.array_equal(offs_h, np.cumsum(lens_h) - lens_h) and int(lens_h.sum()) == signal.numel():
            out = torch.empty_like(signal)  # (the utterances cover the buffer: every sample is written)
        else:
            out = signal.clone()  # gaps between utterances keep their contents
        if not B or not unit_total:
            return (out, out.clone()) if return_wet else out
        h, bank_table, tw, tap_gains = self._bank_on(signal.device)
        transformed = plan.applied & (self._rir_taps[plan.rir] < 0)
        normalise = self.normalize_output and bool(plan.applied.any())
        # everything the kernels need of the batch goes up in one copy (the ratio 1.0 travels as its bits)
        table = torch.as_tensor(np.stack([
            offs_h, lens_h, np.where(plan.applied, plan.rir, -1).astype(np.int64), spec_base, unit_base, chunk_bases,
            np.arange(B, dtype=np.int64), np.full(B, 1.0).view(np.int64), plan.applied.astype(np.int64),
            np.where(transformed, plan.rir, -1).astype(np.int64),
        ])).to(signal.device)
        xtype = {"f32": 0, "f64": 1, "i16": 2}[_suffix(signal.dtype)]
        with torch.cuda.device(signal.device):
            stream = torch.cuda.current_stream(signal.device).cuda_stream
            ws = None
            if spec_total:
                ws = torch.empty((spec_total * _REVERB_FFT * 2,), dtype=torch.float32, device=signal.device)
                fn = getattr(lib, "pds_reverb_spectra_" + _suffix(signal.dtype))
                rc = fn(signal.data_ptr(), table[0].data_ptr(), table[1].data_ptr(), table[9].data_ptr(),
                        table[3].data_ptr(), B, spec_total, tw.data_ptr(), ws.data_ptr(), stream)
                _native.check_stages6(rc, "pds_reverb_spectra")
            rc = lib.pds_reverb_convolve(signal.data_ptr(), xtype, table[0].data_ptr(), table[1].data_ptr(),
                                         table[2].data_ptr(), table[3].data_ptr(), table[4].data_ptr(), B, unit_total,
                                         ws.data_ptr() if ws is not None else None, h.data_ptr(),
                                         bank_table[0].data_ptr(), bank_table[1].data_ptr(), bank_table[2].data_ptr(),
                                         bank_table[3].data_ptr(), tap_gains.data_ptr(), self.num_rirs, tw.data_ptr(), out.data_ptr(), stream)
            _native.check_stages6(rc, "pds_reverb_convolve")
            wet = out.clone() if return_wet else None
            if normalise:
                mix = _native.stages5_lib()
                energy = (table[0], table[1], table[5])

                def power(x, mode, pn):
                    partials = torch.empty((chunk_total,), dtype=torch.float64, device=x.device)
                    fn = getattr(mix, "pds_mix_chunk_energy_" + _suffix(x.dtype))
                    rc = fn(x.data_ptr(), energy[0].data_ptr(), energy[1].data_ptr(), energy[2].data_ptr(), B,
                            chunk_total, partials.data_ptr(), stream)
                    _native.check_stages5(rc, "pds_mix_chunk_energy")
                    res = torch.empty((B,), dtype=torch.float64, device=x.device)
                    rc = mix.pds_mix_gain(partials.data_ptr(), energy[2].data_ptr(), energy[1].data_ptr(), B, mode,
                                          table[6].data_ptr() if mode == 2 else None,
                                          table[7].view(torch.float64).data_ptr() if mode == 2 else None,
                                          table[8].data_ptr() if mode == 2 else None,
                                          pn.data_ptr() if mode == 2 else None, B if mode == 2 else 0, res.data_ptr(),
                                          stream)
                    _native.check_stages5(rc, "pds_mix_gain")
                    return res

                py = power(out, 1, None)
                gains = power(signal, 2, py)  # sqrt(Ps / (Py * 1.0)) where applied, Ps > 0 and Py > 0, else 0.0
                for lo, hi, longest in scale_calls:
                    rc = lib.pds_reverb_scale(out.data_ptr(), table[0, lo:].data_ptr(), table[1, lo:].data_ptr(),
                                              gains[lo:].data_ptr(), hi - lo, longest, stream)
                    _native.check_stages6(rc, "pds_reverb_scale")
        return (out, wet) if return_wet else out

    def apply(self, signal, axis: Optional[int] = None, in_place: bool = False):
        """Reverberation of a signal, or of every vector along `axis` (default: the last) of an array of more
        dimensions

        A 1-D signal is one utterance; with more dimensions every vector along `axis` is an utterance of its own draw,
        and the seed sequence advances once per vector, in C order of the other axes.  numpy arrays go to the device and
        come back in their dtype; GPU tensors stay, and the result is float32 (float32 and float64 samples as they are,
        any other dtype through float64).
        """
        t, was_gpu, dtype = _device_copy(signal)
        if t.dim() == 0:
            raise ValueError("Reverb applies to signals of at least one dimension")
        if t.numel() == 0:
            return _finish(t.clone(), was_gpu, dtype, signal, in_place)
        ax = t.dim() - 1 if axis is None else int(axis) % t.dim()
        work = t.movedim(ax, -1).contiguous()
        n = work.shape[-1]
        rows = work.numel() // n
        out = self.apply_packed(work.reshape(-1), np.arange(rows, dtype=np.int64) * n, np.full(rows, n, dtype=np.int64))
        out = out.reshape(work.shape).movedim(-1, ax)
        if was_gpu and in_place and out.dtype == signal.dtype:
            signal.copy_(out)
            return signal
        return _finish(out.contiguous(), was_gpu, dtype, signal, in_place)
