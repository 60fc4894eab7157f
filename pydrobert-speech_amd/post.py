"""Post-processors on the hot path: ``Deltas``, ``Standardize`` / ``CMVN``, ``Cepstra``, ``SlidingCMVN``, ``EnergyVAD``,
``PCEN``, ``SpecAugment``, ``PLP``.

Same classes, aliases, arguments and error behaviour as the reference's (post.py:38-491);
the element-wise and stencil arithmetic runs in HIP kernels (``csrc/post.hip``) -- there
is no CPU path.  Host code only decides shapes, pads for the non-default ``pad_mode`` s,
and finalises the ``O(num_coeffs)`` mean/scale vectors of CMVN.

``Cepstra`` is not in the reference: the DCT-II and lifter that turn log filter-bank outputs into cepstral
coefficients (MFCCs), one HIP kernel over the rows with the matrix built on the host in float64.

``SlidingCMVN`` is not in the reference either: mean (and variance) normalisation over a sliding window of frames,
Kaldi's ``apply-cmvn-sliding``, one HIP kernel of the stages library (``csrc/sliding.hip``) over a packed ragged batch.

``EnergyVAD`` is not in the reference either: Kaldi's energy-based voiced-frame decision (``compute-vad-energy``) and
the selection of the voiced rows (``select-voiced-frames``), two HIP kernels of the stages library (``csrc/vad.hip``)
over a packed ragged batch.

``PCEN`` is not in the reference either: per-channel energy normalisation of linear filter-bank energies, a one-pole
smoother per column and a root compression, two HIP kernels of the second stages library (``csrc/pcen.hip``) over a
packed ragged batch.

``SpecAugment`` is not in the reference either: a time warp, frequency masks and time masks over the feature matrix
for training, drawn from a counter-based generator keyed per utterance, three HIP kernels of the third stages library
(``csrc/specaug.hip``) over a packed ragged batch.

``PLP`` is not in the reference either: perceptual linear prediction cepstra of linear filter-bank energies, Kaldi's
third feature type, row by row in one HIP kernel of the fourth stages library (``csrc/plp.hip``).

``Stack`` moves data only: views for a single tensor, one copy
kernel for a packed ragged batch.  CMVN statistics files (``rfilename``, ``save``) go through
``util.read_signal`` / numpy.
"""
import abc
import math
import warnings
from typing import Callable, Optional, Tuple, Union

import numpy as np

from . import _native
from . import pre as _pre
from .alias import AliasedFactory

__all__ = ["CMVN", "Cepstra", "Deltas", "EnergyVAD", "PCEN", "PLP", "PostProcessor", "SlidingCMVN", "SpecAugment",
           "Stack", "Standardize"]


class PostProcessor(AliasedFactory):
    """A transform applied to a feature tensor (reference post.py:38-63)"""

    @abc.abstractmethod
    def apply(self, features: np.ndarray, axis: int = -1, in_place: bool = False) -> np.ndarray:
        pass


def _is_gpu_tensor(x) -> bool:
    return bool(getattr(x, "is_cuda", False))


def _to_device(array: np.ndarray):
    torch = _native.require_device()
    return torch.from_numpy(np.ascontiguousarray(array)).to("cuda")


def _stream(torch, tensor):
    return torch.cuda.current_stream(tensor.device).cuda_stream


_ROWS_META = {}  # device copies of the ragged-row descriptions used most recently (insertion-ordered)
_ROWS_META_ENTRIES = 64


def _rows_meta(row_offsets, device):
    """Device ``int64[2][B]`` (first row, row count) of a packed ragged batch + host row counts

    Repeated calls with the same `row_offsets` (a pipeline processing batch after batch of a few
    geometries) reuse the device copy instead of a host-to-device transfer per launch.
    """
    torch = _native.require_device()
    rows = np.ascontiguousarray(row_offsets, dtype=np.int64)
    key = (rows.tobytes(), str(device))
    hit = _ROWS_META.pop(key, None)
    if hit is None:
        nrows = np.diff(rows)
        hit = (torch.from_numpy(np.stack([rows[:-1], nrows])).to(device), nrows)
        while len(_ROWS_META) >= _ROWS_META_ENTRIES:
            _ROWS_META.pop(next(iter(_ROWS_META)))  # the least recently used
    _ROWS_META[key] = hit  # (re-)inserted as the most recent
    return hit


# ------------------------------------------------------------------ Standardize ------


class Standardize(PostProcessor):
    """Zero mean (and unit variance) per coefficient; always returns float64

    `axis` of :func:`apply` / :func:`accumulate` is the *coefficient* axis; statistics run
    over every other axis.  Without accumulated statistics the tensor's own are used
    (reference post.py:66-305).  Sums and the normalisation run on the GPU in float64.
    """

    aliases = {"standardize", "normalize", "unit", "cmvn"}

    def __init__(self, rfilename: Optional[str] = None, norm_var: bool = True, **kwargs):
        self._stats = None  # float64 [2, C + 1]: sums | count, sums of squares | unused
        self._norm_var = bool(norm_var)
        if rfilename is None:
            if kwargs:
                raise TypeError("Invalid keyword arguments: {}".format(tuple(kwargs)))
            return
        # Statistics written by save() or by Kaldi's compute-cmvn-stats (reference
        # post.py:104-122): read with util.read_signal; keyword arguments go to the reader.
        from .util import read_signal

        if "dtype" in kwargs:
            self._stats = read_signal(rfilename, **kwargs)
            return
        for guess in (np.float64, np.float32, "dm", "fm"):
            try:
                self._stats = read_signal(rfilename, dtype=guess, **kwargs)
                break
            except (IOError, ValueError, ImportError, TypeError):
                continue
        if self._stats is None:
            raise IOError("Unable to load stats from {}".format(rfilename))
        if self._stats.ndim == 1:
            self._stats = self._two_rows(self._stats)

    @staticmethod
    def _two_rows(flat):
        """Raw binary statistics -> ``[2, C + 1]`` float64 (reference post.py:124-152)

        A headerless file does not say whether it holds float64 or float32 words.  A valid
        table has an integral count in ``[0, -1]`` and no negative entry; if the first
        interpretation fails that test the same bytes are tried as the other float width.
        """

        def plausible(table):
            return bool(np.isclose(np.round(table[0, -1]), table[0, -1]) and np.all(table >= 0))

        if flat.dtype not in (np.float32, np.float64):
            raise ValueError(
                "Statistics were loaded with a weird data type ({}) and are invalid. Make sure "
                "the arguments you passed to the init are correct".format(flat.dtype)
            )
        other = np.float32 if flat.dtype == np.float64 else np.float64
        for words in (flat, np.frombuffer(flat.tobytes(), dtype=other).astype(np.float64)):
            if words.size and words.size % 2 == 0:
                table = words.reshape(2, -1)
                if plausible(table):
                    return table
        raise IOError(
            "Could not properly load statistics. Try specifying additional parameters in init "
            "(see docstring)"
        )

    def save(self, wfilename: str, key: Optional[str] = None, compress: bool = False,
             overwrite: bool = True) -> None:
        """Write the accumulated statistics (reference post.py:307-361)

        ``.npy``: :func:`numpy.save`.  ``.npz``: an archive entry named `key` (default: the first
        free ``arr_<n>``), next to the archive's existing entries when `overwrite` is true (the
        reference's flag reads that way round, post.py:349-353), compressed on request.  Any
        other name: raw float64 words (:meth:`numpy.ndarray.tofile`).
        """
        if not self.have_stats:
            raise ValueError("No stats have been accumulated to save")
        if wfilename.endswith(".npy"):
            np.save(wfilename, self._stats)
        elif wfilename.endswith(".npz"):
            entries = {}
            if overwrite:
                try:
                    with np.load(wfilename) as archive:
                        entries = {name: archive[name] for name in archive.files}
                except IOError:
                    pass
            if key is None:
                n = 0
                while "arr_{}".format(n) in entries:
                    n += 1
                key = "arr_{}".format(n)
            entries[key] = self._stats
            (np.savez_compressed if compress else np.savez)(wfilename, **entries)
        else:
            self._stats.tofile(wfilename)

    @property
    def have_stats(self) -> bool:
        return self._stats is not None and self._stats[0, -1]

    # -- device helpers -----------------------------------------------------------------

    @staticmethod
    def _as_device_3d(features, axis):
        # view as [outer, coeff, inner] on the GPU in float32 or float64
        torch = _native.require_device()
        if _is_gpu_tensor(features):
            t = features
            if t.dtype not in (torch.float32, torch.float64):
                t = t.to(torch.float64)
        else:
            arr = np.asarray(features)
            if arr.dtype not in (np.float32, np.float64):
                arr = arr.astype(np.float64)
            t = _to_device(arr)
        t = t.contiguous()
        shape = tuple(t.shape)
        axis = axis % len(shape)
        outer = int(np.prod(shape[:axis], dtype=np.int64))
        inner = int(np.prod(shape[axis + 1 :], dtype=np.int64))
        return t, outer, shape[axis], inner

    @staticmethod
    def _device_sums(t, outer, C, inner):
        torch = _native.require_device()
        lib = _native.lib()
        stats = torch.empty(2 * C, dtype=torch.float64, device=t.device)
        scratch = torch.empty(
            int(lib.pds_cmvn_scratch_len(C, inner)), dtype=torch.float64, device=t.device
        )
        fn = lib.pds_cmvn_stats_f32 if t.dtype == torch.float32 else lib.pds_cmvn_stats_f64
        with torch.cuda.device(t.device):
            rc = fn(t.data_ptr(), outer, C, inner, stats.data_ptr(), scratch.data_ptr(), _stream(torch, t))
        _native.check(rc, "pds_cmvn_stats")
        return stats.cpu().numpy().reshape(2, C)

    def _check_width(self, num_coeffs):
        if self._stats is not None and self._stats.shape[1] != num_coeffs + 1:
            raise ValueError(
                "Expected feature vector of length {}; got {}".format(
                    self._stats.shape[1] - 1, num_coeffs
                )
            )

    # -- public -------------------------------------------------------------------------

    def accumulate(self, features, axis: int = -1) -> None:
        """Add `features` to the global statistics (reference post.py:193-212)"""
        shape = tuple(features.shape)
        if (shape and not np.prod(shape)) or not len(features):
            raise ValueError("Cannot accumulate from empty array")
        if len(shape) <= 1:
            features, axis = features.reshape(1, -1), 1
        t, outer, C, inner = self._as_device_3d(features, axis)
        self._check_width(C)
        sums = self._device_sums(t, outer, C, inner)
        if self._stats is None:
            self._stats = np.zeros((2, C + 1), dtype=np.float64)
        self._stats[0, -1] += outer * inner
        self._stats[0, :-1] += sums[0]
        self._stats[1, :-1] += sums[1]

    def apply(self, features, axis: int = -1, in_place: bool = False):
        shape = tuple(features.shape)
        if (shape and not np.prod(shape)) or not len(features):
            raise ValueError("Cannot apply to empty array")
        torch = _native.require_device()
        on_gpu = _is_gpu_tensor(features)
        vector = len(shape) <= 1
        if vector:
            view, ax = features.reshape(1, -1), 1
        else:
            view, ax = features, axis
        t, outer, C, inner = self._as_device_3d(view, ax)
        self._check_width(C)
        count = outer * inner
        if self.have_stats:
            count = self._stats[0, -1]
            means = self._stats[0, :-1] / count
            varss = self._stats[1, :-1] / count - means ** 2
        elif count == 1:
            # a lone vector has no variance of its own (reference post.py:240-247, 268-277)
            if self._norm_var:
                raise ValueError(
                    "Unable to standardize the variance of a vector with no global statistics"
                )
            warnings.warn("Standardizing a single vector to 0")
            zeros = torch.zeros(shape, dtype=torch.float64, device=t.device)
            return zeros if on_gpu else zeros.cpu().numpy()
        else:
            sums = self._device_sums(t, outer, C, inner)
            means = sums[0] / count
            varss = sums[1] / count - means ** 2
        if self._norm_var:
            close_zero = np.isclose(varss, 0)
            if np.any(close_zero):
                warnings.warn("0 variance encountered. Replacing with 1")
                varss = np.where(close_zero, 1.0, varss)
            scales = 1 / (varss ** 0.5)
        else:
            scales = np.ones(C, dtype=np.float64)
        lib = _native.lib()
        d_scale = _to_device(np.asarray(scales, dtype=np.float64))
        d_shift = _to_device(np.asarray(means * scales, dtype=np.float64))
        if in_place and on_gpu and features.dtype == torch.float64 and features.is_contiguous():
            out = t
        else:
            out = torch.empty(t.shape, dtype=torch.float64, device=t.device)
        fn = lib.pds_cmvn_apply_f32 if t.dtype == torch.float32 else lib.pds_cmvn_apply_f64
        with torch.cuda.device(t.device):
            rc = fn(
                t.data_ptr(), outer, C, inner, d_scale.data_ptr(), d_shift.data_ptr(),
                out.data_ptr(), _stream(torch, t),
            )
        _native.check(rc, "pds_cmvn_apply")
        out = out.reshape(shape)
        if on_gpu:
            return out
        res = out.cpu().numpy()
        if in_place and isinstance(features, np.ndarray) and features.dtype == np.float64:
            features[...] = res
            return features
        return res

    def apply_rows(self, feats, row_offsets, out_dtype=None):
        """Per-utterance (local) CMVN over a packed ragged batch, entirely on the GPU

        `feats` is the ``(total_rows, C)`` GPU tensor :func:`compute_packed` returns and
        `row_offsets` its ``B + 1`` row offsets.  Returns a float64 tensor (or float32
        with ``out_dtype=torch.float32``) of the same shape.
        """
        torch = _native.require_device()
        lib = _native.lib()
        if self.have_stats:
            raise ValueError("apply_rows standardises locally; global statistics are set")
        if not _is_gpu_tensor(feats) or feats.dtype != torch.float32 or feats.dim() != 2:
            raise ValueError("feats must be a 2-D float32 GPU tensor")
        if feats.stride(1) != 1:
            feats = feats.contiguous()
        B, C = len(row_offsets) - 1, feats.shape[1]
        out_dtype = torch.float64 if out_dtype is None else out_dtype
        out = torch.empty(feats.shape, dtype=out_dtype, device=feats.device)
        if B <= 0 or feats.shape[0] == 0:
            return out
        meta, _ = _rows_meta(row_offsets, feats.device)
        stats = torch.empty((B, 2, C), dtype=torch.float64, device=feats.device)
        zero_var = torch.zeros(1, dtype=torch.int32, device=feats.device)
        fn = lib.pds_cmvn_rows_f32 if out_dtype == torch.float64 else lib.pds_cmvn_rows_f32out
        with torch.cuda.device(feats.device):
            for lo in range(0, B, 65535):
                hi = min(B, lo + 65535)
                rc = fn(
                    feats.data_ptr(), feats.stride(0), meta[0, lo:].data_ptr(),
                    meta[1, lo:].data_ptr(), hi - lo, C, int(self._norm_var),
                    stats[lo:].data_ptr(), out.data_ptr(), out.stride(0),
                    zero_var.data_ptr(), _stream(torch, feats),
                )
                _native.check(rc, "pds_cmvn_rows")
        self._last_zero_var = zero_var  # inspect with .item() (synchronises)
        return out


CMVN = Standardize


# ------------------------------------------------------------------ Deltas -----------


class Deltas(PostProcessor):
    """Append (or stack) delta features: repeated correlation with a ramp filter

    `axis` of :func:`apply` is the *time* axis.  The order-k filter is the k-fold
    convolution of ``arange(-W, W + 1) / sum(j^2)``; slices are padded (default
    ``"edge"``), correlated in float64 and cast back to the input dtype (reference
    post.py:367-491).
    """

    aliases = {"deltas"}

    def __init__(
        self,
        num_deltas: int,
        target_axis: int = -1,
        concatenate: bool = True,
        context_window: int = 2,
        pad_mode: Union[str, Callable] = "edge",
        **kwargs,
    ):
        self._target_axis = target_axis
        self._pad_mode = pad_mode
        self._pad_kwargs = kwargs
        self.concatenate = bool(concatenate)
        self.num_deltas = num_deltas
        ramp = np.arange(1 + 2 * context_window, dtype=np.float64)
        ramp -= context_window
        ramp /= np.sum(ramp ** 2)
        self._filts = [np.ones(1, dtype=np.float64)]
        for idx in range(num_deltas):
            self._filts.append(np.convolve(self._filts[idx], ramp))
        self._device_filts = {}

    def _filters_on(self, device):
        key = str(device)
        if key not in self._device_filts:
            torch = _native.require_device()
            lens = [len(f) for f in self._filts[1:]]
            offs = np.zeros(len(lens) + 1, dtype=np.int32)
            np.cumsum(lens, out=offs[1:])
            flat = np.concatenate(self._filts[1:]) if lens else np.zeros(1)
            self._device_filts[key] = (
                torch.from_numpy(flat).to(device),
                torch.from_numpy(offs).to(device),
            )
        return self._device_filts[key]

    def _apply_per_order(self, features, host, axis, target, on_gpu, in_dtype):
        """:func:`apply` for pad modes whose samples are computed or depend on the pad width"""
        torch = _native.require_device()
        lib = _native.lib()
        host = np.asarray(host, dtype=np.float64)
        shape = host.shape
        ndim = host.ndim
        time = shape[axis]
        outer = int(np.prod(shape[:axis], dtype=np.int64))
        inner = int(np.prod(shape[axis + 1 :], dtype=np.int64))
        statics = features if on_gpu else _to_device(np.asarray(features))
        res_dtype = statics.dtype if on_gpu else None
        pieces = [statics]
        for filt in self._filts[1:]:
            reach = (len(filt) - 1) // 2
            widths = [(0, 0)] * ndim
            widths[axis] = (reach, reach)
            src = _to_device(np.pad(host, widths, self._pad_mode, **self._pad_kwargs))
            d_filt = torch.from_numpy(np.ascontiguousarray(filt)).to(src.device)
            d_offs = torch.tensor([0, len(filt)], dtype=torch.int32, device=src.device)
            out = torch.empty((2,) + shape, dtype=torch.float64, device=src.device)
            with torch.cuda.device(src.device):
                rc = lib.pds_deltas_f64(
                    src.data_ptr(), outer, time, inner, d_filt.data_ptr(), d_offs.data_ptr(), 1, 0, reach,
                    out.data_ptr(), outer * time * inner, time * inner, inner, 1, _stream(torch, src),
                )
            _native.check(rc, "pds_deltas")
            pieces.append(out[1])
        if on_gpu:
            pieces = [pieces[0]] + [p.to(res_dtype) for p in pieces[1:]]
            return torch.cat(pieces, target) if self.concatenate else torch.stack(pieces, target)
        # the reference casts every order back to the input dtype before concatenating
        cast = [np.asarray(features)] + [p.cpu().numpy().astype(in_dtype) for p in pieces[1:]]
        return np.concatenate(cast, target) if self.concatenate else np.stack(cast, target)

    def apply(self, features, axis: int = -1, in_place: bool = False):
        torch = _native.require_device()
        lib = _native.lib()
        on_gpu = _is_gpu_tensor(features)
        K = self.num_deltas
        if on_gpu:
            t = features
            in_dtype = None
            if t.dtype not in (torch.float32, torch.float64):
                raise TypeError("GPU features must be float32 or float64")
        else:
            arr = np.asarray(features)
            in_dtype = arr.dtype
            work = arr if arr.dtype in (np.float32, np.float64) else arr.astype(np.float64)
            t = None
        shape = tuple(features.shape)
        ndim = len(shape)
        axis = axis % ndim
        target = self._target_axis
        out_ndim = ndim if self.concatenate else ndim + 1
        if not -out_ndim <= target < out_ndim:
            raise np.exceptions.AxisError(target, out_ndim)
        target %= out_ndim
        time = shape[axis]
        outer = int(np.prod(shape[:axis], dtype=np.int64))
        inner = int(np.prod(shape[axis + 1 :], dtype=np.int64))
        stacked_shape = (K + 1,) + shape
        if outer * time * inner == 0 or K == 0:
            # nothing to correlate; only the layout changes
            pieces = [features] * (K + 1)
            if on_gpu:
                return torch.cat(pieces, target) if self.concatenate else torch.stack(pieces, target)
            return np.concatenate(pieces, target) if self.concatenate else np.stack(pieces, target)
        edge = self._pad_mode == "edge" and not self._pad_kwargs
        max_off = (len(self._filts[-1]) - 1) // 2
        # modes that COPY samples from positions fixed relative to the signal's ends: padding once
        # by the widest filter's reach gives every order the samples the reference's own, narrower
        # padding would (post.py:470-483)
        copies = (isinstance(self._pad_mode, str) and self._pad_mode in ("reflect", "symmetric", "wrap")
                  and not self._pad_kwargs)
        if edge:
            if t is None:
                t = _to_device(work)
            src = t.contiguous()
        elif copies:
            host = work if t is None else t.cpu().numpy()
            widths = [(0, 0)] * ndim
            widths[axis] = (max_off, max_off)
            src = _to_device(np.pad(host, widths, self._pad_mode, **self._pad_kwargs))
        else:
            # every other numpy.pad mode (linear_ramp, statistics, constants, odd reflection,
            # callables): the padded samples are computed, in float64, and may depend on the pad
            # width -- pad each order by its own reach on a float64 copy, one launch per order, as
            # the reference does
            return self._apply_per_order(features, work if t is None else t.cpu().numpy(), axis, target,
                                         on_gpu, in_dtype)
        d_filts, d_offs = self._filters_on(src.device)
        direct = self.concatenate and ndim == 2 and target != axis
        if direct:
            # (time, coeff) or (coeff, time) matrix with deltas appended to the other axis:
            # the kernel writes the concatenated layout itself
            out_shape = list(shape)
            out_shape[target] *= K + 1
            out = torch.empty(out_shape, dtype=src.dtype, device=src.device)
            if axis == 0:  # [1, time, inner=F] -> (time, (K+1) F)
                sk, so, st, si = shape[1], 0, shape[1] * (K + 1), 1
            else:  # [outer=F, time, 1] -> ((K+1) F, time)
                sk, so, st, si = shape[0] * time, time, 1, 0
        else:
            out = torch.empty(stacked_shape, dtype=src.dtype, device=src.device)
            sk, so, st, si = outer * time * inner, time * inner, inner, 1
        fn = lib.pds_deltas_f32 if src.dtype == torch.float32 else lib.pds_deltas_f64
        with torch.cuda.device(src.device):
            rc = fn(
                src.data_ptr(), outer, time, inner, d_filts.data_ptr(), d_offs.data_ptr(), K,
                int(edge), max_off, out.data_ptr(), sk, so, st, si, _stream(torch, src),
            )
        _native.check(rc, "pds_deltas")
        if not direct:
            pieces = list(out.unbind(0))
            out = torch.cat(pieces, target) if self.concatenate else torch.stack(pieces, target)
        if on_gpu:
            return out
        res = out.cpu().numpy()
        return res if res.dtype == in_dtype else res.astype(in_dtype)

    def apply_rows(self, feats, row_offsets, out=None):
        """Deltas of every utterance of a packed ragged batch, appended per row, on the GPU

        `feats`: ``(total_rows, F)`` float32 GPU tensor (rows may be strided), utterance
        b in rows ``row_offsets[b]:row_offsets[b+1]``.  Returns ``(total_rows, (K+1) F)``.
        Time is the row axis (Kaldi layout); padding is ``"edge"``.
        """
        torch = _native.require_device()
        lib = _native.lib()
        if self._pad_mode != "edge" or self._pad_kwargs:
            raise ValueError("apply_rows supports the default 'edge' padding only")
        if not _is_gpu_tensor(feats) or feats.dtype != torch.float32 or feats.dim() != 2:
            raise ValueError("feats must be a 2-D float32 GPU tensor")
        if feats.stride(1) != 1:
            feats = feats.contiguous()
        # `feats` may be a column slice of `out` (statics already in place): the kernel then only
        # adds the delta columns, in place
        B, F, K = len(row_offsets) - 1, feats.shape[1], self.num_deltas
        if out is None:
            out = torch.empty((feats.shape[0], (K + 1) * F), dtype=torch.float32, device=feats.device)
        elif (not _is_gpu_tensor(out) or out.dtype != torch.float32 or out.device != feats.device or out.dim() != 2
              or out.shape[0] < feats.shape[0] or out.shape[1] < (K + 1) * F
              or (out.shape[1] and out.stride(1) != 1) or (out.shape[0] > 1 and out.stride(0) < (K + 1) * F)):
            # (the kernel writes (K + 1) F floats at row r * stride(0) for every row of feats: anything else is out of bounds)
            raise ValueError(
                "out must be a 2-D float32 GPU tensor on feats' device with at least feats' rows and (K + 1) F "
                "columns, contiguous rows (stride(1) == 1) that do not overlap (stride(0) >= (K + 1) F)")
        if B <= 0 or feats.shape[0] == 0:
            return out
        meta, nrows = _rows_meta(row_offsets, feats.device)
        d_filts, d_offs = self._filters_on(feats.device)
        with torch.cuda.device(feats.device):
            for lo in range(0, B, 65535):
                hi = min(B, lo + 65535)
                rc = lib.pds_deltas_rows_f32(
                    feats.data_ptr(), feats.stride(0), meta[0, lo:].data_ptr(),
                    meta[1, lo:].data_ptr(), hi - lo, int(nrows[lo:hi].max()), F,
                    d_filts.data_ptr(), d_offs.data_ptr(), K, (len(self._filts[-1]) - 1) // 2,
                    out.data_ptr(), out.stride(0),
                    _stream(torch, feats),
                )
                _native.check(rc, "pds_deltas_rows")
        return out


# ------------------------------------------------------------------ Stack ------------


class Stack(PostProcessor):
    """Concatenate every `num_vectors` consecutive frames into one (reference post.py:494-563)

    `time_axis` is the axis frames are drawn from; `axis` of :func:`apply` the coefficient axis
    that grows `num_vectors`-fold.  Frames that do not fill a last group are dropped, or, with
    `pad_mode` (and keyword arguments of :func:`numpy.pad`), the time axis is first padded on
    the right up to a multiple of `num_vectors`.

    Stacking is data movement, not arithmetic: a host array is re-viewed / re-gathered with
    numpy and a GPU tensor with torch indexing, exactly as the reference does it, and a packed
    ragged batch goes through one HIP copy kernel (:func:`apply_rows`).
    """

    aliases = {"stack"}

    def __init__(self, num_vectors: int, time_axis: int = 0,
                 pad_mode: Optional[Union[str, Callable]] = None, **kwargs):
        if num_vectors < 1:
            raise ValueError(f"Expected num_vectors to be positive, got {num_vectors}")
        self.num_vectors = num_vectors
        self.time_axis = time_axis
        self._pad_mode = pad_mode
        self._pad_kwargs = kwargs

    def apply(self, features, axis: int = -1, in_place: bool = False):
        nd = features.ndim if not _is_gpu_tensor(features) else features.dim()
        axis, time_axis = axis % nd, self.time_axis % nd
        if axis == time_axis:
            raise RuntimeError(f"feature and time axes are the same ({axis})")
        nv = self.num_vectors
        on_gpu = _is_gpu_tensor(features)
        T = features.shape[time_axis]
        if self._pad_mode is not None and T % nv:
            extra = nv - T % nv
            if on_gpu:
                features = self._pad_tensor(features, time_axis, extra)
            else:
                widths = [(0, 0)] * nd
                widths[time_axis] = (0, extra)
                features = np.pad(features, widths, self._pad_mode, **self._pad_kwargs)
            in_place = True  # already a private copy
            T += extra
        groups = T // nv
        if nd == 2:
            # the (T, F) matrix re-read as (T / nv, nv F): a reshape of the time-major layout
            if not in_place:
                features = features.clone() if on_gpu else features.copy()
            mat = features.T if time_axis else features
            mat = mat[: groups * nv].reshape(groups, mat.shape[1] * nv)
            return mat.T if time_axis else mat
        # general rank: frame v of every group, for v = 0 .. nv - 1, side by side on `axis`
        index = [slice(None)] * nd
        parts = []
        for v in range(nv):
            index[time_axis] = slice(v, groups * nv, nv)
            parts.append(features[tuple(index)])
        if on_gpu:
            return _native.require_device().cat(parts, axis)
        return np.concatenate(parts, axis)

    def _pad_tensor(self, t, time_axis, extra):
        torch = _native.require_device()
        if self._pad_mode == "edge" and not self._pad_kwargs:
            last = t.narrow(time_axis, t.shape[time_axis] - 1, 1)
            reps = [1] * t.dim()
            reps[time_axis] = extra
            return torch.cat([t, last.repeat(*reps)], time_axis)
        if self._pad_mode == "constant" and set(self._pad_kwargs) <= {"constant_values"}:
            shape = list(t.shape)
            shape[time_axis] = extra
            fill = self._pad_kwargs.get("constant_values", 0)
            return torch.cat([t, torch.full(shape, fill, dtype=t.dtype, device=t.device)], time_axis)
        raise ValueError("GPU tensors support pad_mode 'edge' and 'constant' only")

    def apply_rows(self, feats, row_offsets):
        """Stack every utterance of a packed ragged batch on the GPU

        `feats`: ``(total_rows, F)`` float32 GPU tensor, utterance b in rows
        ``row_offsets[b]:row_offsets[b+1]`` (time is the row axis).  Returns
        ``(stacked, new_row_offsets)`` with ``stacked`` of shape ``(new_total, num_vectors F)``.
        """
        torch = _native.require_device()
        lib = _native.lib()
        if not _is_gpu_tensor(feats) or feats.dtype != torch.float32 or feats.dim() != 2:
            raise ValueError("feats must be a 2-D float32 GPU tensor")
        if self._pad_mode is None:
            pad = 0
        elif self._pad_mode == "constant" and not self._pad_kwargs:
            pad = 1
        elif self._pad_mode == "edge" and not self._pad_kwargs:
            pad = 2
        else:
            raise ValueError("apply_rows supports pad_mode None, 'constant' (zeros) and 'edge'")
        if feats.stride(1) != 1:
            feats = feats.contiguous()
        nv, F = self.num_vectors, feats.shape[1]
        rows = np.ascontiguousarray(row_offsets, dtype=np.int64)
        nrows = np.diff(rows)
        out_rows = (nrows + nv - 1) // nv if pad else nrows // nv
        new_offsets = np.concatenate([[0], np.cumsum(out_rows)]).astype(np.int64)
        out = torch.empty((int(new_offsets[-1]), nv * F), dtype=torch.float32, device=feats.device)
        B = len(nrows)
        if B == 0 or out.shape[0] == 0:
            return out, new_offsets
        meta = torch.from_numpy(np.stack([rows[:-1], nrows, new_offsets[:-1]])).to(feats.device)
        with torch.cuda.device(feats.device):
            for lo in range(0, B, 65535):
                hi = min(B, lo + 65535)
                rc = lib.pds_stack_rows_f32(
                    feats.data_ptr(), feats.stride(0), meta[0, lo:].data_ptr(), meta[1, lo:].data_ptr(),
                    meta[2, lo:].data_ptr(), hi - lo, int(out_rows[lo:hi].max()), F, nv, pad,
                    out.data_ptr(), out.stride(0), _stream(torch, feats),
                )
                _native.check(rc, "pds_stack_rows")
        return out, new_offsets


# ------------------------------------------------------------------ Cepstra ----------

_CEPSTRA_MAX_WIDTH = 256  # columns of an input row pds_cepstra_rows serves (include/pds_amd.h)


class Cepstra(PostProcessor):
    """Cepstral coefficients: a DCT-II over the coefficient axis, then a lifter (MFCCs of log-mel features)

    `axis` of :func:`apply` is the *coefficient* axis, of width W; it becomes `num_ceps` wide, every other axis is
    kept.  With ``F = W`` (``F = W - 1`` with `energy`) the transform is

        D[k, f] = s_k cos(pi k (f + 0.5) / F),  s_0 = sqrt(1 / F), s_k = sqrt(2 / F)      (``norm="ortho"``)
        D[k, f] = 2 cos(pi k (f + 0.5) / F)                                               (``norm=None``)

    -- Kaldi's matrix and ``scipy.fft.dct(type=2, norm="ortho")``, or scipy's unnormalised form -- and row k is scaled
    by ``1 + 0.5 Q sin(pi k / Q)`` with ``Q = lifter`` (Kaldi's formula; ``0`` or ``None``: no lifter).  Both are folded
    into one float64 matrix ``M[k, f] = lift[k] D[k, f]`` on the host (:func:`matrix`), once per width and device.

    `energy`: column 0 of the input is the energy of a computer built with ``include_energy=True``; it is copied to
    column 0 of the output as it is, the transform runs over the other ``W - 1`` columns and output columns
    ``1 .. num_ceps - 1`` are cepstra ``1 .. num_ceps - 1`` (Kaldi's ``--use-energy=true``: the energy in the place of
    c0).

    The arithmetic is fixed: per row and output k a float64 accumulator starts at ``+0.0`` and takes
    ``acc = acc + M[k, f] * float64(x[f])`` for ``f = 0 .. F - 1`` in that order, product and sum rounded separately,
    and is rounded once to the row's dtype.  float32 and float64 keep their dtype; anything else is computed and
    returned as float64.
    """

    aliases = {"cepstra", "dct", "mfcc"}

    def __init__(self, num_ceps: int = 13, lifter: Optional[float] = 22.0, norm: Optional[str] = "ortho",
                 energy: bool = False):
        if isinstance(num_ceps, (bool, np.bool_)) or not isinstance(num_ceps, (int, np.integer)) or num_ceps < 1:
            raise ValueError(f"Expected num_ceps to be a positive integer, got {num_ceps!r}")
        if norm is not None and norm != "ortho":
            raise ValueError(f'norm must be "ortho" or None, got {norm!r}')
        if lifter is None:
            lifter = 0.0
        if isinstance(lifter, (bool, np.bool_)) or not isinstance(lifter, (int, float, np.integer, np.floating)):
            raise ValueError(f"lifter must be a number or None, got {lifter!r}")
        lifter = float(lifter)
        if not np.isfinite(lifter) or lifter < 0:
            raise ValueError(f"lifter must be finite and not negative, got {lifter!r}")
        self.num_ceps, self.lifter, self.norm, self.energy = int(num_ceps), lifter, norm, bool(energy)
        self._device_matrix = {}  # (width, device) -> device float64 [K, F]

    def table(self, F: int) -> np.ndarray:
        """the float64 ``[num_ceps, F]`` matrix of an `F`-point transform: DCT-II rows scaled by the lifter"""
        k = np.arange(self.num_ceps, dtype=np.float64)[:, None]
        f = np.arange(F, dtype=np.float64)[None, :]
        D = np.cos(np.pi * k * (f + 0.5) / F)
        if self.norm == "ortho":
            D *= np.sqrt(2.0 / F)
            D[0] = np.sqrt(1.0 / F)  # (cos(0) = 1)
        else:
            D *= 2.0
        if self.lifter:
            D *= 1.0 + 0.5 * self.lifter * np.sin(np.pi * k / self.lifter)
        return D

    def _split(self, width: int) -> Tuple[int, int]:
        """``(F, copy_cols)`` of input rows of `width` columns, or ``ValueError``: the width is only known at apply"""
        width, copy = int(width), int(self.energy)
        F = width - copy
        if F < 1 or self.num_ceps > F:
            raise ValueError(
                f"Cepstra: num_ceps = {self.num_ceps} needs at least {self.num_ceps + copy} coefficients"
                f"{' (the energy among them)' if copy else ''}, got {width}")
        if width > _CEPSTRA_MAX_WIDTH:
            raise ValueError(f"Cepstra: rows of {width} coefficients; at most {_CEPSTRA_MAX_WIDTH} are served")
        return F, copy

    def matrix(self, width: int) -> Tuple[np.ndarray, int]:
        """``(M, copy_cols)`` for input rows of `width` columns, as pds_cepstra_rows takes them: the host float64
        ``[K, F]`` matrix and the leading columns that pass unchanged -- the whole table and 0, or with `energy` rows
        ``1 ..`` of the ``(width - 1)``-point table and 1.  ``ValueError`` unless ``1 <= num_ceps <= F`` and
        ``width <= 256``"""
        F, copy = self._split(width)
        return np.ascontiguousarray(self.table(F)[copy:]), copy

    def _matrix_on(self, width, device):
        key = (int(width), str(device))
        if key not in self._device_matrix:
            M, copy = self.matrix(width)
            torch = _native.require_device()
            # (num_ceps = 1 with energy: nothing to transform, no matrix)
            self._device_matrix[key] = (torch.from_numpy(M).to(device) if len(M) else None, len(M), copy)
        return self._device_matrix[key]

    def apply(self, features, axis: int = -1, in_place: bool = False):
        # (`in_place` is accepted and ignored: the shape changes)
        on_gpu = _is_gpu_tensor(features)
        if not on_gpu:
            features = np.asarray(features)
        shape = tuple(features.shape)
        if not shape:
            raise ValueError("Cepstra: expected at least one dimension")
        axis = axis % len(shape)
        W = shape[axis]
        self._split(W)  # (the width's errors come before any device work)
        torch = _native.require_device()
        if on_gpu:
            t = features if features.dtype in (torch.float32, torch.float64) else features.to(torch.float64)
        else:
            t = _to_device(features if features.dtype in (np.float32, np.float64) else features.astype(np.float64))
        d_matrix, K, copy = self._matrix_on(W, t.device)
        rows = t.movedim(axis, -1)
        lead = tuple(rows.shape[:-1])
        # a matrix whose rows are contiguous goes as it is, whatever its row stride (a column slice of a wider
        # tensor); anything else as a contiguous (rows, W) copy
        if not (rows.dim() == 2 and rows.stride(1) == 1 and (rows.stride(0) >= W or rows.shape[0] <= 1)):
            rows = rows.reshape(int(np.prod(lead, dtype=np.int64)), W).contiguous()
        R = rows.shape[0]
        out = torch.empty((R, copy + K), dtype=t.dtype, device=t.device)
        if R and K:
            lib = _native.lib()
            fn = lib.pds_cepstra_rows_f32 if t.dtype == torch.float32 else lib.pds_cepstra_rows_f64
            with torch.cuda.device(t.device):
                rc = fn(rows.data_ptr(), rows.stride(0) if R > 1 else W, R, W - copy, d_matrix.data_ptr(), K, copy,
                        out.data_ptr(), out.stride(0), _stream(torch, t))
            _native.check(rc, "pds_cepstra_rows")
        elif R:
            out.copy_(rows[:, :copy])
        out = out.reshape(lead + (copy + K,)).movedim(-1, axis)
        return out if on_gpu else out.cpu().numpy()


# ------------------------------------------------------------------ SlidingCMVN ------


def _positive_int(value, what):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or value < 1:
        raise ValueError(f"SlidingCMVN: {what} must be a positive integer, got {value!r}")
    if value >= 1 << 31:
        raise ValueError(f"SlidingCMVN: {what} must be below 2**31, got {value!r}")
    return int(value)


def _flag(value, what):
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError(f"SlidingCMVN: {what} must be a bool, got {value!r}")
    return bool(value)


class SlidingCMVN(PostProcessor):
    """Mean (and variance) normalisation over a sliding window of frames: Kaldi's ``apply-cmvn-sliding``

    `axis` of :func:`apply` is the *coefficient* axis; time is the axis in front of it (rows of a ``(frames, coeffs)``
    matrix).  For an utterance of T frames, frame t and ``W = cmn_window`` the window ``[ws, we)`` is

        center:      ws = t - W // 2;  we = ws + W
        not center:  ws = t - W;       we = t + 1
        if ws < 0:                 we -= ws;  ws = 0
        if not center and we > t:  we = max(t + 1, min_window)
        if we > T:                 ws -= we - T;  we = T;  ws = max(ws, 0)

    -- Kaldi's rule, its causal window of ``W + 1`` frames included.  ``0 <= ws <= t < we <= T``, ``ws`` and ``we``
    each move by 0 or 1 from one frame to the next, and the window holds at most ``max(W + 1, min_window)`` frames.

    The arithmetic is fixed: per coefficient, in float64, x widened first, every operation rounded separately,
    division and square root correctly rounded.

        t % refresh == 0:  s1 = s2 = 0, then for u = ws .. we - 1 in order  s1 += x_u;  s2 += x_u * x_u
        other frames:      if ws moved  s1 -= x_old;  s2 -= x_old * x_old  (the frame that left), and then, if we moved,
                           s1 += x_new;  s2 += x_new * x_new  (the frame that entered)
        n = we - ws;  mean = s1 / n;  y = x_t - mean
        norm_vars:  y = 0 if n == 1, else  var = s2 / n - mean * mean;  var = 1e-10 unless var > 1e-10;
                    y = y * (1 / sqrt(var))

    and y is rounded once to the input's type: float32 gives float32, float64 gives float64, anything else is widened
    to float64 first.  `refresh` (default: `cmn_window`) is part of the result, in its last bits: the sums are rebuilt
    every `refresh` frames, so segments of `refresh` frames are computed in parallel, rounding does not drift over a
    long stream, and a NaN or infinite frame stops affecting the output at the first refresh after it has left the
    window.  The same object gives the same bits offline and, with ``center=False`` and ``min_window=1``, streamed
    (``StreamBatch(sliding_cmvn=...)``).
    """

    aliases = {"sliding_cmvn", "cmvn_sliding", "sliding"}

    def __init__(self, cmn_window: int = 600, min_window: int = 100, center: bool = False, norm_vars: bool = False,
                 refresh: Optional[int] = None):
        self.cmn_window = _positive_int(cmn_window, "cmn_window")
        self.min_window = _positive_int(min_window, "min_window")
        self.center = _flag(center, "center")
        self.norm_vars = _flag(norm_vars, "norm_vars")
        self.refresh = self.cmn_window if refresh is None else _positive_int(refresh, "refresh")

    def apply_rows(self, feats, row_offsets, out=None):
        """Every utterance of a packed ragged batch normalised by itself, in one launch on the GPU

        `feats`: ``(total_rows, C)`` float32 or float64 GPU tensor (rows may be strided: a column slice of a wider
        tensor), utterance b in rows ``row_offsets[b]:row_offsets[b+1]``; empty and one-row utterances are allowed.
        Returns a tensor of the same shape and dtype (`out`, if given: it must not share memory with `feats`).
        """
        torch = _native.require_device()
        lib = _native.stages_lib()
        if not _is_gpu_tensor(feats) or feats.dtype not in (torch.float32, torch.float64) or feats.dim() != 2:
            raise ValueError("feats must be a 2-D float32 or float64 GPU tensor")
        if feats.shape[1] and feats.stride(1) != 1:
            feats = feats.contiguous()
        R, C = feats.shape
        rows = np.ascontiguousarray(row_offsets, dtype=np.int64)
        if rows.ndim != 1 or len(rows) < 1 or (np.diff(rows) < 0).any() or (len(rows) and (rows[0] < 0 or rows[-1] > R)):
            raise ValueError("row_offsets must be B + 1 ascending row indices within feats")
        if out is None:
            out = torch.empty((R, C), dtype=feats.dtype, device=feats.device)
        elif (not _is_gpu_tensor(out) or out.dtype != feats.dtype or out.device != feats.device
              or tuple(out.shape) != (R, C) or (C and out.stride(1) != 1)):
            raise ValueError("out must be a GPU tensor of feats' shape, dtype and device with contiguous rows")
        elif R and C and out.untyped_storage().data_ptr() == feats.untyped_storage().data_ptr():
            raise ValueError("out must not share memory with feats: the kernel works out of place")
        B = len(rows) - 1
        if B <= 0 or R == 0 or C == 0:
            return out
        meta, nrows = _rows_meta(rows, feats.device)
        in_stride = feats.stride(0) if R > 1 else C
        out_stride = out.stride(0) if R > 1 else C
        if in_stride < C or out_stride < C:
            raise ValueError("rows of feats and out must not overlap")
        fn = lib.pds_sliding_cmvn_rows_f32 if feats.dtype == torch.float32 else lib.pds_sliding_cmvn_rows_f64
        # one launch, unless the batch needs more lanes (utterances x segments x C) than a grid has blocks for
        step = B
        segs = -(-int(nrows.max()) // self.refresh)
        if segs:
            step = max(1, min(B, ((1 << 31) - 1) * 256 // (segs * C)))
        with torch.cuda.device(feats.device):
            for lo in range(0, B, step):
                hi = min(B, lo + step)
                rc = fn(feats.data_ptr(), in_stride, meta[0, lo:].data_ptr(), meta[1, lo:].data_ptr(), hi - lo,
                        int(nrows[lo:hi].max()), C, self.cmn_window, self.min_window, int(self.center),
                        int(self.norm_vars), self.refresh, out.data_ptr(), out_stride, _stream(torch, feats))
                _native.check_stages(rc, "pds_sliding_cmvn_rows")
        return out

    def apply(self, features, axis: int = -1, in_place: bool = False):
        on_gpu = _is_gpu_tensor(features)
        if not on_gpu:
            features = np.asarray(features)
        shape = tuple(features.shape)
        if len(shape) not in (2, 3):
            raise ValueError("SlidingCMVN: expected (frames, coeffs) or (batch, frames, coeffs)")
        axis = axis % len(shape)
        torch = _native.require_device()
        if on_gpu:
            t = features if features.dtype in (torch.float32, torch.float64) else features.to(torch.float64)
        else:
            t = _to_device(features if features.dtype in (np.float32, np.float64) else features.astype(np.float64))
        # coefficients last, time in front of them, utterances in front of that
        moved = t.movedim(axis, -1)
        lead = tuple(moved.shape)
        T, C = lead[-2], lead[-1]
        B = lead[0] if len(lead) == 3 else 1
        if moved.dim() == 2 and moved.stride(1) == 1 and (moved.stride(0) >= C or T <= 1):
            rows = moved  # a matrix whose rows are contiguous goes as it is, whatever its row stride
        else:
            rows = moved.reshape(B * T, C).contiguous()
        out = self.apply_rows(rows, np.arange(B + 1, dtype=np.int64) * T)
        out = out.reshape(lead).movedim(-1, axis)
        if on_gpu:
            if in_place and features.dtype == out.dtype:
                features.copy_(out)
                return features
            return out
        res = out.cpu().numpy()
        if in_place and features.dtype == res.dtype and features.flags.writeable:
            features[...] = res
            return features
        return res


# ------------------------------------------------------------------ EnergyVAD --------

_SELECT_TILE = 256  # rows of a block of pds_select_rows_w32 (include/pds_amd_stages.h)
_SELECT_MAX_BLOCKS = (1 << 31) - 1  # ... and the blocks one call of it may launch


def _vad_number(value, what):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"EnergyVAD: {what} must be a number, got {value!r}")
    value = float(value)
    if not np.isfinite(value):
        raise ValueError(f"EnergyVAD: {what} must be finite, got {value!r}")
    return value


def _vad_index(value, what):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or value < 0:
        raise ValueError(f"EnergyVAD: {what} must be an integer that is not negative, got {value!r}")
    if value >= 1 << 31:
        raise ValueError(f"EnergyVAD: {what} must be below 2**31, got {value!r}")
    return int(value)


class EnergyVAD(PostProcessor):
    """Energy-based voice activity detection: Kaldi's ``compute-vad-energy`` and ``select-voiced-frames``

    `axis` of :func:`decide` / :func:`apply` is the *coefficient* axis; time is the axis in front of it (rows of a
    ``(frames, coeffs)`` matrix).  Column `energy_col` of a row is the frame's log energy: column 0 of a computer built
    with ``include_energy=True`` and of ``Cepstra(energy=True)``.  The defaults and the rule are Kaldi's
    ``ComputeVadEnergy``.  For an utterance of ``T >= 1`` frames with energies ``e_t``, each widened to float64 first,

        if energy_mean_scale != 0:
            p_j = sum of e_t over t = j, j + 64, j + 128, .. in that order, starting from +0.0       (0 <= j < 64)
            s   = +0.0;  for j = 0 .. 63 in order:  s += p_j
            thr = energy_threshold + (energy_mean_scale * s) / T        (each operation rounded once, in float64)
        else:
            thr = energy_threshold                                       (the energies are not summed)
        for frame t:  lo = max(0, t - frames_context);  hi = min(T - 1, t + frames_context)
            den = hi - lo + 1;  num = the number of u in [lo, hi] with e_u > thr
            voiced_t = float(num) >= float(den) * proportion_threshold

    The 64 interleaved partial sums are part of the result, in its last bits: a wave of the device sums an utterance
    with one partial per lane, and the host can reproduce the sum.  A NaN energy is never above the threshold; a NaN or
    infinite sum makes every comparison false or true as IEEE says.  An utterance without frames gives no decisions.

    Selection keeps the voiced rows, in order and byte for byte; an utterance without a voiced frame gives 0 rows
    (Kaldi skips such an utterance).  float32 stays float32 and float64 stays float64; anything else is widened to
    float64 first.

    `select_last` is read by ``signals-to-torch-feat-dir`` only: the decisions are taken where the stage stands in
    ``--postprocess``, the later stages see all frames, and the rows are dropped after the last stage -- Kaldi's order
    (``compute-vad-energy``, ``apply-cmvn-sliding``, ``select-voiced-frames``).
    """

    aliases = {"vad", "energy_vad", "vad_energy"}

    def __init__(self, energy_threshold: float = 5.0, energy_mean_scale: float = 0.5, frames_context: int = 0,
                 proportion_threshold: float = 0.6, energy_col: int = 0, select_last: bool = False):
        self.energy_threshold = _vad_number(energy_threshold, "energy_threshold")
        self.energy_mean_scale = _vad_number(energy_mean_scale, "energy_mean_scale")
        if self.energy_mean_scale < 0:
            raise ValueError(f"EnergyVAD: energy_mean_scale must not be negative, got {energy_mean_scale!r}")
        self.frames_context = _vad_index(frames_context, "frames_context")
        self.proportion_threshold = _vad_number(proportion_threshold, "proportion_threshold")
        if not 0.0 < self.proportion_threshold < 1.0:
            raise ValueError(
                f"EnergyVAD: proportion_threshold must lie strictly between 0 and 1, got {proportion_threshold!r}")
        self.energy_col = _vad_index(energy_col, "energy_col")
        if not isinstance(select_last, (bool, np.bool_)):
            raise ValueError(f"EnergyVAD: select_last must be a bool, got {select_last!r}")
        self.select_last = bool(select_last)

    # -- packed ragged batches ----------------------------------------------------------------

    @staticmethod
    def _check_rows(feats, row_offsets):
        torch = _native.require_device()
        if not _is_gpu_tensor(feats) or feats.dtype not in (torch.float32, torch.float64) or feats.dim() != 2:
            raise ValueError("feats must be a 2-D float32 or float64 GPU tensor")
        R = feats.shape[0]
        rows = np.ascontiguousarray(row_offsets, dtype=np.int64)
        if rows.ndim != 1 or len(rows) < 1 or (np.diff(rows) < 0).any() or rows[0] < 0 or rows[-1] > R:
            raise ValueError("row_offsets must be B + 1 ascending row indices within feats")
        return torch, rows

    def decide_rows(self, feats, row_offsets):
        """The decisions of every utterance of a packed ragged batch, in one launch on the GPU

        `feats`: ``(total_rows, C)`` float32 or float64 GPU tensor (rows may be strided: a column slice of a wider
        tensor), utterance b in rows ``row_offsets[b]:row_offsets[b+1]``; empty utterances are allowed.  Returns
        ``(voiced, counts)``: a uint8 GPU tensor ``(total_rows,)`` of 0 and 1 (0 in rows of no utterance), and the
        host int64 ``(B,)`` numbers of voiced rows per utterance -- fetching them is the call's one synchronisation.
        """
        torch, rows = self._check_rows(feats, row_offsets)
        lib = _native.stages_lib()
        R, C = feats.shape
        if self.energy_col >= C:
            raise ValueError(f"EnergyVAD: energy_col = {self.energy_col}, but the rows have {C} coefficients")
        B = len(rows) - 1
        voiced = torch.zeros((R,), dtype=torch.uint8, device=feats.device)
        if B <= 0 or R == 0:
            return voiced, np.zeros(max(B, 0), dtype=np.int64)
        meta, nrows = _rows_meta(rows, feats.device)
        if not int(nrows.max()):
            return voiced, np.zeros(B, dtype=np.int64)
        col = feats[:, self.energy_col]
        stride = col.stride(0) if R > 1 else 1
        if stride < 1:
            col, stride = col.contiguous(), 1
        counts = torch.zeros((B,), dtype=torch.int64, device=feats.device)
        fn = lib.pds_vad_energy_rows_f32 if feats.dtype == torch.float32 else lib.pds_vad_energy_rows_f64
        with torch.cuda.device(feats.device):
            # (one wave per utterance: B < 2**31 utterances are always one grid)
            rc = fn(col.data_ptr(), stride, meta[0].data_ptr(), meta[1].data_ptr(), B, int(nrows.max()),
                    self.energy_threshold, self.energy_mean_scale, self.frames_context, self.proportion_threshold,
                    voiced.data_ptr(), counts.data_ptr(), _stream(torch, feats))
            _native.check_stages(rc, "pds_vad_energy_rows")
        return voiced, counts.cpu().numpy()

    def _select(self, torch, feats, rows, keep, counts):
        """the kept rows of `feats` (``keep``: uint8 GPU ``(R,)``; ``counts``: host kept rows per utterance)"""
        lib = _native.stages_lib()
        if feats.shape[1] and feats.stride(1) != 1:
            feats = feats.contiguous()
        R, C = feats.shape
        new_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        out = torch.empty((int(new_offsets[-1]), C), dtype=feats.dtype, device=feats.device)
        B = len(rows) - 1
        if B <= 0 or out.shape[0] == 0 or C == 0:
            return out, new_offsets
        meta, nrows = _rows_meta(rows, feats.device)
        per = feats.element_size() // 4  # 32-bit words of an element
        in_stride = (feats.stride(0) if R > 1 else C) * per
        if in_stride < C * per:
            raise ValueError("rows of feats must not overlap")
        out_off = torch.from_numpy(new_offsets[:-1].copy()).to(feats.device)
        # one launch, unless the batch needs more blocks (utterances x tiles of rows) than a grid has
        tiles = -(-int(nrows.max()) // _SELECT_TILE)
        step = max(1, min(B, _SELECT_MAX_BLOCKS // tiles))
        with torch.cuda.device(feats.device):
            for lo in range(0, B, step):
                hi = min(B, lo + step)
                rc = lib.pds_select_rows_w32(
                    feats.data_ptr(), in_stride, C * per, meta[0, lo:].data_ptr(), meta[1, lo:].data_ptr(), hi - lo,
                    int(nrows[lo:hi].max()), keep.data_ptr(), out_off[lo:].data_ptr(), out.data_ptr(), C * per,
                    _stream(torch, feats))
                _native.check_stages(rc, "pds_select_rows")
        return out, new_offsets

    def select_rows(self, feats, row_offsets, voiced):
        """The rows of a packed ragged batch whose `voiced` is set, in order and byte for byte, in one launch

        `feats`, `row_offsets` as for :func:`decide_rows`; `voiced`: a uint8 or bool mask of ``total_rows`` entries
        (a GPU tensor, or an array that is uploaded).  Returns ``(out, out_row_offsets)``: the kept rows packed, and the
        host int64 ``(B + 1,)`` offsets of the utterances in them, derived from the mask.
        """
        torch, rows = self._check_rows(feats, row_offsets)
        R = feats.shape[0]
        if not _is_gpu_tensor(voiced):
            voiced = torch.from_numpy(np.ascontiguousarray(voiced)).to(feats.device)
        if voiced.dtype not in (torch.uint8, torch.bool) or tuple(voiced.shape) != (R,) or voiced.device != feats.device:
            raise ValueError("voiced must be a uint8 or bool mask with one entry per row of feats, on feats' device")
        keep = voiced.contiguous()
        keep = keep.view(torch.uint8) if keep.dtype == torch.bool else keep
        B = len(rows) - 1
        if B <= 0 or R == 0:
            counts = np.zeros(max(B, 0), dtype=np.int64)
        else:
            # kept rows in front of every row, gathered at the utterances' ends (32-bit while the rows allow it)
            wide = torch.int32 if R < (1 << 31) else torch.int64
            before = torch.zeros((R + 1,), dtype=wide, device=feats.device)
            torch.cumsum(keep != 0, 0, dtype=wide, out=before[1:])
            at = before[torch.from_numpy(rows).to(feats.device)]
            counts = (at[1:] - at[:-1]).cpu().numpy().astype(np.int64)
        return self._select(torch, feats, rows, keep, counts)

    def apply_rows(self, feats, row_offsets):
        """:func:`select_rows` of :func:`decide_rows`: the voiced rows of every utterance of a packed ragged batch.
        Returns ``(out, out_row_offsets)``"""
        voiced, counts = self.decide_rows(feats, row_offsets)
        torch, rows = self._check_rows(feats, row_offsets)
        return self._select(torch, feats, rows, voiced, counts)

    # -- single tensors and arrays ------------------------------------------------------------

    @staticmethod
    def _device_rows(features, axis, dims, what):
        """(on_gpu, float32 / float64 GPU tensor with the coefficients last)"""
        on_gpu = _is_gpu_tensor(features)
        if not on_gpu:
            features = np.asarray(features)
        if len(features.shape) not in dims:
            raise ValueError(what)
        torch = _native.require_device()
        if on_gpu:
            t = features if features.dtype in (torch.float32, torch.float64) else features.to(torch.float64)
        else:
            t = _to_device(features if features.dtype in (np.float32, np.float64) else features.astype(np.float64))
        return on_gpu, t.movedim(axis % t.dim(), -1)

    def decide(self, features, axis: int = -1):
        """Which frames are voiced: a bool array (a bool GPU tensor for a GPU tensor) shaped like `features` without
        its coefficient axis.  ``(frames, coeffs)``, or ``(batch, frames, coeffs)`` with every utterance decided by
        itself"""
        on_gpu, moved = self._device_rows(features, axis, (2, 3),
                                          "EnergyVAD: expected (frames, coeffs) or (batch, frames, coeffs)")
        lead = tuple(moved.shape)
        T, C = lead[-2], lead[-1]
        B = lead[0] if len(lead) == 3 else 1
        rows = moved if moved.dim() == 2 else moved.reshape(B * T, C)
        voiced, _ = self.decide_rows(rows, np.arange(B + 1, dtype=np.int64) * T)
        voiced = voiced.view(_native.require_device().bool).reshape(lead[:-1])
        return voiced if on_gpu else voiced.cpu().numpy()

    def apply(self, features, axis: int = -1, in_place: bool = False):
        """The voiced rows of one utterance, a 2-D array or tensor, in order.  A batch would come out ragged (use
        :func:`apply_rows`) and the shape changes: 3-D input and ``in_place=True`` are ``ValueError`` s"""
        if in_place:
            raise ValueError("EnergyVAD: the number of rows changes, so there is no in_place")
        nd = features.dim() if _is_gpu_tensor(features) else np.ndim(features)
        if nd != 2:
            raise ValueError("EnergyVAD: apply takes one utterance, (frames, coeffs): the voiced rows of a batch are "
                             "ragged (apply_rows takes a packed batch)")
        on_gpu, moved = self._device_rows(features, axis, (2,), "EnergyVAD: expected (frames, coeffs)")
        out, _ = self.apply_rows(moved, np.asarray([0, moved.shape[0]], dtype=np.int64))
        out = out.movedim(-1, axis % 2)
        return out if on_gpu else out.cpu().numpy()


# ------------------------------------------------------------------ PCEN -------------


def _pcen_number(value, what):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"PCEN: {what} must be a number, got {value!r}")
    value = float(value)
    if not np.isfinite(value):
        raise ValueError(f"PCEN: {what} must be finite, got {value!r}")
    return value


def refuse_log_computer(computer, who: str = "PCEN") -> None:
    """``ValueError`` if `computer` (an STFT or short-integration frame computer) takes the logarithm of its
    energies (its ``use_log``): PCEN -- and PLP, `who` -- takes linear energies"""
    if bool(getattr(computer, "_log", False)):
        raise ValueError(f"{who} takes linear energies: the computer takes their logarithm (build it with use_log=False)")


class PCEN(PostProcessor):
    """Per-channel energy normalisation (PCEN; Wang et al. 2017, ``librosa.pcen``): a one-pole automatic gain control
    per column followed by a root compression, in place of ``log`` and utterance-level CMVN

    `axis` of :func:`apply` / :func:`smooth` is the *time* axis; every other axis holds independent columns.

    The definition.

    Per utterance of T >= 1 rows and per column c, in float64, every operation rounded by itself (no contraction):

    1. oms = 1.0 - smooth, rounded once on the host, and bp = bias ** power as numpy float64 on the host.  Both are
       passed to the kernels as arguments.  The device never recomputes them.
    2. M[0] = E[0], widened exactly.  For t >= 1, M[t] = (oms * M[t-1]) + (smooth * E[t]): two products and one sum,
       each rounded once.  This is librosa's steady-state start.
    3. y[t] = pow(E[t] / pow(eps + M[t], gain) + bias, power) - bp.  Every operation is float64.  There are no special
       cases for particular exponents.  The result is rounded once to the row type.

    The output has the input's type (float32 or float64) and shape.  Every column is treated alike, including an energy
    column.  The input is meant to be the non-negative linear energies of a computer with use_log=False.  A negative
    base gives what IEEE pow gives.  A NaN or infinite E[t] stays in M for the rest of the utterance, because a one-pole
    filter does not forget.  T = 0 gives nothing.

    M is plain IEEE arithmetic, which numpy reproduces bit for bit (:func:`smooth_rows` returns it).  y goes through the
    device's ``pow``, which is not numpy's: it agrees with a numpy model within the float32 / float64 tolerances of this
    package, and it is bit-identical between :func:`apply`, :func:`apply_rows` and ``StreamBatch(pcen=...)``, whatever
    the cuts of a stream.  Anything but float32 and float64 input is widened to float64 first.

    The object keeps `smooth` as ``smooth_coeff`` (:func:`smooth` is the method that returns M), ``oms`` and ``bp`` as
    the kernels are given them, and the other arguments under their names.
    """

    aliases = {"pcen", "per_channel_energy_norm"}

    def __init__(self, smooth: float = 0.025, gain: float = 0.98, bias: float = 2.0, power: float = 0.5,
                 eps: float = 1e-6):
        self.smooth_coeff = _pcen_number(smooth, "smooth")  # (`smooth` itself is the method that returns M)
        self.gain = _pcen_number(gain, "gain")
        self.bias = _pcen_number(bias, "bias")
        self.power = _pcen_number(power, "power")
        self.eps = _pcen_number(eps, "eps")
        if not 0.0 < self.smooth_coeff <= 1.0:
            raise ValueError(f"PCEN: smooth must lie in (0, 1], got {smooth!r}")
        if self.gain < 0.0:
            raise ValueError(f"PCEN: gain must not be negative, got {gain!r}")
        if self.bias < 0.0:
            raise ValueError(f"PCEN: bias must not be negative, got {bias!r}")
        if not self.power > 0.0:
            raise ValueError(f"PCEN: power must be positive, got {power!r}")
        if not self.eps > 0.0:
            raise ValueError(f"PCEN: eps must be positive, got {eps!r}")
        # what the kernels are given and never recompute (step 1 of the definition)
        self.oms = float(np.float64(1.0) - np.float64(self.smooth_coeff))
        self.bp = float(np.float64(self.bias) ** np.float64(self.power))

    @classmethod
    def from_time_constant(cls, time_constant_s: float = 0.4, frame_shift_ms: float = 10.0, **kw):
        """``PCEN(smooth=s, **kw)`` with librosa's rule for the smoother: ``T = time_constant_s / (frame_shift_ms /
        1000)`` frames and ``s = (sqrt(1 + 4 T**2) - 1) / (2 T**2)``, computed in float64 on the host"""
        if "smooth" in kw:
            raise ValueError("PCEN.from_time_constant: the time constant gives smooth; do not pass it")
        tc = _pcen_number(time_constant_s, "time_constant_s")
        shift = _pcen_number(frame_shift_ms, "frame_shift_ms")
        if not tc > 0.0 or not shift > 0.0:
            raise ValueError("PCEN.from_time_constant: time_constant_s and frame_shift_ms must be positive")
        T = np.float64(tc) / (np.float64(shift) / np.float64(1000.0))
        smooth = (np.sqrt(np.float64(1.0) + np.float64(4.0) * T * T) - np.float64(1.0)) / (np.float64(2.0) * T * T)
        return cls(smooth=float(smooth), **kw)

    # ---- packed ragged batches ------------------------------------------------------

    @staticmethod
    def _check_rows(torch, feats, row_offsets):
        if not _is_gpu_tensor(feats) or feats.dtype not in (torch.float32, torch.float64) or feats.dim() != 2:
            raise ValueError("feats must be a 2-D float32 or float64 GPU tensor")
        if feats.shape[1] and feats.stride(1) != 1:
            feats = feats.contiguous()
        R, C = feats.shape
        rows = np.ascontiguousarray(row_offsets, dtype=np.int64)
        if rows.ndim != 1 or len(rows) < 1 or (np.diff(rows) < 0).any() or rows[0] < 0 or rows[-1] > R:
            raise ValueError("row_offsets must be B + 1 ascending row indices within feats")
        stride = feats.stride(0) if R > 1 else C
        if stride < C:
            raise ValueError("rows of feats must not overlap")
        return feats, rows, stride

    def _smooth_into(self, torch, lib, feats, rows, stride, m):
        """the smoother's launches over the checked batch: M of every utterance into float64 `m`, ``(R, C)``"""
        R, C = feats.shape
        B = len(rows) - 1
        meta, _ = _rows_meta(rows, feats.device)
        fn = lib.pds_pcen_smooth_rows_f32 if feats.dtype == torch.float32 else lib.pds_pcen_smooth_rows_f64
        # one launch, unless the batch needs more lanes (utterances x C) than a grid has blocks for
        step = max(1, min(B, ((1 << 31) - 1) * 256 // C))
        with torch.cuda.device(feats.device):
            for lo in range(0, B, step):
                hi = min(B, lo + step)
                rc = fn(feats.data_ptr(), stride, meta[0, lo:].data_ptr(), meta[1, lo:].data_ptr(), hi - lo, C,
                        self.smooth_coeff, self.oms, m.data_ptr(), C, _stream(torch, feats))
                _native.check_stages2(rc, "pds_pcen_smooth_rows")

    def smooth_rows(self, feats, row_offsets):
        """The smoother's output M of every utterance of a packed ragged batch (step 2 of the definition): a float64
        GPU tensor shaped like `feats`.  `feats` and `row_offsets` as :func:`apply_rows` takes them; rows of `feats`
        outside ``row_offsets[0]:row_offsets[-1]`` are not written"""
        torch = _native.require_device()
        lib = _native.stages2_lib()
        feats, rows, stride = self._check_rows(torch, feats, row_offsets)
        R, C = feats.shape
        m = torch.empty((R, C), dtype=torch.float64, device=feats.device)
        if len(rows) > 1 and R and C and rows[-1] > rows[0]:
            self._smooth_into(torch, lib, feats, rows, stride, m)
        return m

    def apply_rows(self, feats, row_offsets, out=None):
        """Every utterance of a packed ragged batch normalised by itself, in two launches on the GPU

        `feats`: ``(total_rows, C)`` float32 or float64 GPU tensor (rows may be strided: a column slice of a wider
        tensor), utterance b in rows ``row_offsets[b]:row_offsets[b+1]``; empty and one-row utterances are allowed.
        Returns a tensor of the same shape and dtype (`out`, if given; it may be `feats` itself: the second launch is
        elementwise).  Rows outside ``row_offsets[0]:row_offsets[-1]`` are not written.
        """
        torch = _native.require_device()
        lib = _native.stages2_lib()
        feats, rows, stride = self._check_rows(torch, feats, row_offsets)
        R, C = feats.shape
        if out is None:
            out = torch.empty((R, C), dtype=feats.dtype, device=feats.device)
        elif (not _is_gpu_tensor(out) or out.dtype != feats.dtype or out.device != feats.device
              or tuple(out.shape) != (R, C) or (C and out.stride(1) != 1)):
            raise ValueError("out must be a GPU tensor of feats' shape, dtype and device with contiguous rows")
        out_stride = out.stride(0) if R > 1 else C
        if out_stride < C:
            raise ValueError("rows of out must not overlap")
        first, last = int(rows[0]), int(rows[-1])
        if len(rows) <= 1 or R == 0 or C == 0 or last == first:
            return out
        m = torch.empty((R, C), dtype=torch.float64, device=feats.device)
        self._smooth_into(torch, lib, feats, rows, stride, m)
        fn = lib.pds_pcen_compress_rows_f32 if feats.dtype == torch.float32 else lib.pds_pcen_compress_rows_f64
        with torch.cuda.device(feats.device):
            rc = fn(feats[first:].data_ptr(), stride, m[first:].data_ptr(), C, last - first, C, self.gain, self.bias,
                    self.power, self.eps, self.bp, out[first:].data_ptr(), out_stride, _stream(torch, feats))
            _native.check_stages2(rc, "pds_pcen_compress_rows")
        return out

    # ---- arrays and tensors ---------------------------------------------------------

    @staticmethod
    def _device_rows(features, axis, who="PCEN"):
        """`features` on the device as ``(B * T, C)`` rows with time in front of the columns -> (on_gpu, features, rows,
        B, T, the shape with time moved to -2)"""
        on_gpu = _is_gpu_tensor(features)
        if not on_gpu:
            features = np.asarray(features)
        shape = tuple(features.shape)
        if len(shape) not in (2, 3):
            raise ValueError(f"{who}: expected a 2-D or 3-D array or tensor")
        axis = axis % len(shape)
        torch = _native.require_device()
        if on_gpu:
            t = features if features.dtype in (torch.float32, torch.float64) else features.to(torch.float64)
        else:
            t = _to_device(features if features.dtype in (np.float32, np.float64) else features.astype(np.float64))
        # time in front of the last axis; what is in front of time are utterances, what is behind it columns
        moved = t.movedim(axis, -2)
        lead = tuple(moved.shape)
        T, C = lead[-2], lead[-1]
        B = lead[0] if len(lead) == 3 else 1
        if moved.dim() == 2 and moved.stride(1) == 1 and (moved.stride(0) >= C or T <= 1):
            rows = moved  # a matrix whose rows are contiguous goes as it is, whatever its row stride
        else:
            rows = moved.reshape(B * T, C).contiguous()
        return on_gpu, features, rows, B, T, lead

    def smooth(self, features, axis: int = -1):
        """The smoother's output M (step 2 of the definition) as float64, shaped like `features`: a numpy array for an
        array, a GPU tensor for a GPU tensor"""
        on_gpu, _, rows, B, T, lead = self._device_rows(features, axis)
        m = self.smooth_rows(rows, np.arange(B + 1, dtype=np.int64) * T)
        m = m.reshape(lead).movedim(-2, axis % len(lead))
        return m if on_gpu else m.cpu().numpy()

    def apply(self, features, axis: int = -1, in_place: bool = False):
        on_gpu, features, rows, B, T, lead = self._device_rows(features, axis)
        out = self.apply_rows(rows, np.arange(B + 1, dtype=np.int64) * T)
        return _finish_rows(out, lead, axis, on_gpu, features, in_place)


def _finish_rows(out, lead, axis, on_gpu, features, in_place):
    """the packed result `out` of ``PCEN._device_rows``'s rows in `features`' shape and kind"""
    out = out.reshape(lead).movedim(-2, axis % len(lead))
    if on_gpu:
        if in_place and features.dtype == out.dtype:
            features.copy_(out)
            return features
        return out
    res = out.cpu().numpy()
    if in_place and features.dtype == res.dtype and features.flags.writeable:
        features[...] = res
        return features
    return res


# ------------------------------------------------------------------ PLP --------------

_PLP_MAX_WIDTH = 256  # columns of an input row pds_plp_rows serves (include/pds_amd_stages4.h)
_PLP_MAX_ORDER = 32  # ... and the largest LPC order
_PLP_BLOCK_ROWS = 64  # rows of a block of it (pds_plp_block_rows, csrc/plp_rule.h)
_PLP_MAX_BLOCKS = (1 << 31) - 1  # ... and the blocks one call of it may launch


def _plp_int(value, what, lo, hi):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not lo <= value <= hi:
        raise ValueError(f"PLP: {what} must be an integer in [{lo}, {hi}], got {value!r}")
    return int(value)


def _plp_number(value, what):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"PLP: {what} must be a number, got {value!r}")
    return float(value)


def _plp_lifter(value, what):
    # (as Cepstra checks its lifter: a number, finite, not negative)
    value = _plp_number(value, what)
    if not np.isfinite(value) or value < 0:
        raise ValueError(f"PLP: {what} must be finite and not negative, got {value!r}")
    return value


class PLP(PostProcessor):
    """Perceptual linear prediction (PLP) cepstra of linear filter-bank energies, modelled on Kaldi's
    ``feature-plp.cc``: an equal-loudness weighting, a root compression, an inverse DFT to autocorrelations, the
    Levinson-Durbin recursion and the LPC-to-cepstrum recursion, row by row, in one HIP kernel of the fourth stages
    library (``csrc/plp.hip``)

    `axis` of :func:`apply` is the *coefficient* axis, of width W; it becomes `num_ceps` wide, every other axis is
    kept.  The input is the linear energies of a computer built with ``use_log=False`` (``use_power=True`` gives
    Kaldi's PLP).  float32 and float64 keep their dtype; anything else is computed and returned as float64.

    The definition.

    Notation for a row `x` of width `W`:

    - `copy = int(energy)`
    - `F = W − copy ≥ 1`
    - `D = F + 2`
    - `p = lpc_order`
    - `K = num_ceps`

    Refused with `ValueError`, before any device work:

    - `W > 256`
    - `p` outside `[1, min(F + 1, 32)]`
    - `K` outside `[1, p + 1]`
    - `compress_factor` not finite or not positive
    - `floor` not positive
    - `lifter` or `scale` as `Cepstra` checks its `lifter`
    - `equal_loudness=True` without `F` centre frequencies

    Host tables, float64, built once per `(width, device)`:

    - `w[f]`, the equal-loudness weight.
      - It is `1.0` when `equal_loudness=False`.
      - Otherwise `fsq = c_f²`, `fs = fsq / (fsq + 1.6e5)` and `w[f] = fs · fs · ((fsq + 1.44e6) / (fsq + 9.61e6))` for
        centre `c_f` in Hz.
    - `B[i][j]` for `0 ≤ i ≤ p`, `0 ≤ j < D`, with `s = 1 / (2 (D − 1))` and `θ = π / (D − 1)`:
      - `B[i][0] = s`
      - `B[i][j] = 2 s cos(θ i j)` for `0 < j < D − 1`
      - `B[i][D−1] = s cos(θ i (D − 1))`
    - `L[k] = scale · (1 + 0.5 Q sin(π k / Q))` with `Q = lifter`, for `0 ≤ k < K`.
      - `lifter` of `0` or `None` means no lifter: `L[k] = scale`.

    Per row, float64 throughout. Every operation is rounded by itself (no contraction: `-ffp-contract=off` for the
    object).

    1. Widen the row exactly: `e[f] = float64(x[copy + f])`.
    2. Floor: `g[f] = (e[f] < floor) ? floor : e[f]`. A NaN passes.
    3. Compress: `h[f] = pow(g[f] · w[f], compress_factor)`. The product is rounded once, then the device's `pow`.
    4. Duplicate the edges: `d[0] = h[0]`, `d[1 + f] = h[f]`, `d[D − 1] = h[F − 1]`.
    5. Autocorrelation: `r[i]` starts at `+0.0` and takes `r[i] = r[i] + B[i][j] · d[j]` for `j = 0 … D − 1`, in that
       order.
    6. Durbin. `E = r[0]`. For `i = 0 … p − 1`:
       1. `k = r[i+1]`, then `k = k + a[j] · r[i − j]` for `j = 0 … i − 1`.
       2. `k = k / E`.
       3. `c = 1 − k · k`, then `c = (c < 1e-5) ? 1e-5 : c`.
       4. `E = E · c`.
       5. `t[i] = −k`, and `t[j] = a[j] − k · a[i − j − 1]` for `j < i`.
       6. `a[0..i] = t[0..i]`.
    7. Cepstrum. For `i = 0 … p − 1`:
       1. `s = +0.0`.
       2. `s = s + (double(i − j) · a[j]) · q[i − j − 1]` for `j = 0 … i − 1`.
       3. `q[i] = −a[i] − s / double(i + 1)`.
    8. Output, each value rounded once to the row's dtype.
       - Without `energy`: `out[0] = L[0] · log(E)`, using the device's `log`.
       - With `energy`: `out[0] = log((e0 < floor) ? floor : e0)`, where `e0` is the widened column 0. It is neither
         lifted nor scaled.
       - `out[k] = L[k] · q[k − 1]` for `1 ≤ k < K`.
       - The output width is `K`.

    Consequences:

    - Everything but the `pow` of step 3 and the `log` of step 8 is plain IEEE arithmetic, so numpy reproduces it bit
      for bit **given the same `d`**.
    - A row holding a NaN gives NaN in every computed column, and the clamp in step 6 is written so that it does.
    - A row holding +inf is only promised not to disturb other rows.
    - A row of zeros is finite, because of the floor.

    `centers_hz`: the filters' centre frequencies, ``bank.centers_hz`` of the computer; :func:`for_computer`,
    ``StreamBatch(plp=...)`` and the command-line tool take them from their computer when the object has none.
    `energy`: column 0 is the energy of a computer built with ``include_energy=True``; ``None``, the default, reads as
    ``False`` and lets those three take it from their computer too (:attr:`energy` is always a bool).

    :func:`apply`, :func:`apply_rows` and the streaming stage launch the same kernel, whose every instantiation inlines
    one row function (``csrc/plp_rule.h``): their results agree bit for bit.  :func:`apply_rows` takes an `aux` buffer
    for the row's `d` and final `E`, which is what makes the claim above checkable.
    """

    aliases = {"plp", "plp_cepstra", "rasta_plp_off"}

    def __init__(self, num_ceps: int = 13, lpc_order: int = 12, compress_factor: float = 1.0 / 3.0,
                 lifter: Optional[float] = 22.0, scale: float = 1.0, equal_loudness: bool = True, centers_hz=None,
                 floor: float = 2.0 ** -126, energy: Optional[bool] = None):
        self.lpc_order = _plp_int(lpc_order, "lpc_order", 1, _PLP_MAX_ORDER)
        self.num_ceps = _plp_int(num_ceps, "num_ceps", 1, self.lpc_order + 1)
        self.compress_factor = _plp_number(compress_factor, "compress_factor")
        if not np.isfinite(self.compress_factor) or not self.compress_factor > 0.0:
            raise ValueError(f"PLP: compress_factor must be finite and positive, got {compress_factor!r}")
        self.floor = _plp_number(floor, "floor")
        if not self.floor > 0.0 or not np.isfinite(self.floor):
            raise ValueError(f"PLP: floor must be positive and finite, got {floor!r}")
        self.lifter = _plp_lifter(0.0 if lifter is None else lifter, "lifter")
        self.scale = _plp_lifter(scale, "scale")
        if not isinstance(equal_loudness, (bool, np.bool_)):
            raise ValueError(f"PLP: equal_loudness must be a bool, got {equal_loudness!r}")
        self.equal_loudness = bool(equal_loudness)
        if energy is not None and not isinstance(energy, (bool, np.bool_)):
            raise ValueError(f"PLP: energy must be a bool or None, got {energy!r}")
        self._energy_given = energy is not None
        self.energy = bool(energy)
        if centers_hz is not None:
            try:
                centers = np.asarray(centers_hz, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"PLP: centers_hz must be a sequence of frequencies in Hz, got {centers_hz!r}")
            if centers.ndim != 1 or not len(centers) or not np.isfinite(centers).all() or (centers < 0).any():
                raise ValueError("PLP: centers_hz must be a non-empty sequence of finite frequencies in Hz, none negative")
            centers_hz = tuple(float(c) for c in centers)
        self.centers_hz = centers_hz
        self._device_tables = {}  # (width, device) -> device float64 w[F], B[p + 1, D], L[K]

    # ---- what a computer knows ------------------------------------------------------

    def _arguments(self) -> dict:
        return dict(num_ceps=self.num_ceps, lpc_order=self.lpc_order, compress_factor=self.compress_factor,
                    lifter=self.lifter, scale=self.scale, equal_loudness=self.equal_loudness,
                    centers_hz=self.centers_hz, floor=self.floor, energy=self.energy if self._energy_given else None)

    def bound_to(self, computer) -> "PLP":
        """This object with what it leaves open taken from `computer` (a frame computer over a filter bank): the centre
        frequencies from ``computer.bank.centers_hz`` if it has none and weights by them, `energy` from
        ``computer.includes_energy`` if it was not given.  The object itself if nothing was open; it is not changed.
        ``ValueError`` for a computer that takes logs"""
        refuse_log_computer(computer, "PLP")
        args = self._arguments()
        if args["energy"] is None:
            args["energy"] = bool(getattr(computer, "includes_energy", False))
        if args["centers_hz"] is None and self.equal_loudness:
            args["centers_hz"] = tuple(float(c) for c in computer.bank.centers_hz)
        if args["centers_hz"] == self.centers_hz and self._energy_given:
            return self
        return PLP(**args)

    @classmethod
    def for_computer(cls, computer, **kw) -> "PLP":
        """``PLP(**kw)`` for the rows of `computer`: `centers_hz` from ``computer.bank.centers_hz`` and `energy` from
        ``computer.includes_energy`` unless given; ``ValueError`` for a computer that takes logs"""
        return cls(**kw).bound_to(computer)

    # ---- the host tables ------------------------------------------------------------

    def aux_width(self, width: int) -> int:
        """columns of :func:`apply_rows`' `aux` for input rows of `width` columns: ``D + 1 = F + 3``"""
        return int(width) - int(self.energy) + 3

    def _split(self, width: int) -> Tuple[int, int]:
        """``(F, copy)`` of input rows of `width` columns, or ``ValueError``: the width is only known at apply"""
        width, copy = int(width), int(self.energy)
        F = width - copy
        if width > _PLP_MAX_WIDTH:
            raise ValueError(f"PLP: rows of {width} coefficients; at most {_PLP_MAX_WIDTH} are served")
        if F < 1:
            raise ValueError(f"PLP: rows of {width} coefficients{' (the energy among them)' if copy else ''} hold no "
                             "filter-bank energy")
        if self.lpc_order > F + 1:
            raise ValueError(f"PLP: lpc_order = {self.lpc_order} needs at least {self.lpc_order - 1} filter-bank "
                             f"energies, got {F}")
        if self.equal_loudness and (self.centers_hz is None or len(self.centers_hz) != F):
            have = "none" if self.centers_hz is None else str(len(self.centers_hz))
            raise ValueError(f"PLP: equal_loudness needs the {F} centre frequencies of the filters (centers_hz), got "
                             f"{have}: PLP.for_computer(computer) takes them from the bank")
        return F, copy

    def tables(self, width: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The float64 host tables ``(w[F], B[p + 1, D], L[K])`` of the definition for rows of `width` columns"""
        F, _ = self._split(width)
        D, p = F + 2, self.lpc_order
        if self.equal_loudness:
            c = np.asarray(self.centers_hz, dtype=np.float64)
            fsq = c * c
            fs = fsq / (fsq + 1.6e5)
            w = fs * fs * ((fsq + 1.44e6) / (fsq + 9.61e6))
        else:
            w = np.ones(F, dtype=np.float64)
        s = 1.0 / (2 * (D - 1))
        theta = math.pi / (D - 1)
        # (the C library's cos and sin, one call an element: an array call may take another code path with other
        # roundings, and the tables are part of the definition)
        B = np.empty((p + 1, D), dtype=np.float64)
        for i in range(p + 1):
            B[i, 0] = s
            for j in range(1, D - 1):
                B[i, j] = 2.0 * s * math.cos(theta * i * j)
            B[i, D - 1] = s * math.cos(theta * i * (D - 1))
        L = np.full(self.num_ceps, self.scale, dtype=np.float64)
        if self.lifter:
            for k in range(self.num_ceps):
                L[k] = self.scale * (1.0 + 0.5 * self.lifter * math.sin(math.pi * k / self.lifter))
        return np.ascontiguousarray(w), np.ascontiguousarray(B), np.ascontiguousarray(L)

    def _tables_on(self, width, device):
        key = (int(width), str(device))
        if key not in self._device_tables:
            tables = self.tables(width)
            torch = _native.require_device()
            self._device_tables[key] = tuple(torch.from_numpy(t).to(device) for t in tables)
        return self._device_tables[key]

    # ---- packed rows ----------------------------------------------------------------

    def apply_rows(self, feats, row_offsets=None, out=None, aux=None):
        """The rows of a packed batch, each by itself, in one launch on the GPU

        `feats`: ``(total_rows, W)`` float32 or float64 GPU tensor (rows may be strided: a column slice of a wider
        tensor).  `row_offsets`: the utterances' ``B + 1`` ascending row indices, of which only the first and the last
        matter here -- a row depends on nothing but itself --, or ``None`` for every row.  Returns ``(total_rows,
        num_ceps)`` of `feats`' dtype (`out`, if given: its rows contiguous, possibly strided, not overlapping `feats`);
        rows outside ``row_offsets[0]:row_offsets[-1]`` and columns past `num_ceps` of a wider `out` are not written.
        `aux`: ``None`` or a contiguous float64 GPU tensor ``(total_rows, aux_width(W))`` that takes the row's
        ``d[0 .. D - 1]`` and its final ``E``.
        """
        F, copy = self._split(feats.shape[1]) if getattr(feats, "ndim", 0) == 2 else (0, 0)
        torch = _native.require_device()
        lib = _native.stages4_lib()
        if not _is_gpu_tensor(feats) or feats.dtype not in (torch.float32, torch.float64) or feats.dim() != 2:
            raise ValueError("feats must be a 2-D float32 or float64 GPU tensor")
        if feats.stride(1) != 1:
            feats = feats.contiguous()
        R, W = feats.shape
        K = self.num_ceps
        stride = feats.stride(0) if R > 1 else W
        if stride < W:
            raise ValueError("rows of feats must not overlap")
        first, last = 0, R
        if row_offsets is not None:
            rows = np.ascontiguousarray(row_offsets, dtype=np.int64)
            if rows.ndim != 1 or len(rows) < 1 or (np.diff(rows) < 0).any() or rows[0] < 0 or rows[-1] > R:
                raise ValueError("row_offsets must be B + 1 ascending row indices within feats")
            first, last = int(rows[0]), int(rows[-1])
        if out is None:
            out = torch.empty((R, K), dtype=feats.dtype, device=feats.device)
        elif (not _is_gpu_tensor(out) or out.dtype != feats.dtype or out.device != feats.device
              or tuple(out.shape) != (R, K) or out.stride(1) != 1):
            raise ValueError("out must be a GPU tensor of (rows of feats, num_ceps), feats' dtype and device, with "
                             "contiguous rows")
        out_stride = out.stride(0) if R > 1 else K
        if out_stride < K:
            raise ValueError("rows of out must not overlap")
        if R and out.untyped_storage().data_ptr() == feats.untyped_storage().data_ptr():
            raise ValueError("out must not share feats' memory: the shape changes, nothing is done in place")
        if aux is not None and (not _is_gpu_tensor(aux) or aux.dtype != torch.float64 or aux.device != feats.device
                                or tuple(aux.shape) != (R, F + 3) or not aux.is_contiguous()):
            raise ValueError(f"aux must be a contiguous float64 GPU tensor of shape ({R}, {F + 3}) on feats' device")
        if last == first:
            return out
        d_w, d_B, d_L = self._tables_on(W, feats.device)
        fn = lib.pds_plp_rows_f32 if feats.dtype == torch.float32 else lib.pds_plp_rows_f64
        step = _PLP_BLOCK_ROWS * _PLP_MAX_BLOCKS  # one launch, unless there are more rows than a grid has blocks for
        with torch.cuda.device(feats.device):
            for lo in range(first, last, step):
                n = min(last, lo + step) - lo
                rc = fn(feats[lo:].data_ptr(), stride, n, F, copy, d_w.data_ptr(), d_B.data_ptr(), d_L.data_ptr(),
                        self.lpc_order, K, self.compress_factor, self.floor, out[lo:].data_ptr(), out_stride,
                        aux[lo:].data_ptr() if aux is not None else None, _stream(torch, feats))
                _native.check_stages4(rc, "pds_plp_rows")
        return out

    # ---- arrays and tensors ---------------------------------------------------------

    def apply(self, features, axis: int = -1, in_place: bool = False):
        # (`in_place` is accepted and ignored: the shape changes)
        on_gpu = _is_gpu_tensor(features)
        if not on_gpu:
            features = np.asarray(features)
        shape = tuple(features.shape)
        if not shape:
            raise ValueError("PLP: expected at least one dimension")
        axis = axis % len(shape)
        W = shape[axis]
        self._split(W)  # (the width's errors come before any device work)
        torch = _native.require_device()
        if on_gpu:
            t = features if features.dtype in (torch.float32, torch.float64) else features.to(torch.float64)
        else:
            t = _to_device(features if features.dtype in (np.float32, np.float64) else features.astype(np.float64))
        rows = t.movedim(axis, -1)
        lead = tuple(rows.shape[:-1])
        # a matrix whose rows are contiguous goes as it is, whatever its row stride (a column slice of a wider
        # tensor); anything else as a contiguous (rows, W) copy
        if not (rows.dim() == 2 and rows.stride(1) == 1 and (rows.stride(0) >= W or rows.shape[0] <= 1)):
            rows = rows.reshape(int(np.prod(lead, dtype=np.int64)), W).contiguous()
        out = self.apply_rows(rows)
        out = out.reshape(lead + (self.num_ceps,)).movedim(-1, axis)
        return out if on_gpu else out.cpu().numpy()


# ------------------------------------------------------------------ SpecAugment ------

_SPECAUG_TILE = 32  # rows of a block's tile of pds_specaug_apply_rows (pds_specaug_tile_rows, csrc/specaug_rule.h)
_SPECAUG_MAX_BLOCKS = (1 << 31) - 1  # ... and the blocks one call of it may launch
_SPECAUG_MAX_MASKS = 16
_SPECAUG_MAX_WIDTH = (1 << 31) - 2
_SPECAUG_MAX_WARP = 1 << 29
_SPECAUG_MAX_ROWS = (1 << 31) - 1  # rows of an utterance the draws are defined for


def _specaug_int(value, what, hi):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"SpecAugment: {what} must be an integer, got {value!r}")
    value = int(value)
    if not 0 <= value <= hi:
        raise ValueError(f"SpecAugment: {what} must lie in [0, {hi}], got {value!r}")
    return value


def _specaug_spans(nrows, limit=None):
    """``[(lo, hi, max_rows), ...]``: the batch cut into launches of at most `limit` blocks each, one block per
    (utterance, tile of ``_SPECAUG_TILE`` rows of the span's longest utterance).  Greedy and in order; an utterance of
    fewer than 2^31 rows always fits a launch of its own"""
    limit = _SPECAUG_MAX_BLOCKS if limit is None else limit
    if len(nrows) and len(nrows) * -(-int(np.max(nrows)) // _SPECAUG_TILE) <= limit:
        return [(0, len(nrows), int(np.max(nrows)))]  # (what nearly every batch is: one launch)
    spans, lo, longest = [], 0, 0
    for b, n in enumerate(int(n) for n in nrows):
        grown = max(longest, n)
        if b > lo and (b + 1 - lo) * -(-grown // _SPECAUG_TILE) > limit:
            spans.append((lo, b, longest))
            lo, grown = b, n
        longest = grown
    if len(nrows) > lo:
        spans.append((lo, len(nrows), longest))
    return spans


class SpecAugment(_pre._Seeded, PostProcessor):
    """SpecAugment (Park et al. 2019): a time warp, frequency masks and time masks over a feature matrix, for training

    `axis` of :func:`apply` is the *time* axis; the last remaining axis holds the columns.  The draws come from a
    counter-based generator keyed per utterance, as ``pre.Dither``'s noise does: an utterance's result depends on its key
    and nothing else, whatever the batch it stands in.  `seed` works as in ``Dither``: the object holds a state, and every
    utterance it augments without explicit seeds advances it.

    The definition.

    Per utterance of T ≥ 1 rows and C ≥ 1 columns with a 64-bit key k:

    0. Generator.
       - `P(i, d)` is one Philox4x32-10 block with counter words `(i, 0, d, 0)` and key words `(k mod 2³², k >> 32)`.
         Its output words are `r0..r3`. The round function is the one `csrc/dither_noise.h` already has.
       - `U(r, n) = (uint64(r) · uint64(n + 1)) >> 32` for 0 ≤ n < 2³¹. It is an integer in [0, n].
    1. Warp.
       - If `warp = W ≥ 1` and `T ≥ 2W + 3`, let `r = P(0, 1)`.
       - `w0 = W + 1 + U(r0, T − 3 − 2W)`.
       - `w1 = w0 − W + U(r1, 2W)`.
       - Then `W + 1 ≤ w0 ≤ T − 2 − W` and `1 ≤ w1 ≤ T − 2`.
       - Otherwise `w0 = w1 = −1` (no warp).
    2. Frequency mask j, 0 ≤ j < freq_masks.
       - `r = P(j, 2)`.
       - `f = U(r0, min(freq_width, C))`.
       - `f0 = U(r1, C − f)`.
       - The mask covers columns `[f0, f0 + f)`.
    3. Time mask j, 0 ≤ j < time_masks.
       - `b = min(time_width, (int64) floor(time_ratio · (double) T))`, the product rounded once.
       - `r = P(j, 3)`.
       - `t = U(r0, b)`.
       - `t0 = U(r1, T − t)`.
       - The mask covers rows `[t0, t0 + t)`.
    4. Warped value `v[t][c]`.
       - Without a warp, `v[t][c]` is `x[t][c]`, copied.
       - With one, the source position is float64 with every operation rounded by itself (no contraction):
         - for `t ≤ w1`: `s = ((double) t · (double) w0) / (double) w1`
         - for `t > w1`: `s = (double) w0 + ((double)(t − w1) · (double)(T − 1 − w0)) / (double)(T − 1 − w1)`
       - `i = floor(s)` and `a = s − i`.
       - If `a == 0`, the value is `x[i][c]`, copied.
       - Otherwise the value is `x[i][c] + a · (x[i+1][c] − x[i][c])`, with the samples widened exactly, the
         difference, product and sum each rounded once, and the result rounded once to the row type.
       - I checked on the CPU for every T < 60, W < 8 and every admissible (w0, w1) that:
         - s is strictly increasing,
         - s(0) = 0, s(w1) = w0 and s(T − 1) = T − 1 exactly,
         - `i + 1 ≤ T − 1` whenever `a > 0`.
    5. Mean (only for `fill="mean"`).
       - It is taken over the utterance's T · C input elements in float64, as 64 interleaved partial sums.
       - `p_j` sums the elements with flat index `e = t · C + c ≡ j (mod 64)`, in ascending e, starting from +0.0.
       - `s = ((+0.0 + p_0) + p_1) + … + p_63`.
       - `m = s / (double)(T · C)`.
       - This is the rule and the reason of §4.8. Lane j of one wave owns `p_j`, and the host restates it in a few
         lines.
    6. Output.
       - `out[t][c]` is the fill value, rounded once to the row type, if c lies in any frequency mask or t in any time
         mask.
       - Otherwise `out[t][c]` is `v[t][c]`.
       - T = 0 gives nothing.

    The plan (steps 1 to 3) is integers only.  Unmasked values without a warp, or at ``a == 0``, are copies, byte for
    byte: NaN payloads and signed zeros pass.  Everything else is plain IEEE float64 arithmetic, which numpy reproduces
    bit for bit; a computed NaN (such as inf - inf in the interpolation) is only promised to be a NaN.  Anything but
    float32 and float64 input is widened to float64 first.  An utterance of 2^31 rows or more is a ``ValueError``.

    Not a stage of batched streaming: a time mask's bound and the warp need T, and augmentation is a training-time
    stage.
    """

    aliases = {"specaugment", "spec_augment", "specaug"}
    _SEEDS_ERROR = "SpecAugment: one seed per utterance"

    def __init__(self, freq_masks: int = 2, freq_width: int = 10, time_masks: int = 2, time_width: int = 50,
                 time_ratio: float = 1.0, warp: int = 0, fill: Union[float, str] = 0.0, seed: Optional[int] = None):
        self.freq_masks = _specaug_int(freq_masks, "freq_masks", _SPECAUG_MAX_MASKS)
        self.freq_width = _specaug_int(freq_width, "freq_width", _SPECAUG_MAX_WIDTH)
        self.time_masks = _specaug_int(time_masks, "time_masks", _SPECAUG_MAX_MASKS)
        self.time_width = _specaug_int(time_width, "time_width", _SPECAUG_MAX_WIDTH)
        if isinstance(time_ratio, (bool, np.bool_)) or not isinstance(time_ratio, (int, float, np.integer, np.floating)):
            raise ValueError(f"SpecAugment: time_ratio must be a number, got {time_ratio!r}")
        self.time_ratio = float(time_ratio)
        if not 0.0 < self.time_ratio <= 1.0:
            raise ValueError(f"SpecAugment: time_ratio must lie in (0, 1], got {time_ratio!r}")
        self.warp = _specaug_int(warp, "warp", _SPECAUG_MAX_WARP)
        if isinstance(fill, str):
            if fill != "mean":
                raise ValueError(f'SpecAugment: fill must be a number or "mean", got {fill!r}')
            self.fill = "mean"
        elif isinstance(fill, (bool, np.bool_)) or not isinstance(fill, (int, float, np.integer, np.floating)):
            raise ValueError(f'SpecAugment: fill must be a number or "mean", got {fill!r}')
        else:
            self.fill = float(fill)  # (finite or not: a NaN or an infinity marks the masked elements as well)
        if seed is not None and (isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer))
                                 or int(seed) < 0):
            raise ValueError(f"SpecAugment: seed must be None or a non-negative integer, got {seed!r}")
        self._start_seed(seed)

    @property
    def plan_words(self) -> int:
        """int64 words of an utterance's plan: ``w0, w1``, ``(f0, f)`` per frequency mask, ``(t0, t)`` per time mask"""
        return 2 + 2 * self.freq_masks + 2 * self.time_masks

    def __repr__(self) -> str:
        # (what the object was built with and nothing of its state: a test id made of it is the same in every run)
        return (f"SpecAugment(freq_masks={self.freq_masks!r}, freq_width={self.freq_width!r}, "
                f"time_masks={self.time_masks!r}, time_width={self.time_width!r}, time_ratio={self.time_ratio!r}, "
                f"warp={self.warp!r}, fill={self.fill!r}, seed={self._given_seed!r})")

    # ---- packed ragged batches ------------------------------------------------------

    @staticmethod
    def _check_counts(nrows, C):
        nrows = np.ascontiguousarray(nrows, dtype=np.int64).reshape(-1)
        if isinstance(C, (bool, np.bool_)) or not isinstance(C, (int, np.integer)) or not 1 <= int(C) <= (1 << 31) - 1:
            raise ValueError(f"SpecAugment: C must be an integer in [1, 2^31 - 1], got {C!r}")
        if len(nrows) > (1 << 31) - 1:
            raise ValueError("SpecAugment: too many utterances")
        if len(nrows) and (nrows.min() < 0 or nrows.max() > _SPECAUG_MAX_ROWS):
            raise ValueError("SpecAugment: an utterance's row count must lie in [0, 2^31 - 1]")
        return nrows, int(C)

    def _plan_into(self, torch, lib, d_nrows, d_keys, B, C, device):
        """the plan kernel over B utterances whose counts and keys are on the device: an int64 ``(B, plan_words)``"""
        plan = torch.empty((B, self.plan_words), dtype=torch.int64, device=device)
        if B:
            with torch.cuda.device(device):
                rc = lib.pds_specaug_plan(d_nrows.data_ptr(), d_keys.data_ptr(), B, C, self.freq_masks, self.freq_width,
                                          self.time_masks, self.time_width, self.time_ratio, self.warp, plan.data_ptr(),
                                          torch.cuda.current_stream(device).cuda_stream)
            _native.check_stages3(rc, "pds_specaug_plan")
        return plan

    def plan_rows(self, nrows, C, seeds=None, device=None):
        """The plans of B utterances of ``nrows[b]`` rows and `C` columns (steps 1 to 3 of the definition): an int64 GPU
        tensor ``(B, 2 + 2 * freq_masks + 2 * time_masks)`` of ``w0, w1``, ``(f0, f)`` per frequency mask and ``(t0,
        t)`` per time mask.  With `seeds`, one integer per utterance, utterance b gets the plan of the first ``apply``
        of ``SpecAugment(..., seed=seeds[b])`` and this object's sequence is left alone; with ``seeds=None`` the
        sequence advances once per utterance, in order.  What :func:`apply_rows` takes as `plan`"""
        torch = _native.require_device()
        lib = _native.stages3_lib()
        nrows, C = self._check_counts(nrows, C)
        B = len(nrows)
        keys = self._keys(B, seeds)
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        table = torch.from_numpy(np.stack([nrows, keys.view(np.int64)])).to(device)  # counts and keys in one copy
        return self._plan_into(torch, lib, table[0], table[1], B, C, device)

    def mean_rows(self, feats, row_offsets):
        """The mean of every utterance of a packed ragged batch (step 5 of the definition): a float64 GPU tensor
        ``(B,)``, NaN for an empty utterance.  `feats` and `row_offsets` as :func:`apply_rows` takes them"""
        torch = _native.require_device()
        lib = _native.stages3_lib()
        feats, rows, stride = PCEN._check_rows(torch, feats, row_offsets)
        B, C = len(rows) - 1, feats.shape[1]
        self._check_counts(np.diff(rows), max(C, 1))
        mean = torch.empty((B,), dtype=torch.float64, device=feats.device)
        if B and C == 0:
            mean.fill_(float("nan"))
        elif B:
            meta, _ = _rows_meta(rows, feats.device)
            self._mean_into(torch, lib, feats, stride, meta[0], meta[1], B, mean)
        return mean

    @staticmethod
    def _mean_into(torch, lib, feats, stride, d_row_off, d_nrows, B, mean):
        fn = lib.pds_specaug_mean_rows_f32 if feats.dtype == torch.float32 else lib.pds_specaug_mean_rows_f64
        with torch.cuda.device(feats.device):
            rc = fn(feats.data_ptr(), stride, d_row_off.data_ptr(), d_nrows.data_ptr(), B, feats.shape[1],
                    mean.data_ptr(), _stream(torch, feats))
        _native.check_stages3(rc, "pds_specaug_mean_rows")

    def _apply_into(self, fn, nrows, C, d_in, in_stride, d_row_off, d_nrows, d_plan, d_mean, d_out, out_stride, stream):
        """the apply kernel's launches over the checked batch, every array by its address: one launch, unless the batch
        needs more blocks (utterances x tiles of the longest) than a grid holds; then span by span"""
        for lo, hi, longest in _specaug_spans(nrows, _SPECAUG_MAX_BLOCKS):
            rc = fn(d_in, in_stride, d_row_off + 8 * lo, d_nrows + 8 * lo, hi - lo, C,
                    d_plan + 8 * self.plan_words * lo, self.freq_masks, self.time_masks,
                    (d_mean + 8 * lo) if d_mean else None, 0.0 if self.fill == "mean" else self.fill, d_out, out_stride,
                    longest, stream)
            _native.check_stages3(rc, "pds_specaug_apply_rows")

    def apply_rows(self, feats, row_offsets, seeds=None, plan=None, out=None):
        """Every utterance of a packed ragged batch augmented by itself on the GPU: one upload of offsets, counts and
        keys, then two launches (three with ``fill="mean"``), no host synchronisation

        `feats`: ``(total_rows, C)`` float32 or float64 GPU tensor (rows may be strided: a column slice of a wider
        tensor), utterance b in rows ``row_offsets[b]:row_offsets[b+1]``; empty utterances are allowed.  `seeds` as
        :func:`plan_rows` takes them.  `plan`: the tensor a previous :func:`plan_rows` returned, in place of drawing one
        (the same masks on two views of an utterance; any plan a caller writes: a warp centre outside ``[1, T - 2]`` is
        no warp); `plan` together with `seeds` is a ``ValueError``, and with `plan` the object's sequence is left alone.
        Returns a tensor of the same shape and dtype (`out`, if given; it may be `feats` itself only where ``warp ==
        0``: a warped row reads its neighbours).  Rows outside ``row_offsets[0]:row_offsets[-1]`` are not written.
        """
        if plan is not None and seeds is not None:
            raise ValueError("SpecAugment: plan and seeds together: the plan holds what the seeds would draw")
        if out is not None and out is feats and self.warp > 0:
            raise ValueError("SpecAugment: out is feats under warp > 0: a warped row reads its neighbours")
        torch = _native.require_device()
        lib = _native.stages3_lib()
        feats, rows, stride = PCEN._check_rows(torch, feats, row_offsets)
        R, C = feats.shape
        B = len(rows) - 1
        nrows, _ = self._check_counts(np.diff(rows), max(C, 1))
        if seeds is not None and len(seeds) != B:
            raise ValueError("SpecAugment: one seed per utterance")
        if out is None:
            out = torch.empty((R, C), dtype=feats.dtype, device=feats.device)
        elif (not _is_gpu_tensor(out) or out.dtype != feats.dtype or out.device != feats.device
              or tuple(out.shape) != (R, C) or (C and out.stride(1) != 1)):
            raise ValueError("out must be a GPU tensor of feats' shape, dtype and device with contiguous rows")
        out_stride = out.stride(0) if R > 1 else C
        if out_stride < C:
            raise ValueError("rows of out must not overlap")
        if self.warp > 0 and R and C and out.data_ptr() == feats.data_ptr():
            raise ValueError("SpecAugment: out shares feats' memory under warp > 0: a warped row reads its neighbours")
        if plan is not None:
            if (not _is_gpu_tensor(plan) or plan.dtype != torch.int64 or plan.device != feats.device
                    or tuple(plan.shape) != (B, self.plan_words) or not plan.is_contiguous()):
                raise ValueError(f"plan must be a contiguous int64 GPU tensor ({B}, {self.plan_words}) on feats' device")
            keys = None
        else:
            keys = self._keys(B, seeds)
        if B == 0 or R == 0 or C == 0 or rows[-1] == rows[0]:
            return out
        if keys is None:
            meta, _ = _rows_meta(rows, feats.device)
        else:  # offsets, counts and keys go up in one copy (a key's bits travel as int64)
            meta = torch.from_numpy(np.stack([rows[:-1], nrows, keys.view(np.int64)])).to(feats.device)
            plan = self._plan_into(torch, lib, meta[1], meta[2], B, C, feats.device)
        mean = None
        if self.fill == "mean":
            mean = torch.empty((B,), dtype=torch.float64, device=feats.device)
            self._mean_into(torch, lib, feats, stride, meta[0], meta[1], B, mean)
        fn = lib.pds_specaug_apply_rows_f32 if feats.dtype == torch.float32 else lib.pds_specaug_apply_rows_f64
        with torch.cuda.device(feats.device):
            self._apply_into(fn, nrows, C, feats.data_ptr(), stride, meta[0].data_ptr(), meta[1].data_ptr(),
                             plan.data_ptr(), mean.data_ptr() if mean is not None else 0, out.data_ptr(), out_stride,
                             _stream(torch, feats))
        return out

    # ---- arrays and tensors ---------------------------------------------------------

    def apply(self, features, axis: int = -2, in_place: bool = False):
        """`features` augmented: 2-D, or 3-D where each slice along the remaining leading axis is an utterance of its
        own with the next key of the sequence.  `axis` is the time axis, the last remaining axis the columns.  A numpy
        array gives an array, a GPU tensor a tensor.  `in_place` only where ``warp == 0``"""
        if in_place and self.warp > 0:
            raise ValueError("SpecAugment: in_place under warp > 0: a warped row reads its neighbours")
        on_gpu, features, rows, B, T, lead = PCEN._device_rows(features, axis, "SpecAugment")
        out = self.apply_rows(rows, np.arange(B + 1, dtype=np.int64) * T)
        return _finish_rows(out, lead, axis, on_gpu, features, in_place)
