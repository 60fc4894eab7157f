"""A plain numpy restatement of windowed-sinc rate conversion as ``pre.Resample`` and ``include/pds_amd_stages.h``
define it (test infrastructure, CPU only), written from the definition's text: the table phase by phase and tap by tap
with ``math``, the conversion in float64 with every product and sum rounded separately, taps in ascending order."""
import math

import numpy as np

from tests.sliding_model import same_bits  # noqa: F401  (NaNs compare by position)


def table(from_rate, to_rate, num_zeros=6, rolloff=0.99):
    """``(in_unit, out_unit, first, ntaps, w)``: int32 ``first`` and ``ntaps`` per phase, float64 ``w`` of shape
    ``(out_unit, max_taps)`` with zeros behind each phase's taps"""
    g = math.gcd(from_rate, to_rate)
    in_unit, out_unit = from_rate // g, to_rate // g
    cutoff = rolloff * 0.5 * min(from_rate, to_rate)
    width = num_zeros / (2 * cutoff)
    first, ntaps, rows = [], [], []
    for p in range(out_unit):
        t = p / to_rate
        lo = math.ceil((t - width) * from_rate)
        hi = math.floor((t + width) * from_rate)
        row = []
        for j in range(hi - lo + 1):
            d = (lo + j) / from_rate - t
            f = 2 * cutoff if d == 0 else math.sin(2 * math.pi * cutoff * d) / (math.pi * d)
            h = 0.5 * (1 + math.cos(2 * math.pi * cutoff / num_zeros * d)) if abs(d) < width else 0.0
            row.append(f * h / from_rate)
        first.append(lo)
        ntaps.append(hi - lo + 1)
        rows.append(row)
    w = np.zeros((out_unit, max(ntaps)), dtype=np.float64)
    for p, row in enumerate(rows):
        w[p, : len(row)] = row
    return in_unit, out_unit, np.asarray(first, dtype=np.int32), np.asarray(ntaps, dtype=np.int32), w


def num_output_samples(n, from_rate, to_rate):
    """``ceil(n * to_rate / from_rate)`` in integers"""
    return -(-n * to_rate // from_rate)


def resample(x, from_rate, to_rate, num_zeros=6, rolloff=0.99, weights=None):
    """The resampled 1-D signal `x` (float32, float64 or int16; int16 gives float32).  `weights`, where given, stands
    in for the table's ``w`` (the kernel is judged on its arithmetic with the table it was given, not on ``sin``)."""
    x = np.asarray(x)
    assert x.ndim == 1 and x.dtype in (np.float32, np.float64, np.int16)
    out_dtype = np.float64 if x.dtype == np.float64 else np.float32
    in_unit, out_unit, first, ntaps, w = table(from_rate, to_rate, num_zeros, rolloff)
    if weights is not None:
        assert weights.shape == w.shape and weights.dtype == np.float64
        w = weights
    n = len(x)
    m = num_output_samples(n, from_rate, to_rate)
    xd = x.astype(np.float64)
    k = np.arange(m, dtype=np.int64)
    u, p = k // out_unit, k % out_unit
    base = first[p].astype(np.int64) + u * in_unit
    y = np.zeros(m, dtype=np.float64)  # +0.0
    with np.errstate(all="ignore"):  # (NaN and infinite samples are part of the contract; the suite raises on warnings)
        for j in range(w.shape[1]):
            idx = base + j
            has = (j < ntaps[p]) & (idx >= 0) & (idx < n)  # any other tap contributes nothing
            y[has] = y[has] + w[p[has], j] * xd[idx[has]]
        return y.astype(out_dtype)


def resample_scalar(x, from_rate, to_rate, num_zeros=6, rolloff=0.99):
    """:func:`resample` as the scalar double loop of the text (for the model's own check)"""
    x = np.asarray(x)
    out_dtype = np.float64 if x.dtype == np.float64 else np.float32
    in_unit, out_unit, first, ntaps, w = table(from_rate, to_rate, num_zeros, rolloff)
    n = len(x)
    y = np.zeros(num_output_samples(n, from_rate, to_rate), dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(len(y)):
            u, p = divmod(k, out_unit)
            s = np.float64(0.0)
            for j in range(int(ntaps[p])):
                i = int(first[p]) + u * in_unit + j
                if 0 <= i < n:
                    s = s + w[p, j] * np.float64(x[i])
            y[k] = s
        return y.astype(out_dtype)


def due(n, in_unit, out_unit, first, ntaps):
    """The outputs due after `n` samples of a stream: the k whose last input index is at most ``n - 1``, counted by a
    scan over every k that could be (none beyond ``ceil(n * out_unit / in_unit)`` plus a unit is)"""
    count = 0
    for k in range(-(-n * out_unit // in_unit) + out_unit):
        u, p = divmod(k, out_unit)
        if int(first[p]) + u * in_unit + int(ntaps[p]) - 1 <= n - 1:
            count += 1
    return count
