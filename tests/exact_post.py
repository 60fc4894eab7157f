"""Plain numpy restatements of the offline post-processor kernels (csrc/post.hip), every operation rounded separately
in float64, for the tests that hold those kernels to the bit (tests/test_gpu_post_shapes.py; CPU checks of this module
itself in tests/test_exact_post.py).

Two kinds of CMVN input make a summation order-independent check possible:

* integer-valued, ``|x| <= 2048``: with ``count * 2048**2 < 2**53`` every partial sum of x and of x * x, in any order,
  is an integer below 2**53 and so exact in float64 -- the statistics equal the integer sums whatever the kernel's
  slabs, phases and unrolling (:func:`exact_sums`, :func:`exactness_holds`);
* random float32 values: x * x is exact in float64, and n terms summed in ANY order land within
  ``gamma_(n-1) * sum |term| <= n * 2**-52 * sum |term|`` of the true sum (Higham, Accuracy and Stability of Numerical
  Algorithms, section 4.2; the factor 2 over n * 2**-53 covers gamma's denominator for every n < 2**51 and the
  rounding of the reference sum itself) -- :func:`fsum_columns`, :func:`sum_bound`.
"""
import math

import numpy as np

MAX_ABS = 2048  # integer-valued inputs lie in [-MAX_ABS, MAX_ABS]


# ------------------------------------------------------------------ Deltas -----------


def delta_filters(num_deltas, context_window):
    """the order 1 .. num_deltas filters as ``post.Deltas`` builds them (order k has 2 k W + 1 taps)"""
    ramp = np.arange(1 + 2 * context_window, dtype=np.float64)
    ramp -= context_window
    ramp /= np.sum(ramp ** 2)
    filts = [np.ones(1, dtype=np.float64)]
    for _ in range(num_deltas):
        filts.append(np.convolve(filts[-1], ramp))
    return filts[1:]


def deltas_ref(x, axis, filts, pad_mode="edge", **pad_kwargs):
    """``[x, order 1, order 2, ..]``: x widened to float64, padded along `axis` by each order's own reach with
    :func:`numpy.pad`, ``acc = 0.0; for j ascending: acc = acc + w[j] * x[t + j]`` (product and sum rounded
    separately), cast back to x's dtype"""
    x = np.asarray(x)
    wide = np.moveaxis(x, axis, 0).astype(np.float64)
    T = wide.shape[0]
    pieces = [x]
    with np.errstate(invalid="ignore"):  # (0 * inf and inf - inf are NaN here as they are on the device)
        for w in filts:
            reach = (len(w) - 1) // 2
            padded = np.pad(wide, [(reach, reach)] + [(0, 0)] * (wide.ndim - 1), pad_mode, **pad_kwargs)
            acc = np.zeros_like(wide)
            for j in range(len(w)):
                acc = acc + w[j] * padded[j : j + T]
            pieces.append(np.moveaxis(acc, 0, axis).astype(x.dtype))
    return pieces


def deltas_layout(pieces, target_axis, concatenate):
    return np.concatenate(pieces, target_axis) if concatenate else np.stack(pieces, target_axis)


# ------------------------------------------------------------------ CMVN -------------


def exactness_holds(count):
    """every partial sum of `count` integer-valued terms (and of their squares) is exact in float64"""
    return count * MAX_ABS ** 2 < 2 ** 53


def exact_sums(x, axis):
    """per-coefficient sums of x and of x * x over every axis but `axis`, as lists of Python integers"""
    x = np.asarray(x)
    ints = x.astype(np.int64)
    assert np.array_equal(ints, x) and (np.abs(ints) <= MAX_ABS).all(), "integer-valued input expected"
    cols = np.moveaxis(ints, axis, 0).reshape(ints.shape[axis], -1)
    assert cols.shape[1] * MAX_ABS ** 2 < 2 ** 62  # (int64 holds the sums)
    return [int(v) for v in cols.sum(axis=1)], [int(v) for v in (cols * cols).sum(axis=1)]


def scale_shift(s1, s2, count, norm_var=True):
    """``(scale, mean * scale, zero-variance mask)`` per coefficient, as the host (post.py Standardize.apply) and
    cmvn_rows_kernel compute them: mean = s1 / count, var = s2 / count - mean * mean, |var| <= 1e-8 -> 1
    (``numpy.isclose(var, 0)``), scale = 1 / sqrt(var); every operation rounded separately.  `count` may broadcast
    against the sums (one count per utterance)"""
    s1 = np.asarray(s1, dtype=np.float64)
    s2 = np.asarray(s2, dtype=np.float64)
    count = np.asarray(count, dtype=np.float64)
    mean = s1 / count
    if norm_var:
        square = mean * mean
        var = s2 / count - square
        zero = np.abs(var) <= 1e-8
        var = np.where(zero, 1.0, var)
        scale = 1.0 / np.sqrt(var)
    else:
        zero = np.zeros(mean.shape, dtype=bool)
        scale = np.ones_like(mean)
    return scale, mean * scale, zero


def cmvn_from_sums(x, s1, s2, count, norm_var=True, axis=-1):
    """``y = x * scale - mean * scale`` in float64, two roundings, from the given sums (:func:`scale_shift`)"""
    x = np.asarray(x).astype(np.float64)
    scale, shift, _ = scale_shift(s1, s2, count, norm_var)
    shape = [1] * x.ndim
    shape[axis] = -1
    product = x * scale.reshape(shape)
    return product - shift.reshape(shape)


def cmvn_rows_ref(x, row_offsets, norm_var=True):
    """per-utterance CMVN of integer-valued packed rows ``(total, C)``: ``(y float64, pairs of (utterance, column)
    with zero variance, s1, s2)`` -- the integer sums per utterance, then :func:`scale_shift` with one count each"""
    x = np.asarray(x)
    ints = x.astype(np.int64)
    assert np.array_equal(ints, x) and (np.abs(ints) <= MAX_ABS).all(), "integer-valued input expected"
    rows = np.asarray(row_offsets, dtype=np.int64)
    nrows = np.diff(rows)
    assert exactness_holds(int(nrows.max(initial=0)))
    utt = np.repeat(np.arange(len(nrows)), nrows)
    s1 = np.zeros((len(nrows), x.shape[1]), dtype=np.int64)
    s2 = np.zeros_like(s1)
    span = ints[rows[0] : rows[-1]]
    np.add.at(s1, utt, span)
    np.add.at(s2, utt, span * span)
    live = nrows > 0
    y = np.zeros(x.shape, dtype=np.float64)
    scale, shift, zero = scale_shift(s1[live], s2[live], nrows[live, None], norm_var)
    at = np.repeat(np.arange(int(live.sum())), nrows[live])
    product = span.astype(np.float64) * scale[at]
    y[rows[0] : rows[-1]] = product - shift[at]
    return y, int(zero.sum()), s1, s2


def fsum_columns(x, axis):
    """correctly rounded per-coefficient ``(sum x, sum x * x, sum |x|, terms)`` of float32-valued x"""
    x = np.asarray(x)
    assert np.array_equal(x.astype(np.float32), x), "float32 values expected: their squares are exact in float64"
    cols = np.moveaxis(x.astype(np.float64), axis, 0).reshape(x.shape[axis], -1)
    s1 = np.array([math.fsum(c) for c in cols.tolist()])
    s2 = np.array([math.fsum(c) for c in (cols * cols).tolist()])
    a1 = np.array([math.fsum(c) for c in np.abs(cols).tolist()])
    return s1, s2, a1, cols.shape[1]


def sum_bound(n, abs_sum):
    """how far n terms added in any order, each addition rounded to float64, may land from their true sum"""
    return n * 2.0 ** -52 * np.asarray(abs_sum, dtype=np.float64)


def slabs_for(outer):
    """``(slabs, rows per slab)`` of the two-stage global sum: csrc/post.hip slabs_for and cmvn_partial_kernel"""
    slabs = min(max((outer + 63) // 64, 1), 128)
    return slabs, (outer + slabs - 1) // slabs
