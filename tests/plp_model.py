"""The definition of ``post.PLP`` in numpy (its class docstring and include/pds_amd_stages4.h have the text): the
reference every PLP test compares with.  Every float64 operation is a numpy ufunc call of its own and so rounded once;
the rows of a matrix go through the recursions side by side.  ``pow`` and ``log`` are numpy's here and the device's
there: :func:`plp_from_spectrum` takes the compressed spectrum ``d`` as given, so that everything behind the ``pow``
can be compared bit for bit."""
import math

import numpy as np

from pydrobert_speech_amd.post import PLP


def plp_tables(post: PLP, width: int):
    """``(w[F], B[p + 1, D], L[K])`` of the definition for rows of `width` columns, float64, written from the text"""
    F = int(width) - int(post.energy)
    D, p, K = F + 2, post.lpc_order, post.num_ceps
    w = np.ones(F, dtype=np.float64)
    if post.equal_loudness:
        for f, c in enumerate(post.centers_hz):
            fsq = np.float64(c) * np.float64(c)
            fs = fsq / (fsq + np.float64(1.6e5))
            w[f] = fs * fs * ((fsq + np.float64(1.44e6)) / (fsq + np.float64(9.61e6)))
    # (Python floats are float64, and math.cos / math.sin are the C library's, one call an element)
    s = 1.0 / (2.0 * (D - 1))
    theta = math.pi / (D - 1)
    B = np.empty((p + 1, D), dtype=np.float64)
    for i in range(p + 1):
        B[i, 0] = s
        for j in range(1, D - 1):
            B[i, j] = 2.0 * s * math.cos(theta * float(i) * float(j))
        B[i, D - 1] = s * math.cos(theta * float(i) * float(D - 1))
    L = np.empty(K, dtype=np.float64)
    for k in range(K):
        Q = float(post.lifter)
        L[k] = post.scale * (1.0 + 0.5 * Q * math.sin(math.pi * float(k) / Q)) if post.lifter else post.scale
    return w, B, L


def plp_from_autocorrelation(r, p: int):
    """Steps 6 and 7 of the definition for rows of autocorrelations `r`, ``(R, p + 1)`` float64 -> ``(a, q, E)``"""
    r = np.asarray(r, dtype=np.float64)
    R = r.shape[0]
    a = np.zeros((R, p), dtype=np.float64)
    q = np.zeros((R, p), dtype=np.float64)
    with np.errstate(all="ignore"):
        E = r[:, 0].copy()
        for i in range(p):
            k = r[:, i + 1].copy()
            for j in range(i):
                k = k + a[:, j] * r[:, i - j]
            k = k / E
            c = np.float64(1.0) - k * k
            c = np.where(c < 1e-5, np.float64(1e-5), c)  # (a NaN passes)
            E = E * c
            t = np.empty((R, i + 1), dtype=np.float64)
            t[:, i] = -k
            for j in range(i):
                t[:, j] = a[:, j] - k * a[:, i - j - 1]
            a[:, : i + 1] = t
        for i in range(p):
            s = np.zeros(R, dtype=np.float64)
            for j in range(i):
                s = s + (np.float64(i - j) * a[:, j]) * q[:, i - j - 1]
            q[:, i] = -a[:, i] - s / np.float64(i + 1)
    return a, q, E


def plp_from_spectrum(d, B):
    """Steps 5 to 7 for rows of compressed spectra `d`, ``(R, D)`` float64, and the table `B`, ``(p + 1, D)`` ->
    ``(q, E)``: the cepstra ``(R, p)`` and the final prediction error ``(R,)``"""
    d = np.asarray(d, dtype=np.float64)
    p, D = B.shape[0] - 1, B.shape[1]
    r = np.zeros((d.shape[0], p + 1), dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in range(D):
            r = r + B[None, :, j] * d[:, j : j + 1]
    _, q, E = plp_from_autocorrelation(r, p)
    return q, E


def plp_spectrum(post: PLP, x, w):
    """Steps 1 to 4: ``d``, ``(R, D)`` float64, of rows `x`, ``(R, W)``, with numpy's ``pow``"""
    copy = int(post.energy)
    e = np.asarray(x)[:, copy:].astype(np.float64)
    with np.errstate(all="ignore"):
        g = np.where(e < post.floor, np.float64(post.floor), e)
        h = np.power(g * w[None, :], np.float64(post.compress_factor))
    return np.concatenate([h[:, :1], h, h[:, -1:]], axis=1)


def plp_output(post: PLP, x, q, E, L):
    """Step 8 from `q` and `E` (numpy's ``log``), rounded once to the dtype of the rows `x`"""
    x = np.asarray(x)
    dtype = x.dtype if x.dtype in (np.float32, np.float64) else np.dtype(np.float64)
    K = post.num_ceps
    out = np.empty((x.shape[0], K), dtype=np.float64)
    with np.errstate(all="ignore"):
        if post.energy:
            e0 = x[:, 0].astype(np.float64)
            out[:, 0] = np.log(np.where(e0 < post.floor, np.float64(post.floor), e0))
        else:
            out[:, 0] = L[0] * np.log(E)
        out[:, 1:] = L[None, 1:] * q[:, : K - 1]
    return out.astype(dtype)


def plp_model(post: PLP, x):
    """All steps for rows `x`, ``(R, W)``: the ``(R, K)`` output of x's dtype (float64 for anything but float32)"""
    x = np.asarray(x)
    w, B, L = plp_tables(post, x.shape[1])
    q, E = plp_from_spectrum(plp_spectrum(post, x, w), B)
    return plp_output(post, x, q, E, L)


def energies(rng, shape, dtype, sigma=2.0, zeros=0.02):
    """the tests' inputs: ``exp(N(0, sigma))`` scaled per row by one of 1e-8, 1, 1e6, with a few exact zeros"""
    x = np.exp(sigma * rng.standard_normal(shape))
    x *= rng.choice([1e-8, 1.0, 1e6], size=shape[:-1] + (1,))
    x[rng.random(shape) < zeros] = 0.0
    return x.astype(dtype)


def same_bits(a, b) -> bool:
    """equal shape and dtype, NaNs at the same positions and every other element equal bit for bit"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not (na == nb).all():
        return False
    ints = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool((a.view(ints)[~na] == b.view(ints)[~nb]).all())


def tolerance_ratio(got, ref) -> float:
    """the worst ``|got - ref| / (atol + rtol |ref|)`` over the finite elements under the standing rule of
    :func:`within_tolerance` (a figure to print; below 1 is within)"""
    got, ref = np.asarray(got), np.asarray(ref)
    fin = np.isfinite(ref) & np.isfinite(got)
    if not fin.any():
        return 0.0
    atol, rtol = (1e-5, 1e-4) if ref.dtype == np.float32 else (1e-9, 1e-9)
    g, r = got[fin].astype(np.float64), ref[fin].astype(np.float64)
    return float((np.abs(g - r) / (atol + rtol * np.abs(r))).max())


def within_tolerance(got, ref) -> bool:
    """the package's standing rule for values that go through a device function: ``1e-5 + 1e-4 |ref|`` for float32
    rows, ``rtol = atol = 1e-9`` for float64 rows; NaNs and infinities at the same positions (and the same infinities),
    no element exempted"""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.dtype != ref.dtype or got.shape != ref.shape:
        return False
    if not (np.isnan(got) == np.isnan(ref)).all():
        return False
    fin = np.isfinite(ref)
    if not (got[~fin & ~np.isnan(ref)] == ref[~fin & ~np.isnan(ref)]).all():
        return False
    g, r = got[fin].astype(np.float64), ref[fin].astype(np.float64)
    if not np.isfinite(g).all():
        return False
    atol, rtol = (1e-5, 1e-4) if ref.dtype == np.float32 else (1e-9, 1e-9)
    return bool((np.abs(g - r) <= atol + rtol * np.abs(r)).all())
