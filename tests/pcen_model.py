"""The definition of ``post.PCEN`` in numpy (its class docstring and include/pds_amd_stages2.h have the text): the
reference every PCEN test compares with.  ``M`` is a plain loop over the frames of float64 operations, each a numpy
ufunc call of its own and so rounded once; ``y`` is float64, rounded once to the row type.  ``oms`` and ``bp`` are the
object's, as the kernels are given them."""
import numpy as np

from pydrobert_speech_amd.post import PCEN


def smooth_model(post: PCEN, E) -> np.ndarray:
    """M of one utterance: `E` is ``(T, ...)``, time first; float64 of E's shape"""
    x = np.asarray(E).astype(np.float64)  # (widened exactly)
    oms, s = np.float64(post.oms), np.float64(post.smooth_coeff)
    M = np.empty_like(x)
    with np.errstate(all="ignore"):
        for t in range(len(x)):
            if t == 0:
                M[0] = x[0]
            else:
                kept = oms * M[t - 1]
                fresh = s * x[t]
                M[t] = kept + fresh
    return M


def compress_model(post: PCEN, E, M) -> np.ndarray:
    """y of the definition from E and M, of E's dtype (float32 or float64; anything else gives float64)"""
    E = np.asarray(E)
    out = E.dtype if E.dtype in (np.float32, np.float64) else np.dtype(np.float64)
    x = E.astype(np.float64)
    with np.errstate(all="ignore"):
        agc = np.power(np.float64(post.eps) + M, np.float64(post.gain))
        y = np.power(x / agc + np.float64(post.bias), np.float64(post.power)) - np.float64(post.bp)
        return y.astype(out)


def pcen_model(post: PCEN, E):
    """``(y, M)`` of one utterance `E`, ``(T, ...)`` with time first"""
    M = smooth_model(post, E)
    return compress_model(post, E, M), M


def energies(rng, shape, dtype, zeros=0.05):
    """the tests' inputs: ``exp`` of normals scaled so that three standard deviations span 1e-6 .. 1e6, with exact
    zeros mixed in"""
    x = np.exp(rng.standard_normal(shape) * (np.log(1e6) / 3.0))
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
