"""The definition of ``pre.Reverb`` in numpy (its class docstring and include/pds_amd_stages6.h have the text), a float32
restatement of the partitioned form the kernels take, and a float32 error model for the wet signal.

A plain helper (no tests, no fixtures): test_reverb_model.py, test_gpu_reverb.py and test_gpu_command_line_reverb.py
import it.

The plan and the normalisation are exact: integers and float64 operations rounded one by one, so a numpy model has the
device's bits (the segment energy is tests/mix_model.py's).  The wet signal is not: its contract is the model below,
after tests/si_structured.py.

The yardstick is ``np.convolve`` of the samples (float64 samples rounded to float32 first, as the definition loads
them) and the float64 taps, shifted by `d` and cut to the utterance's length.  With ``|h|`` the 2-norm of the float64
taps, ``P = ceil(L / 512)``, and for the output at ``tau = t + d`` in the block beginning at ``b0 = 512 floor(tau / 512)``

    E_tau = sum x[i]^2   over   b0 - 512 (P + 2) <= i < b0 + 1536   (the definition's window of locality)

an element passes if

    |wet - want| <= RTOL |want| + kappa EPS32 |h| sqrt(E_tau)

No element is exempt, and where ``E_tau = 0`` the output must be exactly zero.  ``RTOL = 4 EPS32`` is the rounding of
the stored float32 itself and of the spectra's one rounding to complex64; the strict rule ``atol + rtol |want|`` with
``atol = 0`` is this bound's first term, so it is subsumed and not tested separately.

``kappa_ref(n)`` is measured, never derived from kernel output: the worst kappa restate() needs on the CPU over
calibration_cases(), for utterances of at least one block (``KAPPA_REF_REVERB``) and for shorter ones
(``KAPPA_REF_REVERB_SHORT``) apart.  The GPU tests allow ``structured.MARGIN`` times it (the project's margin, for its
stated reasons: another factorisation of the 32-point transforms, multiply-adds contracted, another order inside a complex product).
"""
import numpy as np

from tests import mix_model
from tests import structured as st
from tests.structured import EPS32, FAMILIES

BLOCK, FFT = 512, 1024
COUNTER = (0, 0, 0, 0x52495231)
RTOL = 4 * EPS32
MARGIN = st.MARGIN
LEVELS = (1e-3, 1.0, 3e4)  # amplitudes (the families' own is 3000)
FAMILY_NAMES = ("tone_bin", "tone_off", "tone_low", "tone_high", "dc", "nyquist", "impulses", "chirp", "step", "noise")
CAL_TAPS = (1, 2, 7, 511, 512, 513, 1024, 1025, 1537, 4000)
CAL_LENGTHS_SHORT = (1, 2, 3, 64, 511)  # utterances shorter than one block of 512 samples
CAL_LENGTHS = (512, 513, 1023, 1025, 2600)

# Worst kappa restate() needs, measured by calibrate() on the CPU (numpy 2.2.6) over calibration_cases(): every L of
# CAL_TAPS (peak in the middle of the taps and at 0), every family of FAMILY_NAMES and a burst, at every level of LEVELS,
# as float32 and as int16-quantised samples.  Two classes of utterance length, calibrated apart so that a handful of
# samples does not set the bound of an ordinary utterance: an utterance shorter than one block (CAL_LENGTHS_SHORT) stands
# with all of its energy against the round-off of whole 1024-point transforms, and needs more.
# test_reverb_model.py::test_calibration recomputes both and fails if either grows.
#   n >= 512: measured 1.2815 at L=2 d=1 n=512 impulses@30000 as int16 (sparse full-scale impulses: a transform's
#             round-off of one impulse stands against the energy of that impulse alone)
#   n <  512: measured 3.6397 at L=2 d=1 n=2 chirp@30000 as float32 (an utterance of two samples)
KAPPA_REF_REVERB = 1.3
KAPPA_REF_REVERB_SHORT = 3.7


def kappa_ref(n):
    """the calibrated kappa of an utterance of n samples"""
    return KAPPA_REF_REVERB_SHORT if n < BLOCK else KAPPA_REF_REVERB


# ---- the plan -------------------------------------------------------------------------------------------------------


def draws(key, counter=COUNTER):
    """x0..x3 of the plan's Philox block under `key` (Python integers)"""
    return mix_model.philox4x32_10(counter, int(key))


def draw(x, K, prob):
    """(rir, applied) of the output words `x`"""
    return (int(x[0]) * int(K)) >> 32, bool(np.float64(x[3]) * np.float64(2.0 ** -32) < prob)


def plan(keys, K, prob):
    rows = [draw(draws(key), K, prob) for key in keys]
    return (np.asarray([r[0] for r in rows], dtype=np.int64), np.asarray([r[1] for r in rows], dtype=bool))


def peak(taps, shift_output=True):
    """the first index of max |h[k]|, the taps compared as float64; 0 without the shift"""
    if not shift_output:
        return 0
    a = np.abs(np.asarray(taps).astype(np.float64))
    best = 0
    for k in range(len(a)):
        if a[k] > a[best]:
            best = k
    return best


# ---- the yardstick --------------------------------------------------------------------------------------------------


def load32(x):
    """the samples as the kernels load them: float64 rounded to float32, int16 widened"""
    return np.asarray(x).astype(np.float32)


def wet_exact(x, taps, d):
    """float64: y_full[t + d] for 0 <= t < n, from the samples as loaded and the float64 taps"""
    x64 = load32(x).astype(np.float64)
    n = len(x64)
    if n == 0:
        return np.zeros(0)
    full = np.convolve(x64, np.asarray(taps).astype(np.float64))
    out = np.zeros(n)
    seg = full[d : d + n]
    out[: len(seg)] = seg
    return out


def partitions(L):
    return -(-int(L) // BLOCK)


def window_of(t, d, P):
    """[lo, hi) of the input samples the output t may depend on (not clipped to the utterance)"""
    b0 = BLOCK * ((t + d) // BLOCK)
    return b0 - BLOCK * (P + 2), b0 + 3 * BLOCK


def window_energy(x, d, P):
    """E_tau of every output 0 <= t < n (float64)"""
    x64 = load32(x).astype(np.float64)
    n = len(x64)
    cs = np.concatenate([[0.0], np.cumsum(x64 * x64)])
    t = np.arange(n)
    b0 = BLOCK * ((t + d) // BLOCK)
    lo = np.clip(b0 - BLOCK * (P + 2), 0, n)
    hi = np.clip(b0 + 3 * BLOCK, 0, n)
    E = cs[hi] - cs[lo]
    # (a difference of running sums may leave dust where the window is silent: ask the samples)
    nz = np.concatenate([[0], np.cumsum(x64 != 0)])
    return np.where(nz[hi] - nz[lo] > 0, np.maximum(E, np.finfo(np.float64).tiny), 0.0)


# ---- the float32 restatement ----------------------------------------------------------------------------------------

_TABLES = {}


def _tables():
    if not _TABLES:
        k = np.arange(32)
        _TABLES["dft32"] = np.exp(-2j * np.pi * np.outer(k, k) / 32).astype(np.complex64)
        _TABLES["tw1024"] = np.exp(-2j * np.pi * np.outer(k, k) / 1024).astype(np.complex64)  # [k1, l], float32 twiddles
    return _TABLES


def fft1024(z):
    """1024-point DFT along the last axis as csrc/reverb.hip factors it: element 32 q + l; a DFT-32 over q, the
    float32-rounded table W_1024^(l k1), a DFT-32 over l; bin k1 + 32 k2.  complex64 throughout."""
    T = _tables()
    a = z.reshape(z.shape[:-1] + (32, 32))
    a = np.einsum("qk,...ql->...kl", T["dft32"], a, optimize=False)
    a = (a * T["tw1024"]).astype(np.complex64)
    a = np.matmul(a, T["dft32"])
    assert a.dtype == np.complex64, a.dtype
    return np.swapaxes(a, -1, -2).reshape(z.shape)


def partition_spectra(taps):
    """complex64 [P, 1024]: float64 transforms of the partitions of 512 taps, rounded once"""
    taps = np.asarray(taps).astype(np.float64)
    P = partitions(len(taps))
    padded = np.zeros(P * BLOCK)
    padded[: len(taps)] = taps
    return np.fft.fft(padded.reshape(P, BLOCK), n=FFT, axis=1).astype(np.complex64)


def utterance_spectra(x32):
    """{k: complex64 [1024]} for k = -1 .. floor((n - 1) / 512) + 1: block k's stretch in the real part, block k + 1's
    in the imaginary part"""
    n = len(x32)
    last = (n - 1) // BLOCK + 1
    pad = np.zeros((last + 4) * BLOCK, dtype=np.float32)  # sample i at pad[i + 1024]
    pad[2 * BLOCK : 2 * BLOCK + n] = x32
    z = np.stack([pad[(k + 1) * BLOCK : (k + 3) * BLOCK] + 1j * pad[(k + 2) * BLOCK : (k + 4) * BLOCK]
                  for k in range(-1, last + 1)]).astype(np.complex64)
    Z = fft1024(z)
    return {k: Z[k + 1] for k in range(-1, last + 1)}


def restate(x, taps, d, H=None):
    """float32 wet signal by exactly the partitioned form of the kernels: the same pairing of blocks, the same order
    over p, twiddles rounded to float32, complex64 sums"""
    x32 = load32(x)
    n = len(x32)
    out = np.zeros(n, dtype=np.float32)
    if n == 0:
        return out
    t64 = np.asarray(taps).astype(np.float64)
    if np.count_nonzero(t64) == 1:  # one tap: a delay and a gain, one float32 product, no transform
        k0 = int(np.flatnonzero(t64)[0])
        i = np.arange(n) + d - k0
        inside = (i >= 0) & (i < n)
        with np.errstate(all="ignore"):
            out[inside] = np.float32(t64[k0]) * x32[i[inside]]
        return out
    H = partition_spectra(taps) if H is None else H
    P = len(H)
    Z = utterance_spectra(x32)
    last = (n - 1) // BLOCK + 1
    with np.errstate(all="ignore"):
        for m in range(d // FFT, (d + n - 1) // FFT + 1):
            k = 2 * m
            acc = np.zeros(FFT, dtype=np.complex64)
            for p in range(max(0, k - last), min(P - 1, k + 1) + 1):
                acc = acc + Z[k - p] * H[p]
            assert acc.dtype == np.complex64
            y = np.conj(fft1024(np.conj(acc)))[BLOCK:] * np.float32(2.0 ** -10)
            for part, kk in ((y.real, k), (y.imag, k + 1)):
                lo, hi = max(0, kk * BLOCK - d), min(n, kk * BLOCK + BLOCK - d)
                if hi > lo:
                    out[lo:hi] = part[lo - (kk * BLOCK - d) : hi - (kk * BLOCK - d)]
    return out


# ---- the normalisation ----------------------------------------------------------------------------------------------


def normalise(x, wet):
    """(Ps, Py, c, out) of one utterance `x` in its own dtype and its float32 wet signal; c is 0.0 for "leave" """
    wet = np.asarray(wet)
    assert wet.dtype == np.float32
    ps, py = mix_model.power(x), mix_model.power(wet)
    if not (ps > 0.0 and py > 0.0):  # (false for NaN)
        return ps, py, np.float64(0.0), wet.copy()
    with np.errstate(all="ignore"):
        c = np.sqrt(np.float64(ps) / np.float64(py))
        return ps, py, c, (wet.astype(np.float64) * c).astype(np.float32)


def copied(x):
    """an utterance that is not applied: float32 byte for byte, int16 widened, float64 rounded once"""
    x = np.asarray(x)
    with np.errstate(all="ignore"):
        return x.copy() if x.dtype == np.float32 else x.astype(np.float32)


# ---- the error model ------------------------------------------------------------------------------------------------


def kappa_needed(got, x, taps, d):
    """(kappa per element, exact-zero failures): the smallest kappa for which each element passes; inf where a silent
    window did not give an exact zero or the value is not finite"""
    taps64 = np.asarray(taps).astype(np.float64)
    want = wet_exact(x, taps64, d)
    E = window_energy(x, d, partitions(len(taps64)))
    h = np.sqrt(np.sum(taps64 * taps64))
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(all="ignore"):
        excess = np.maximum(np.abs(got - want) - RTOL * np.abs(want), 0.0)
        k = excess / np.maximum(EPS32 * h * np.sqrt(E), np.finfo(np.float64).tiny)
    k = np.where(E > 0, k, np.where(got == 0.0, 0.0, np.inf))
    return np.where(np.isnan(k), np.inf, k)


def check(got, x, taps, d, kappa):
    """(ok, worst kappa, message)"""
    if len(got) != len(x):
        return False, np.inf, f"length {len(got)} vs {len(x)}"
    if not len(x):
        return True, 0.0, ""
    k = kappa_needed(got, x, taps, d)
    t = int(np.argmax(k))
    worst = float(k[t])
    ok = worst <= kappa
    msg = "" if ok else (f"sample {t}: got {np.asarray(got)[t]!r} want {wet_exact(x, taps, d)[t]!r}, needs kappa "
                         f"{worst:.3g} > {kappa:.3g} ({int((k > kappa).sum())} of {len(k)} elements fail)")
    return ok, worst, msg


# ---- signals, responses, calibration --------------------------------------------------------------------------------


def burst(n, N, rng):
    x = np.zeros(n)
    a, b = n // 3, min(n, n // 3 + 200)
    x[a:b] = 3000 * rng.standard_normal(b - a)
    return x


def signals(n, seed=2024, grid=1024):
    """[(label, float64 samples)]: every family and the burst at every level"""
    rng = np.random.default_rng(seed)
    fams = [(name, FAMILIES[name]) for name in FAMILY_NAMES] + [("burst", burst)]
    return [(f"{name}@{a:g}", (a / 3000.0) * np.asarray(f(n, grid, rng), dtype=np.float64)) for name, f in fams
            for a in LEVELS]


def response(L, d, seed=5, dtype=np.float64):
    """a decaying noise response of L taps whose largest tap is at d (a unit tap on top of the tail)"""
    rng = np.random.default_rng(seed + 1000 * L + d)
    h = np.clip(0.3 * rng.standard_normal(L), -0.9, 0.9) * np.exp(-3.0 * np.arange(L) / max(L, 1))
    h[d] = 1.0 if h[d] >= 0 else -1.0
    if np.dtype(dtype) == np.int16:
        return np.clip(np.rint(h * 16384), -32768, 32767).astype(np.int16)
    return h.astype(dtype)


def calibration_cases():
    for L in CAL_TAPS:
        for d in sorted({0, L // 2}):
            yield L, d, response(L, d)


def calibrate():
    """{"short": (worst kappa, its case), "long": ...} of restate() over calibration_cases() x signals(), float32 and
    int16-quantised, for the two classes of utterance length"""
    worst = {"short": (0.0, None), "long": (0.0, None)}
    for L, d, h in calibration_cases():
        H = partition_spectra(h)
        for which, lengths in (("short", CAL_LENGTHS_SHORT), ("long", CAL_LENGTHS)):
            for n in lengths:
                assert (n < BLOCK) == (which == "short")
                for label, x in signals(n):
                    for kind, xs in (("f32", x.astype(np.float32)), ("i16", st.quantise_i16(x))):
                        k = kappa_needed(restate(xs, h, d, H), xs, h, d)
                        assert np.isfinite(k).all(), (L, d, n, label, kind)
                        if k.max() > worst[which][0]:
                            worst[which] = (float(k.max()), f"L={L} d={d} n={n} {label}/{kind}")
    return worst
