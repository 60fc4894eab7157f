"""Structured test signals, float32 restatements of the oracle and a float32 error model for short-integration parity.

Why.  Every other SI parity test feeds Gaussian noise and compares with ``test_gpu_si.close``, which forgives whatever
lies below ``1e-3 max|want|``.  On noise a filter spectrum delayed by 1e-3 sample passes that check with no element
outside it; on tones, impulses and chirps a *correct* float32 overlap-save pipeline fails it (up to a fifth of the
elements of a log-magnitude bank): the filters' stop bands carry the transform's round-off at full size.  So a parity
test on such signals has to know what float32 can deliver.  tests/structured.py does this for the STFT computer; this
module is its SI counterpart and reuses its signal families.

The model.  ``S`` the frame shift, ``M`` the longest support, ``start = skip - lead`` (``so.stream_start``),
``w[t, f]`` the float64 oracle's linear coefficient (no log), ``|h_f|`` the 2-norm of filter f's taps (the energy row
is a unit impulse: 1), ``W1 = sum(window)`` and

    E_t = sum x[j]^2   over the signal samples  t S + start - (M - 1) - R  <=  j  <  t S + start + 2 S + R

with ``R = 2048``, the largest transform: a transform's stretch reaches at most ``NT - S`` before a frame's first
integrated sample and ``V - S`` past its last.  With every filtered sample off by at most ``kappa eps |h_f| sqrt(E_t)``
Cauchy-Schwarz gives

    power       |got - w| <= rtol w + 2 kappa eps sqrt(w W1 |h_f|^2 E_t) + kappa^2 eps^2 W1 |h_f|^2 E_t
    magnitude   |got - w| <= rtol w + kappa eps W1 |h_f| sqrt(E_t)

Log features are compared as ``exp(got)`` against ``max(w, 1e-5)`` (the clamp is 1-Lipschitz).  An element passes if
the strict rule ``|got - want| <= atol + rtol |want|`` holds (2e-5 / 2e-4 for float32: the suite's SI tolerance
without ``close()``'s scale forgiveness; 1e-9 / 1e-9 for float64) OR the bound holds.  No element is exempt; frames
with ``E_t = 0`` get the strict rule only.

``kappa`` is measured, not chosen: ``KAPPA_REF_FFT`` is the worst kappa the two float32 overlap-save restatements
below need on the CPU over every (configuration, family, level) case of the suite, ``KAPPA_REF_DIRECT`` the same for
the direct form.  The GPU tests allow ``structured.MARGIN`` times that.

A plain helper (no tests, no fixtures): test_si_structured_model.py and test_gpu_si_structured.py import it.
"""
import json
from dataclasses import replace

import numpy as np

from oracle import si_oracle as so
from tests import test_gpu_si as _tgs  # (the suite's own lists of banks: imported, not copied)
from tests import test_gpu_si_shapes as _tgss
from tests import structured as st
from tests.structured import EPS32, EPS64, FAMILIES, LEVELS, Result, quantise_i16, strict_ok

R = 2048  # the largest transform
GRID_N = 1024  # frequency grid of the signal families
F32 = dict(eps=EPS32, rtol=2e-4, atol=2e-5)
F64 = dict(eps=EPS64, rtol=1e-9, atol=1e-9)

# Worst kappa the float32 restatements below need, measured by calibrate() on the CPU (numpy 2.2.6, whose FFT of
# complex64 stays complex64) over suite_names() and every family and level of cases(), as float32 samples and as
# int16-quantised ones, on the linear coefficients.  test_si_structured_model.py::test_calibration recomputes both and
# fails if either grows.  Never derived from what a kernel produces.
#   FFT form: 0.2332 (tone_low as int16, gabor41_1024) with the kernel's 32 x 32 factorisation and float32 twiddle
#   tables (0.164 tone_high nw_gammatone40_48k_2.5ms_2048, 0.104 impulses nw_gabor5_8k_5ms_1024); numpy's own complex64
#   FFT needs 0.0394 (impulses, s3_tri_energy_nolog), 0.036 impulses nw_gabor5_8k_5ms_1024, 0.032 chirp gabor41_1024.
#   Direct form: 0.0411 (dc, gabor41_1024); 0.037 step s4_gabor_8k_short, 0.031 tone_high s3_tri_energy_nolog.
KAPPA_REF_FFT = 0.24
KAPPA_REF_DIRECT = 0.042
MARGIN = st.MARGIN  # the STFT suite's, for its reasons: another factorisation, another summation order, v_sqrt_f32
MARGIN_F64 = st.MARGIN_F64  # float64 arithmetic: the oracle's own rounding is as large as the kernel's

FIXTURE_CONFIGS = sorted(_tgs.META["configs"])
BUCKETS = list(_tgs.test_fft_form_window_factor_buckets_against_oracle.pytestmark[0].args[1])


def bucket_name(rate, shift_ms, bank, num_filts, use_power, size):
    return f"nw_{bank}{num_filts}_{rate // 1000}k_{shift_ms:g}ms_{size}"


BUCKET_CONFIGS = {bucket_name(*b): b for b in BUCKETS}
DIRECT_ONLY = "fbank_direct_only"


# ------------------------------------------------------------------------------------- launch shapes (host) ----

MAX_BLOCKS, MAX_WINDOW_REGS, HALF_LANES = 8, 16, 32  # kSiFftMaxBlocks, kSiFftMaxWindowRegs, kSiFftL of csrc/si_shape.h


def si_fft_blocks_for(NT, M, S):
    """csrc/si_shape.h: blocks of S filtered samples one NT-point transform yields for supports of M taps (0: none)"""
    if M > NT:
        return 0
    blocks = min(MAX_BLOCKS, (NT - (M - 1)) // S)
    lanes = NT // HALF_LANES
    return 0 if blocks < 1 or S > MAX_WINDOW_REGS * lanes else blocks


def si_fft_form_for(M, S):
    """csrc/si_shape.h: (NT, blocks) of the overlap-save form that serves supports of M taps at shift S; (0, 0): none"""
    b1, b2 = si_fft_blocks_for(1024, M, S), si_fft_blocks_for(2048, M, S)
    if b1 == 0 and b2 == 0:
        return 0, 0
    eff1, eff2 = b1 * S / 1024, b2 * S / 2048 / 1.2
    return (2048, b2) if eff2 > eff1 else (1024, b1)


def window_factors(NT, S):
    """csrc/si_shape.h: window factors a lane keeps per half (the built counts 3, 5, 8, 16)"""
    nw = -(-S // (NT // HALF_LANES))
    return 3 if nw <= 3 else 5 if nw <= 5 else 8 if nw <= 8 else MAX_WINDOW_REGS


# ------------------------------------------------------------------------------------------ configurations ----


def _build(cfg):
    from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg
    from pydrobert_speech_amd.compute import FrameComputer

    return alias_factory_subclass_from_arg(FrameComputer, json.loads(json.dumps(cfg)))


def direct_only_filters():
    """The fewest fbank filters (16 kHz, 10 ms) whose supports are beyond both transform sizes"""
    for nf in range(3, 41):
        comp = _build({"name": "si", "bank": {"name": "fbank", "num_filts": nf}})
        if si_fft_form_for(comp._max_support, comp.frame_shift) == (0, 0):
            assert si_fft_form_for(_build({"name": "si", "bank": {"name": "fbank", "num_filts": nf - 1}})._max_support,
                                   comp.frame_shift) != (0, 0)
            return nf
    raise AssertionError("no direct-only fbank bank of up to 40 filters")


def suite_names():
    """The six fixture configurations, the eight window-factor-bucket banks of test_gpu_si.py, the 41-coefficient
    energy bank of test_gpu_si_shapes.py and one bank only the direct form serves"""
    return FIXTURE_CONFIGS + list(BUCKET_CONFIGS) + ["gabor41_1024", DIRECT_ONLY]


def build(name):
    """A fresh computer of one name of suite_names() (host tables only until a kernel is asked for)"""
    if name in FIXTURE_CONFIGS:
        return _tgs.build(name)
    if name in BUCKET_CONFIGS:
        rate, shift_ms, bank, num_filts, use_power, _ = BUCKET_CONFIGS[name]
        # (as test_fft_form_window_factor_buckets_against_oracle builds it: power banks take logs, magnitude ones raw sums)
        return _build({"name": "si", "bank": {"name": bank, "scaling_function": "mel", "num_filts": num_filts,
                                              "sampling_rate": rate},
                       "frame_shift_ms": shift_ms, "use_power": use_power, "use_log": use_power})
    if name == "gabor41_1024":
        return _tgss.si_computer(**_tgss.FFT_BANKS[name][0])
    assert name == DIRECT_ONLY, name
    return _build({"name": "si", "bank": {"name": "fbank", "num_filts": direct_only_filters()}, "use_power": True})


def params_from_computer(comp):
    return so.SiParams(comp.frame_shift, comp._max_support, comp._translation, comp.dft_size, comp.taps,
                       comp._window.reshape(-1), comp.frame_style == "centered", bool(comp._power), bool(comp._log))


_SUITE = {}


def suite_config(name):
    """(SiParams, (NT, blocks) of the FFT form or (0, 0)) of one name of suite_names(), built on first use"""
    if name not in _SUITE:
        p = params_from_computer(build(name))
        _SUITE[name] = (p, si_fft_form_for(p.max_support, p.frame_shift))
    return _SUITE[name]


# ------------------------------------------------------------------------------------------------ signals ----


def start_of(p):
    skip, lead = so.stream_start(p)
    return skip - lead


def utterance_length(p):
    return 14 * p.frame_shift + min(p.max_support, 3000)


def linear_params(p):
    return replace(p, use_log=False)


def floor_share(x, p):
    y = so.compute_full(np.asarray(x, np.float64), p)
    return float((y == np.log(so.LOG_FLOOR)).mean()) if y.size else 0.0


_GAINS = {}


def straddle_gain(p, seed=7):
    """structured.straddle_gain against the SI oracle: the gain of a fixed grid (eight per decade) at which white noise
    puts the share of coefficients nearest to one half exactly on log(floor); None for banks that take no log"""
    if not p.use_log:
        return None
    if id(p) not in _GAINS:
        unit = np.random.default_rng(seed).standard_normal(utterance_length(p))
        gains = 10.0 ** (np.arange(-48, 9) / 8.0)
        shares = np.array([floor_share(g * unit, p) for g in gains])
        _GAINS[id(p)] = (p, float(gains[int(np.argmin(np.abs(shares - 0.5)))]))
    return _GAINS[id(p)][1]


def cases(p, seed=2024):
    """[(label, float64 samples)]: every family of tests/structured.py on a 1024-point frequency grid, noise and the
    off-bin tone at LEVELS, and (log banks) noise at the straddle gain"""
    rng = np.random.default_rng(seed)
    n = utterance_length(p)
    out = [(name, np.asarray(f(n, GRID_N, rng), np.float64)) for name, f in FAMILIES.items()]
    for a in LEVELS:
        out.append((f"noise@{a:g}", (a / 3000) * FAMILIES["noise"](n, GRID_N, rng)))
        out.append((f"tone_off@{a:g}", (a / 3000) * FAMILIES["tone_off"](n, GRID_N, rng)))
    gain = straddle_gain(p)
    if gain is not None:
        out.append(("noise@straddle", gain * np.random.default_rng(7).standard_normal(n)))
    return out


# ------------------------------------------------------------------------------- float32 restatements ----


def _stretch(x, a, count):
    """x[a : a + count] with zeros outside the signal"""
    seg = np.zeros(count, x.dtype)
    s0, s1 = max(a, 0), min(a + count, len(x))
    if s1 > s0:
        seg[s0 - a : s1 - a] = x[s0:s1]
    return seg


def _finish32(out, p):
    assert out.dtype == np.float32, out.dtype
    if p.use_log:
        out = np.log(np.maximum(out, np.float32(so.LOG_FLOOR)))
    return out


def filter_spectra(p, NT, mutate=None):
    """[C, NT] complex64: the taps' NT-point DFT formed in float64, 1 / NT folded in, rounded to float32 (as the plan
    builds them).  `mutate` maps the float64 spectra to perturbed ones."""
    H = np.fft.fft(np.asarray(p.taps, np.complex128), n=NT, axis=1) / NT
    if mutate is not None:
        H = mutate(H)
    return H.astype(np.complex64)


def fft_numpy(z):
    out = np.fft.fft(z, axis=-1)
    assert out.dtype == np.complex64, out.dtype
    return out


_TABLES = {}


def _tables():
    if not _TABLES:
        k = np.arange(32)
        _TABLES["dft32"] = np.exp(-2j * np.pi * np.outer(k, k) / 32).astype(np.complex64)  # [q, k1] and [l, k2]
        _TABLES["tw1024"] = np.exp(-2j * np.pi * np.outer(k, k) / 1024).astype(np.complex64)  # [k1, l]
        _TABLES["tw2048"] = np.exp(-2j * np.pi * np.arange(1024) / 2048).astype(np.complex64)
    return _TABLES


def _fft1024_tables(z):
    """1024-point DFT along the last axis as csrc/si_fft.hip factors it: element 32 q + l; a DFT-32 over q, the
    float32-rounded table W_1024^(l k1), a DFT-32 over l; bin k1 + 32 k2.  complex64 throughout."""
    T = _tables()
    a = z.reshape(z.shape[:-1] + (32, 32))  # [q, l]
    a = np.einsum("qk,...ql->...kl", T["dft32"], a, optimize=False)  # [k1, l]
    a = (a * T["tw1024"]).astype(np.complex64)
    a = np.matmul(a, T["dft32"])  # [k1, k2]
    assert a.dtype == np.complex64, a.dtype
    return np.swapaxes(a, -1, -2).reshape(z.shape)  # k = k1 + 32 k2


def fft_tables(z):
    """The forward transform of the kernel: 1024 points, or radix 2 in time on top of it (X = E +- W^j O)"""
    if z.shape[-1] == 1024:
        return _fft1024_tables(z)
    assert z.shape[-1] == 2048
    w = _tables()["tw2048"]
    e, o = _fft1024_tables(np.ascontiguousarray(z[..., 0::2])), _fft1024_tables(np.ascontiguousarray(z[..., 1::2]))
    o = (o * w).astype(np.complex64)
    return np.concatenate([e + o, e - o], axis=-1)


def ifft_tables_conj(z):
    """conj of the unnormalised inverse transform, as the kernel forms it: the forward routine on conj(Z); 2048 points:
    radix 2 in frequency (sum / twiddled difference of the halves, then a 1024-point transform of each)"""
    z = np.conj(z)
    if z.shape[-1] == 1024:
        return _fft1024_tables(z)
    w = _tables()["tw2048"]
    lo, hi = z[..., :1024], z[..., 1024:]
    out = np.empty_like(z)
    out[..., 0::2] = _fft1024_tables(lo + hi)
    out[..., 1::2] = _fft1024_tables(((lo - hi) * w).astype(np.complex64))
    return out


MUTATIONS = ("first_valid", "halves_swapped", "last_block_scaled", "magnitude_for_power", "window_past_block")


def restate_fft(x, p, form, tables=False, mutate_spectra=None, mutation=None, num_frames=None, first_frame=0):
    """The oracle as float32 overlap-save with the plan's `form` = (NT, blocks): float32 filter spectra, complex64
    transforms (numpy's, or with `tables` the kernel's 32 x 32 factorisation with float32 twiddle tables), per block
    two float32 sums weighted by the window's halves, frame t = first-half(t) + second-half(t + 1).

    `mutate_spectra` / `mutation` (one of MUTATIONS) make it wrong the way a defective kernel would be."""
    assert mutation is None or mutation in MUTATIONS, mutation
    NT, blocks = form
    x = np.asarray(x, np.float32)
    S, C = p.frame_shift, p.taps.shape[0]
    T = so.frame_count(len(x), p) if num_frames is None else num_frames
    if not T:
        return np.zeros((0, C), np.float32)
    V = blocks * S
    start = start_of(p) + first_frame * S
    D = -(-(T + 1) // blocks)
    stretches = np.stack([_stretch(x, d * V + start - (NT - V), NT) for d in range(D)]).astype(np.complex64)
    H = filter_spectra(p, NT, mutate_spectra)
    fwd = fft_tables if tables else fft_numpy
    inv = ifft_tables_conj if tables else (lambda z: fft_numpy(np.conj(z)))
    X = fwd(stretches)
    wa, wb = p.window[:S].astype(np.float32), p.window[S:].astype(np.float32)
    if mutation == "halves_swapped":
        wa, wb = wb, wa
    first_valid = NT - V - (1 if mutation == "first_valid" else 0)
    A, B = np.empty((D * blocks, C), np.float32), np.empty((D * blocks, C), np.float32)
    for c in range(C):
        y = inv((X * H[c]).astype(np.complex64))  # (conjugated: it does not matter to |y|)
        z = y.real * y.real + y.imag * y.imag
        if not p.use_power or mutation == "magnitude_for_power":
            z = np.sqrt(z)
        assert z.dtype == np.float32, z.dtype
        zb = z[:, first_valid : first_valid + V].reshape(D * blocks, S)
        A[:, c], B[:, c] = zb @ wa, zb @ wb
        if mutation == "window_past_block":  # the sample behind a block's end, weighted as the block's last one
            past = np.zeros((D, blocks), np.float32)
            past[:, :-1] = z[:, first_valid + S : first_valid + V : S]
            A[:, c] += wa[S - 1] * past.reshape(-1)
            B[:, c] += wb[S - 1] * past.reshape(-1)
    if mutation == "last_block_scaled":
        A[blocks - 1 :: blocks] *= np.float32(1.001)
        B[blocks - 1 :: blocks] *= np.float32(1.001)
    return _finish32(A[:T] + B[1 : T + 1], p)


def restate_direct(x, p, num_frames=None, first_frame=0):
    """The oracle's closed form in float32: y[i] accumulated tap by tap (an explicit loop over k < M, vectorised over
    the samples and the filters), then the window-weighted sums of the two half windows"""
    x = np.asarray(x, np.float32)
    S, M, C = p.frame_shift, p.max_support, p.taps.shape[0]
    T = so.frame_count(len(x), p) if num_frames is None else num_frames
    if not T:
        return np.zeros((0, C), np.float32)
    count = (T + 1) * S
    seg = _stretch(x, first_frame * S + start_of(p) - (M - 1), count + M - 1)
    # (real and imaginary parts apart, as the kernel keeps them: the samples are real)
    gr = np.ascontiguousarray(p.taps.real, np.float32)
    gi = np.ascontiguousarray(p.taps.imag, np.float32) if np.iscomplexobj(p.taps) else None
    yr, yi = np.zeros((C, count), np.float32), np.zeros((C, count), np.float32)
    for k in range(M):
        sk = seg[None, M - 1 - k : M - 1 - k + count]
        yr += gr[:, k, None] * sk
        if gi is not None:
            yi += gi[:, k, None] * sk
    z = yr * yr + yi * yi
    assert z.dtype == np.float32
    if not p.use_power:
        z = np.sqrt(z)
    zb = z.reshape(C, T + 1, S)
    A, B = zb @ p.window[:S].astype(np.float32), zb @ p.window[S:].astype(np.float32)
    return _finish32(np.ascontiguousarray((A[:, :T] + B[:, 1:]).T), p)


# ------------------------------------------------------------------------------------------ error model ----


def frame_energies(signal, num_frames, p, first_frame=0):
    """E_t: the energy of the signal samples within R of frame t's span [t S + start - (M - 1), t S + start + 2 S)"""
    x = np.asarray(signal, np.float64)
    cum = np.concatenate([[0.0], np.cumsum(x * x)])
    t = first_frame + np.arange(num_frames)
    lo = t * p.frame_shift + start_of(p) - (p.max_support - 1) - R
    hi = t * p.frame_shift + start_of(p) + 2 * p.frame_shift + R
    return cum[np.clip(hi, 0, len(x))] - cum[np.clip(lo, 0, len(x))]


def oracle_linear(signal, num_frames, p, first_frame=0):
    """(w, E): the float64 oracle's linear coefficients and the frame energies of the model.  Non-finite samples
    poison the oracle's rows as np.convolve does; they count as zero in E."""
    x = np.asarray(signal, np.float64)
    with np.errstate(all="ignore"):
        w = so.features(x, num_frames, linear_params(p), first_frame)
    E = frame_energies(np.where(np.isfinite(x), x, 0.0), num_frames, p, first_frame)
    w.flags.writeable = E.flags.writeable = False
    return w, E


def kappa_needed(err, w, E, h, W1, use_power, eps, rtol):
    """The smallest kappa for which the model's bound holds, element by element (``err = |got - w|`` linear)"""
    excess = np.maximum(err - rtol * w, 0.0)
    tiny = np.finfo(np.float64).tiny
    if use_power:
        # excess <= b k + a k^2  with  a = eps^2 W1 h^2 E,  b = 2 eps sqrt(w W1 h^2 E)   (the stable root)
        a, b = eps * eps * W1 * h * h * E, 2 * eps * np.sqrt(w * W1 * h * h * E)
        return 2 * excess / np.maximum(b + np.sqrt(b * b + 4 * a * excess), tiny)
    return excess / np.maximum(eps * W1 * h * np.sqrt(E), tiny)


def compare(got, signal, p, kappa, eps=EPS32, rtol=2e-4, atol=2e-5, first_frame=0, pre=None, rows=None):
    """`got` (features as the kernel stores them, frames first_frame .. first_frame + len(got)) against the float64
    oracle on `signal`, under the model.  `pre`: oracle_linear() of the same arguments, if the caller keeps it.
    `rows`: a mask of the frames to hold to the model (non-finite samples: the others are the caller's)."""
    got = np.asarray(got, np.float64)
    T, C = got.shape[0], p.taps.shape[0]
    if got.shape[1:] != (C,):
        return Result(False, np.inf, 0, got.size, f"shape {got.shape} vs (.., {C})")
    w, E = pre if pre is not None else oracle_linear(signal, T, p, first_frame)
    if w.shape != got.shape:
        return Result(False, np.inf, 0, w.size, f"shape {got.shape} vs {w.shape}")
    if not w.size:
        return Result(True, 0.0, 0, 0)
    with np.errstate(all="ignore"):
        want = np.log(np.maximum(w, so.LOG_FLOOR)) if p.use_log else w
        ok_strict = strict_ok(got, want, rtol, atol)
        lin_got = np.exp(got) if p.use_log else got
        lin_want = np.maximum(w, so.LOG_FLOOR) if p.use_log else w
        h = np.sqrt((np.abs(p.taps) ** 2).sum(axis=1))[None, :]
        k = kappa_needed(np.abs(lin_got - lin_want), w, E[:, None], h, float(np.sum(p.window)), p.use_power, eps, rtol)
    k = np.where(E[:, None] > 0, k, np.inf)  # (silent stretches: the strict rule only)
    k = np.where(np.isnan(k), np.inf, k)
    skip = np.zeros(got.shape, bool) if rows is None else ~np.broadcast_to(np.asarray(rows, bool)[:, None], got.shape)
    measured = np.isfinite(k) & ~skip
    kappa_all = float(k[measured].max()) if measured.any() else 0.0
    need = k.copy()
    need[ok_strict] = 0.0
    need[skip] = 0.0
    t, c = np.unravel_index(int(np.argmax(need)), need.shape)
    worst = float(need[t, c])
    bound_only = int(((need > 0) & (need <= kappa)).sum())
    ok = worst <= kappa
    msg = "" if ok else (f"frame {first_frame + t} coefficient {c}: got {got[t, c]!r} want {want[t, c]!r}, needs kappa "
                         f"{worst:.3g} > {kappa:.3g} ({int((need > kappa).sum())} of {want.size} elements fail)")
    return Result(ok, worst, bound_only, int(want.size), msg, (int(first_frame + t), int(c), worst), kappa_all)


def calibrate(names):
    """Worst kappa each restatement needs over cases() of every configuration of `names`, with the case it came from:
    {"fft": ..., "tables": ..., "direct": ...} -> (kappa, configuration, label/kind).  Measured on the linear
    coefficients, over every element of every frame with signal (`Result.kappa_all`), as float32 samples and as
    int16-quantised ones.  Configurations without an FFT form have the direct restatement only."""
    worst = {"fft": (0.0, None, None), "tables": (0.0, None, None), "direct": (0.0, None, None)}
    for name in names:
        p, form = suite_config(name)
        q = linear_params(p)
        for label, x in cases(p):
            for kind, x32 in (("f32", x.astype(np.float32)), ("i16", quantise_i16(x).astype(np.float32))):
                pre = oracle_linear(x32, so.frame_count(len(x32), q), q)
                for which in worst:
                    if which != "direct" and form == (0, 0):
                        continue
                    got = restate_direct(x32, q) if which == "direct" else restate_fft(x32, q, form, which == "tables")
                    r = compare(got, x32, q, kappa=1e30, pre=pre)
                    assert r.ok, (name, which, label, kind, r.message)
                    if r.kappa_all > worst[which][0]:
                        worst[which] = (r.kappa_all, name, f"{label}/{kind}")
    return worst
