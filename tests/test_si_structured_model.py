"""The float32 error model of tests/si_structured.py, checked on the CPU: its calibration, why it exists, its teeth.

Nothing here needs a GPU.  The float32 restatements of the SI oracle (overlap-save with numpy's complex64 FFT, the same
with the kernel's 32 x 32 factorisation and float32 twiddle tables, the direct form with sequential float32 sums) stand
in for a correct float32 kernel: the model must pass them with the committed kappa, ``test_gpu_si.close`` must not (that
is why the model exists), and the model must reject the restatement as soon as it is made wrong the way a defective
kernel would be -- some of which ``close()`` lets through on noise.
"""
import numpy as np
import pytest

from oracle import si_oracle as so
from tests import si_structured as sis
from tests.test_gpu_si import F32 as CLOSE_F32, close

KAPPA = sis.MARGIN * sis.KAPPA_REF_FFT  # what the GPU tests allow the FFT form
FFT_NAMES = [n for n in sis.suite_names() if n != sis.DIRECT_ONLY]


def test_calibration():
    """KAPPA_REF_FFT and KAPPA_REF_DIRECT are what the restatements need here: a numpy (or BLAS) change cannot move
    the calibration silently"""
    worst = sis.calibrate(sis.suite_names())
    for which, (k, name, label) in worst.items():
        print(f"kappa {which} {k:.4f} ({name}, {label})")
    fft = max(worst["fft"], worst["tables"])
    print(f"kappa_ref_fft {fft[0]:.4f} ({fft[1]}, {fft[2]})")
    print(f"kappa_ref_direct {worst['direct'][0]:.4f} ({worst['direct'][1]}, {worst['direct'][2]})")
    assert fft[0] <= sis.KAPPA_REF_FFT, fft
    assert fft[0] > sis.KAPPA_REF_FFT / 2, "the committed constant is stale: more than twice what is measured"
    assert worst["direct"][0] <= sis.KAPPA_REF_DIRECT, worst["direct"]
    assert worst["direct"][0] > sis.KAPPA_REF_DIRECT / 2, "the committed constant is stale: more than twice what is measured"


def test_launch_shape_restatement_and_suite_coverage():
    """si_fft_form_for as restated here gives the sizes the suite's own tests assert, and the configurations cover
    both transform sizes with every window-factor count, both rectifiers, logs and raw sums, real and complex taps,
    both framings, leading virtual zeros and a bank without an FFT form"""
    seen = set()
    for name in sis.suite_names():
        p, (NT, blocks) = sis.suite_config(name)
        if name in sis.BUCKET_CONFIGS:
            assert NT == sis.BUCKET_CONFIGS[name][-1], name
        if NT:
            assert 1 <= blocks <= 8 and blocks * p.frame_shift <= NT - (p.max_support - 1)
            seen.add((NT, sis.window_factors(NT, p.frame_shift)))
        seen.add(("power", p.use_power))
        seen.add(("log", p.use_log))
        seen.add(("complex", np.iscomplexobj(p.taps)))
        seen.add(("centered", p.centered))
        seen.add(("lead", so.stream_start(p)[1] > 0))
    assert {(NT, nw) for NT in (1024, 2048) for nw in (3, 5, 8, 16)} <= seen, seen
    for key in ("power", "log", "complex", "centered", "lead"):
        assert (key, True) in seen and (key, False) in seen, key
    assert sis.suite_config("s6_fbank_long")[1][0] == 2048 and sis.suite_config("gabor41_1024")[1][0] == 1024
    p, form = sis.suite_config(sis.DIRECT_ONLY)
    assert form == (0, 0) and p.taps.shape[0] == sis.direct_only_filters()
    assert sis.suite_config("gabor41_1024")[0].taps.shape[0] == 41


@pytest.mark.parametrize("name", sis.suite_names())
def test_restatements_pass_the_model_on_the_features_themselves(name):
    """The features as a kernel stores them (floored logs, the energy row) and not only the linear coefficients: each
    restatement passes every case with its kappa_ref itself, as float32 and as quantised samples; the oracle's own
    output passes with kappa = 0 and fails once perturbed by 1e-9 (1 + |want|)"""
    p, form = sis.suite_config(name)
    for label, x in sis.cases(p):
        want = so.compute_full(x, p)
        pre = sis.oracle_linear(x, len(want), p)
        assert sis.compare(want, x, p, kappa=0.0, rtol=0.0, atol=1e-12, pre=pre).ok, (name, label)
        assert not sis.compare(want + 1e-9 * (1 + np.abs(want)), x, p, kappa=0.0, rtol=0.0, atol=1e-12, pre=pre).ok
        for x32 in (x.astype(np.float32), sis.quantise_i16(x).astype(np.float32)):
            pre = sis.oracle_linear(x32, len(want), p)
            r = sis.compare(sis.restate_direct(x32, p), x32, p, sis.KAPPA_REF_DIRECT, pre=pre)
            assert r.ok, (name, label, "direct", r.message)
            for tables in (False, True) if form != (0, 0) else ():
                r = sis.compare(sis.restate_fft(x32, p, form, tables), x32, p, sis.KAPPA_REF_FFT, pre=pre)
                assert r.ok, (name, label, "tables" if tables else "fft", r.message)


@pytest.mark.parametrize("name", sis.suite_names())
def test_silence_and_straddle_gain(name):
    p, form = sis.suite_config(name)
    n = sis.utterance_length(p)
    z = np.zeros(n, np.float32)
    # exact silence: E_t = 0 everywhere, so the strict rule alone decides, and it passes the restatements
    gots = [sis.restate_direct(z, p)] + ([sis.restate_fft(z, p, form, True)] if form != (0, 0) else [])
    for got in gots:
        r = sis.compare(got, z, p, kappa=0.0)
        assert r.ok and r.kappa == 0.0 and r.bound_only == 0
        # ... and fails anything else there, whatever kappa: the bound must not turn into an exemption on silence
        r = sis.compare(got + 1e-2, z, p, kappa=1e30)
        assert not r.ok and r.kappa == np.inf
    gain = sis.straddle_gain(p)
    if not p.use_log:
        assert gain is None
        return
    x = gain * np.random.default_rng(7).standard_normal(n)
    share = sis.floor_share(x, p)
    assert 0.2 <= share <= 0.8, (name, gain, share)
    assert dict(sis.cases(p))["noise@straddle"].tolist() == x.tolist()


def fails_close(got, want):
    try:
        close(got, want, **CLOSE_F32)
    except AssertionError:
        return True
    return False


def test_close_fails_a_correct_float32_pipeline():
    """Why the model exists: on a log-magnitude bank the correct float32 overlap-save restatement misses
    test_gpu_si.close -- with its forgiveness of everything below 1e-3 max|want| -- on the low and the high tone, the
    impulses and the chirp, and passes the model through the bound; noise passes close() outright"""
    p, form = sis.suite_config("s1_gabor_mel")
    assert not p.use_power and p.use_log
    sigs = dict(sis.cases(p))
    for label in ("tone_low", "tone_high", "impulses", "chirp"):
        x = sigs[label].astype(np.float32)
        for tables in (False, True):
            got = sis.restate_fft(x, p, form, tables)
            assert fails_close(got, so.compute_full(x.astype(np.float64), p)), (label, tables)
            r = sis.compare(got, x, p, sis.KAPPA_REF_FFT)
            assert r.ok and r.bound_only > 0 and 0 < r.kappa <= sis.KAPPA_REF_FFT, (label, tables, r)
    x = sigs["noise"].astype(np.float32)
    assert not fails_close(sis.restate_fft(x, p, form), so.compute_full(x.astype(np.float64), p))
    assert sis.compare(sis.restate_fft(x, p, form), x, p, sis.KAPPA_REF_FFT).ok


# ---------------------------------------------------------------------------------------------- mutations ----


def nyquist_zeroed(H):
    H = H.copy()
    H[:, H.shape[1] // 2] = 0
    return H


def delayed(H):
    """the filters 1e-3 sample late: a slightly wrong twiddle"""
    return H * np.exp(-2j * np.pi * np.fft.fftfreq(H.shape[1]) * 1e-3)


# mutation -> (arguments of restate_fft, a family the model must reject it on)
MUTANTS = {
    "nyquist_zeroed": (dict(mutate_spectra=nyquist_zeroed), "nyquist"),
    "delayed": (dict(mutate_spectra=delayed), "tone_high"),
    "first_valid": (dict(mutation="first_valid"), "nyquist"),
    "halves_swapped": (dict(mutation="halves_swapped"), "chirp"),
    "last_block_scaled": (dict(mutation="last_block_scaled"), "tone_off@1"),
    "magnitude_for_power": (dict(mutation="magnitude_for_power"), "dc"),
    "window_past_block": (dict(mutation="window_past_block"), "tone_bin"),
}
assert set(sis.MUTATIONS) <= set(MUTANTS)
# mutations test_gpu_si.close lets through on Gaussian noise (for every bank below that they apply to)
PASS_CLOSE_ON_NOISE = ("delayed", "last_block_scaled")


# (s1_gabor_mel is a magnitude bank: it takes the square root anyway)
MUTANT_CASES = [(name, mutant) for name in ("s1_gabor_mel", "s2_gammatone_power", "s6_fbank_long") for mutant in sorted(MUTANTS)
                if (name, mutant) != ("s1_gabor_mel", "magnitude_for_power")]


@pytest.mark.parametrize("name,mutant", MUTANT_CASES)
def test_mutations_are_rejected(name, mutant):
    """A log-magnitude bank (1024 points, complex taps, virtual leading zeros), a causal log-power one and the
    2048-point real one: at the GPU tests' allowance the model rejects every mutated restatement on the family named
    in MUTANTS (and the impulses see the delay too), while the unmutated one passes there; close() on noise lets the
    delayed spectra and the scaled last block through"""
    p, form = sis.suite_config(name)
    kwargs, family = MUTANTS[mutant]
    assert p.use_power or mutant != "magnitude_for_power"
    assert form[1] > 1  # (a block behind a block, a last block that is not the only one)
    sigs = dict(sis.cases(p))
    for label in [family] + (["impulses"] if mutant == "delayed" else []):
        x = sigs[label].astype(np.float32)
        pre = sis.oracle_linear(x, so.frame_count(len(x), p), p)
        assert sis.compare(sis.restate_fft(x, p, form), x, p, KAPPA, pre=pre).ok
        r = sis.compare(sis.restate_fft(x, p, form, **kwargs), x, p, KAPPA, pre=pre)
        print(name, mutant, label, "needs kappa", r.kappa)
        assert not r.ok and r.kappa > KAPPA, (name, mutant, label, r.kappa)
    if mutant in PASS_CLOSE_ON_NOISE:
        x = sigs["noise"].astype(np.float32)
        assert not fails_close(sis.restate_fft(x, p, form, **kwargs), so.compute_full(x.astype(np.float64), p))


def test_nonfinite_rows_are_the_callers():
    """compare(rows=...) holds only the frames named to the model: a NaN sample's rows are skipped, every other row
    is still checked (and a wrong one among them still fails)"""
    p, form = sis.suite_config("s2_gammatone_power")
    x = dict(sis.cases(p))["noise"].astype(np.float32)
    x[len(x) // 2] = np.nan
    with np.errstate(all="ignore"):
        got = sis.restate_direct(x, p)
    bad = ~np.isfinite(so.compute_full(x.astype(np.float64), p)).all(axis=1)
    assert 0 < bad.sum() < len(bad) and np.array_equal(bad, ~np.isfinite(got).all(axis=1))
    assert not sis.compare(got, x, p, KAPPA).ok
    assert sis.compare(got, x, p, KAPPA, rows=~bad).ok
    got[np.argmin(bad)] *= 1.01
    assert not sis.compare(got, x, p, KAPPA, rows=~bad).ok
