"""The float32 error model of tests/structured.py, checked on the CPU: its calibration, why it exists, its teeth.

Nothing here needs a GPU.  The float32 restatements of the oracle (numpy's float32 rFFT, a float32 DFT-matrix product)
stand in for a correct float32 kernel: the model must pass them with the committed kappa, the suite's strict
tolerance must not (that is why the model exists), and the model must reject the restatement as soon as its
spectrum is perturbed the way a defective kernel would perturb it.
"""
import numpy as np
import pytest

from oracle import stft_oracle as orc
from tests import structured as st

KAPPA = st.MARGIN * st.KAPPA_REF  # what the GPU tests allow a float32 kernel


def test_calibration():
    """KAPPA_REF and KAPPA_REF_DFT are what the restatements need here: a numpy (or BLAS) change cannot move the
    calibration silently"""
    configs = st.suite_configs()
    k, name, label = st.calibrate(configs, st.restate_f32)
    print(f"kappa_ref {k:.4f} ({name}, {label})")
    assert k <= st.KAPPA_REF, (k, name, label)
    assert k > st.KAPPA_REF / 2, "the committed constant is stale: far above what is measured"
    k, name, label = st.calibrate([c for c in configs if c[1].dft_size <= 1024], st.restate_f32_dft)
    print(f"kappa_ref_dft {k:.4f} ({name}, {label})")
    assert k <= st.KAPPA_REF_DFT, (k, name, label)
    assert k > st.KAPPA_REF_DFT / 2, "the committed constant is stale: far above what is measured"


@pytest.mark.parametrize("name", st.FIXTURE_CONFIGS + ["n256_tri_8k", "n2048_gammatone_44k", "nopad240_fbank_8k"])
def test_restatement_passes_the_model_on_the_features_themselves(name):
    """The features as a kernel stores them (floored logs, energy column) and not only the linear coefficients:
    the restatement passes every case with kappa_ref itself, as float32 and as quantised samples"""
    p = st.suite_config(name)[0]
    for label, x in st.cases(p):
        # compare() forms the oracle's features from frame_spectra and weights_dense: the same numbers as compute_full
        want = orc.compute_full(x, p)
        assert st.compare(want, x, p, kappa=0.0, rtol=0.0, atol=1e-12).ok, (name, label)
        assert not st.compare(want + 1e-9 * (1 + np.abs(want)), x, p, kappa=0.0, rtol=0.0, atol=1e-12).ok
        for x32 in (x.astype(np.float32), st.quantise_i16(x).astype(np.float32)):
            r = st.compare(st.restate_f32(x32, p), x32, p, st.KAPPA_REF)
            assert r.ok, (name, label, r.message)
            if p.dft_size <= 1024:
                r = st.compare(st.restate_f32_dft(x32, p), x32, p, st.KAPPA_REF_DFT)
                assert r.ok, (name, label, "dft", r.message)


def test_strict_tolerance_fails_a_correct_float32_pipeline():
    """Why the model exists: on two tones 80 dB apart (and on the step and the chirp) the float32 restatement misses
    1e-5 + 1e-4 |ref| on a share of the elements no kernel could avoid, and passes the model through the bound"""
    p = st.suite_config("c3_fbank80_energy")[0]
    sigs = dict(st.cases(p))
    for label, least in (("two_tone_80db", 0.01), ("step", 0.002), ("chirp", 0.002)):
        x = sigs[label].astype(np.float32)
        got = st.restate_f32(x, p)
        share = 1.0 - st.strict_ok(got, orc.compute_full(x.astype(np.float64), p)).mean()
        print(label, "strict failures", share)
        assert share > least, (label, share)
        r = st.compare(got, x, p, st.KAPPA_REF)
        assert r.ok and r.bound_only > 0 and 0 < r.kappa <= st.KAPPA_REF, (label, r)
    # the control: noise passes the strict check outright
    x = sigs["noise"].astype(np.float32)
    r = st.compare(st.restate_f32(x, p), x, p, st.KAPPA_REF)
    assert r.ok and r.bound_only == 0 and r.kappa == 0.0


@pytest.mark.parametrize("name", sorted(st.suite_names()))
def test_silence_floor_levels_and_straddle_gain(name):
    p = st.suite_config(name)[0]
    n = st.utterance_length(p)
    # exact silence: A_t = 0 everywhere, so the strict check alone decides, and it passes the restatement
    z = np.zeros(n, np.float32)
    r = st.compare(st.restate_f32(z, p), z, p, kappa=0.0)
    assert r.ok and r.kappa == 0.0 and r.bound_only == 0
    # ... and fails anything else there, whatever kappa: the bound must not turn into an exemption on silent frames
    r = st.compare(st.restate_f32(z, p) + 1e-2, z, p, kappa=1e30)
    assert not r.ok and r.kappa == np.inf
    gain = st.straddle_gain(p)
    if not p.use_log:
        assert gain is None
        return
    x = gain * np.random.default_rng(7).standard_normal(n)
    share = st.floor_share(x, p)
    assert 0.2 <= share <= 0.8, (name, gain, share)
    assert dict(st.cases(p, gain=gain))["noise@straddle"].tolist() == x.tolist()
    # the lowest level puts every coefficient of a power bank on the floor (magnitudes are ~1e5 times larger)
    if p.use_power:
        assert st.floor_share(dict(st.cases(p, gain=gain))["noise@0.001"], p) == 1.0
    x32 = x.astype(np.float32)
    r = st.compare(st.restate_f32(x32, p), x32, p, st.KAPPA_REF)
    assert r.ok, r.message


# ---------------------------------------------------------------------------------------------- mutations ----


def dc_doubled(sp):
    sp = sp.copy()
    sp[:, 0] *= 2
    return sp


def nyquist_dropped(sp):
    sp = sp.copy()
    sp[:, -1] = 0
    return sp


def swap_bins(k):
    def swapped(sp):
        sp = sp.copy()
        sp[:, [k, k + 1]] = sp[:, [k + 1, k]]
        return sp
    return swapped


def scale_bin(k, factor=1 + 1e-3):
    def scaled(sp):
        sp = sp.copy()
        sp[:, k] *= factor
        return sp
    return scaled


def twiddle_noise(sp):
    """1e-6 of the frame's peak amplitude on every bin (a sine table good to 20 bits)"""
    rng = np.random.default_rng(3)
    peak = np.abs(sp).max(axis=1, keepdims=True)
    return sp + 1e-6 * peak * (rng.standard_normal(sp.shape) + 1j * rng.standard_normal(sp.shape))


def rejected_on(p, mutate):
    """The families on which the model, at the GPU tests' kappa, rejects the mutated restatement"""
    out = []
    for label, x in st.cases(p):
        x32 = x.astype(np.float32)
        if not st.compare(st.restate_f32(x32, p, mutate), x32, p, KAPPA).ok:
            out.append(label)
    return out


def noise_passes_strict(p, mutate):
    x = dict(st.cases(p))["noise"].astype(np.float32)
    return bool(st.strict_ok(st.restate_f32(x, p, mutate), orc.compute_full(x.astype(np.float64), p)).all())


@pytest.mark.parametrize("name", ["c4_gabor64", "c5_gammatone64_48k", "n512_partial_row"])
def test_dc_and_nyquist_mutations_are_rejected(name):
    """Banks that weigh bins 0 and N/2 (the complex ones: their filters wrap around the spectrum's ends)"""
    p = st.suite_config(name)[0]
    W = orc.weights_dense(p)
    assert W[:, 0].max() > 0 and W[:, -1].max() > 0
    got = rejected_on(p, dc_doubled)
    assert "dc" in got and "dc_noise" in got, got
    got = rejected_on(p, nyquist_dropped)
    assert "nyquist" in got, got


def test_dc_and_nyquist_mutations_pass_the_noise_control():
    """The gap this suite closes, written down: on the headline bank a kernel whose DC bin is doubled or whose
    Nyquist bin is lost passes the strict check on white noise -- the triangular (and fbank) banks give both bins no
    weight at all, so only the banks of test_dc_and_nyquist_mutations_are_rejected can tell"""
    p = st.suite_config("c2_tri_mel40")[0]
    assert noise_passes_strict(p, dc_doubled)
    assert noise_passes_strict(p, nyquist_dropped)
    assert orc.weights_dense(p)[:, [0, -1]].max() < 1e-20
    # (that bank's defence is the bins next to them: the two-step real FFT's other special cases)
    assert rejected_on(p, swap_bins(1)) and rejected_on(p, scale_bin(1, 2.0))
    assert rejected_on(p, swap_bins(p.dft_size // 2 - 2))


@pytest.mark.parametrize("name", st.FIXTURE_CONFIGS)
def test_bin_mutations_are_rejected(name):
    p = st.suite_config(name)[0]
    N = p.dft_size
    # two neighbouring bins swapped, next to the tone at N // 7 + 0.37 and in the middle of the band
    for k in (N // 7, N // 4):
        assert rejected_on(p, swap_bins(k)), (name, "swap", k)
    # one bin 0.1 % too large.  At amplitude 3000 the log features are ~25 and the strict rule's 1e-4 |ref| is
    # 0.25 % of the linear coefficient, so the suite has always let this through there; the [-1, 1] level, whose
    # logs are near 0, shows it
    got = rejected_on(p, scale_bin(N // 7))
    assert "tone_off@1" in got, (name, got)
    # a low-accuracy twiddle table: 1e-6 of the peak on every bin is ~17 eps -- the tones' empty bins show it
    got = rejected_on(p, twiddle_noise)
    assert got and "noise" not in got, (name, got)
