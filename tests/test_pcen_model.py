"""The numpy model of ``post.PCEN`` (tests/pcen_model.py) against what the definition implies, no device: a constant
input, ``smooth = 1``, the time-constant rule and the one-pole difference equation run element by element."""
import math

import numpy as np
import pytest

from pydrobert_speech_amd.post import PCEN
from tests.pcen_model import compress_model, energies, pcen_model, same_bits, smooth_model


def test_a_constant_input_gives_a_constant_smoother_and_the_closed_form():
    # dyadic smooth and values: oms * v and smooth * v are exact and sum to v, so M is v to the bit
    for smooth in (0.5, 0.25, 0.125):
        post = PCEN(smooth=smooth, gain=0.98, bias=2.0, power=0.5, eps=1e-6)
        assert post.oms == 1.0 - smooth
        for v in (0.0, 1.0, 3.0, 1024.0, 0.375):
            E = np.full((50, 3), v)
            y, M = pcen_model(post, E)
            assert same_bits(M, E)
            want = math.pow(v / math.pow(1e-6 + v, 0.98) + 2.0, 0.5) - math.pow(2.0, 0.5)
            assert y.dtype == np.float64 and np.allclose(y, want, rtol=1e-13, atol=1e-15)
    # any smooth: M stays v within the rounding of its three operations a step
    post = PCEN()
    _, M = pcen_model(post, np.full((1000, 2), 7.3))
    assert np.abs(M / 7.3 - 1.0).max() < 1000 * 3 * np.finfo(np.float64).eps


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_smooth_of_one_gives_the_input(dtype):
    post = PCEN(smooth=1.0)
    assert post.oms == 0.0
    E = energies(np.random.default_rng(0), (200, 7), dtype)
    M = smooth_model(post, E)
    assert M.dtype == np.float64 and same_bits(M, E.astype(np.float64))


def test_from_time_constant_is_its_formula():
    for tc, shift in ((0.4, 10.0), (0.06, 10.0), (1.0, 16.0), (0.4, 32.0)):
        T = tc / (shift / 1000.0)
        want = (math.sqrt(1.0 + 4.0 * T * T) - 1.0) / (2.0 * T * T)
        post = PCEN.from_time_constant(tc, shift, gain=0.8, bias=10.0, power=0.25, eps=1e-8)
        assert post.smooth_coeff == pytest.approx(want, rel=1e-15) and 0.0 < post.smooth_coeff <= 1.0
        assert (post.gain, post.bias, post.power, post.eps) == (0.8, 10.0, 0.25, 1e-8)
    assert PCEN.from_time_constant().smooth_coeff == pytest.approx(0.02468945304871, rel=1e-12)  # librosa's default, b
    assert PCEN.from_time_constant(0.4, 10.0).smooth_coeff == PCEN.from_time_constant().smooth_coeff
    for bad in ((0.0, 10.0), (-1.0, 10.0), (0.4, 0.0), (float("nan"), 10.0), (0.4, float("inf"))):
        with pytest.raises(ValueError):
            PCEN.from_time_constant(*bad)
    with pytest.raises(ValueError):
        PCEN.from_time_constant(0.4, 10.0, smooth=0.1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_smoother_is_the_difference_equation_element_by_element(dtype):
    post = PCEN(smooth=0.025)
    E = energies(np.random.default_rng(1), (300, 5), dtype)
    M = smooth_model(post, E)
    oms, s = post.oms, post.smooth_coeff  # (Python floats: IEEE doubles, every operation rounded once)
    for c in range(E.shape[1]):
        m = float(E[0, c])
        assert M[0, c] == m
        for t in range(1, len(E)):
            kept = oms * m
            fresh = s * float(E[t, c])
            m = kept + fresh
            assert M[t, c] == m, (t, c)
    # y is the formula over (E, M), rounded once to the row type
    y = compress_model(post, E, M)
    assert y.dtype == dtype
    t, c = 17, 3
    want = math.pow(float(E[t, c]) / math.pow(post.eps + M[t, c], post.gain) + post.bias, post.power) - post.bp
    assert y[t, c] == pytest.approx(want, rel=1e-6 if dtype == np.float32 else 1e-13, abs=1e-12)
    assert post.bp == float(np.float64(2.0) ** np.float64(0.5))


def test_nan_and_infinity_stay_in_the_smoother():
    post = PCEN()
    E = energies(np.random.default_rng(2), (40, 3), np.float64, zeros=0.0)
    E[10, 0] = np.nan
    E[20, 1] = np.inf
    y, M = pcen_model(post, E)
    assert np.isnan(M[10:, 0]).all() and not np.isnan(M[:10, 0]).any()
    assert np.isinf(M[20:, 1]).all() and np.isfinite(M[:20, 1]).all()
    assert np.isfinite(M[:, 2]).all() and np.isnan(y[10:, 0]).all() and np.isnan(y[20, 1])
    assert np.isfinite(y[21:, 1]).all()  # (E / inf = 0: the gain control has shut the channel)
    assert pcen_model(post, np.zeros((0, 4), dtype=np.float32))[0].shape == (0, 4)
