"""The window rule and the running sums of sliding-window CMVN (tests/sliding_model.py; CPU only): the three window
properties the kernels rely on, by a brute-force loop over every small case, and the model's subtract-and-add sums
against direct sums with a bound that comes from the operation count."""
import numpy as np
import pytest

from tests.sliding_model import sliding_cmvn, window


def test_window_properties():
    checked = 0
    for W in range(1, 9):
        for min_window in range(1, 12):
            for center in (False, True):
                for T in range(1, 30):
                    prev = None
                    for t in range(T):
                        ws, we = window(t, T, W, min_window, center)
                        assert 0 <= ws <= t < we <= T, (W, min_window, center, T, t, ws, we)
                        assert we - ws <= max(W + 1, min_window)
                        if prev is not None:
                            assert ws - prev[0] in (0, 1) and we - prev[1] in (0, 1), (W, min_window, center, T, t)
                        prev = (ws, we)
                        checked += 1
    assert checked == 8 * 11 * 2 * sum(range(1, 30))


def test_streamable_window_is_the_last_w_plus_one_frames():
    # center=False, min_window=1: what the streaming kernel computes without knowing T
    for W in (1, 4, 7):
        for T in (1, 5, 30):
            for t in range(T):
                assert window(t, T, W, 1, False) == (max(0, t - W), t + 1)


CASES = [(4, 1, False, 3, 40), (5, 3, True, 8, 50), (600, 100, False, 600, 2000), (300, 100, True, 128, 1500)]


@pytest.mark.parametrize("W,min_window,center,refresh,T", CASES)
def test_sums_stay_within_the_operation_count_bound(W, min_window, center, refresh, T):
    """A sum at frame t is built by at most W + 1 additions at the last refresh and, since then, at most `refresh`
    subtractions and `refresh` additions: m = W + 1 + 2 refresh operations of relative error 2^-53 each, over values
    that all lie in the window widened by `refresh` frames to the left (the frames subtracted since the refresh).  Each
    partial sum is bounded by the sum of magnitudes over that widened window, which gives
    |s1^ - s1| <= m 2^-53 sum|x| and, with one more rounding for each square, |s2^ - s2| <= (m + 1) 2^-53 sum x^2."""
    rng = np.random.default_rng(W * 1000 + T)
    x = 20.0 + 5.0 * rng.standard_normal((T, 3))
    _, s1, s2 = sliding_cmvn(x, W, min_window, center, False, refresh)
    wide = x.astype(np.longdouble)
    m = W + 1 + 2 * refresh
    worst = 0.0
    for t in range(T):
        ws, we = window(t, T, W, min_window, center)
        lo = max(0, ws - refresh)
        d1 = np.abs(s1[t].astype(np.longdouble) - wide[ws:we].sum(axis=0))
        d2 = np.abs(s2[t].astype(np.longdouble) - (wide[ws:we] ** 2).sum(axis=0))
        b1 = m * 2.0 ** -53 * np.abs(wide[lo:we]).sum(axis=0)
        b2 = (m + 1) * 2.0 ** -53 * (wide[lo:we] ** 2).sum(axis=0)
        assert (d1 <= b1).all() and (d2 <= b2).all(), (t, d1 / b1, d2 / b2)
        worst = max(worst, float((d1 / b1).max()), float((d2 / b2).max()))
    print(f"W={W} min_window={min_window} center={center} refresh={refresh} T={T}: worst error / bound = {worst:.4f}")
    # (these inputs, 20 + 5 N(0, 1), use a part of the bound: 17.5 % and 6.2 % of it in the two short cases, 1.0 % and
    # 2.2 % in the two long ones with this draw; the bound is the check, the fraction is printed)


def test_refresh_is_part_of_the_result_only_in_the_last_bits():
    rng = np.random.default_rng(5)
    x = (20.0 + 5.0 * rng.standard_normal((200, 4))).astype(np.float32)
    a, _, _ = sliding_cmvn(x, 30, 10, False, True, 7)
    b, _, _ = sliding_cmvn(x, 30, 10, False, True, 1)  # every frame summed afresh
    assert a.dtype == np.float32 and np.allclose(a, b, rtol=1e-5, atol=1e-6)


def test_a_nan_frame_is_forgotten_at_the_refresh_after_it_left():
    rng = np.random.default_rng(6)
    x = rng.standard_normal((60, 2))
    x[10] = np.nan
    W, refresh = 4, 8
    y, _, _ = sliding_cmvn(x, W, 1, False, False, refresh)
    # frame 10 is in the windows of frames 10 .. 14; the sums carry it until the refresh at 16
    bad = np.isnan(y).any(axis=1)
    assert bad[10:16].all() and not bad[:10].any() and not bad[16:].any()
