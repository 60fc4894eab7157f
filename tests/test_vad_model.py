"""The numpy model of the energy VAD (tests/vad_model.py; CPU only) against a literal loop restatement of Kaldi's
``ComputeVadEnergy`` on integer-valued energies, whose sums are exact in any order, and on the ties of the rule."""
import numpy as np
import pytest

from tests.vad_model import energy_sum, select_rows, threshold, vad_decide, vad_decide_rows


def kaldi_loop(e, energy_threshold, energy_mean_scale, frames_context, proportion_threshold):
    """Kaldi's function as it is written there: the threshold from the plain sum of the log energies, then per frame
    a count over the window cut at the utterance's ends"""
    T = len(e)
    thr = energy_threshold
    if energy_mean_scale != 0.0:
        total = 0.0
        for t in range(T):
            total += float(e[t])
        thr += energy_mean_scale * total / T
    out = []
    for t in range(T):
        num = den = 0
        for t2 in range(t - frames_context, t + frames_context + 1):
            if 0 <= t2 < T:
                den += 1
                if float(e[t2]) > thr:
                    num += 1
        out.append(num >= den * proportion_threshold)
    return np.asarray(out, dtype=bool)


@pytest.mark.parametrize("context", [0, 1, 2, 5])
def test_integer_energies_give_kaldis_decisions(context):
    rng = np.random.default_rng(context)
    voiced = unvoiced = 0
    for T in range(1, 201):
        # multiples of 4 whatever T: energy_mean_scale 0.5 and 0.25 keep the threshold's product exact, and sums of a
        # few hundred small integers are exact in any order; T divides them with one rounding in both forms
        e = 4.0 * rng.integers(-3, 9, size=T)
        for scale, p in ((0.5, 0.6), (0.25, 0.5), (0.0, 0.3)):
            want = kaldi_loop(e, 5.0, scale, context, p)
            got = vad_decide(e, 5.0, scale, context, p)
            assert got.dtype == bool and got.shape == (T,) and (got == want).all(), (T, scale, p)
            voiced += int(want.sum())
            unvoiced += int((~want).sum())
    assert voiced > 1000 and unvoiced > 1000


def test_an_energy_equal_to_the_threshold_is_unvoiced():
    # thr = 5 + 0.5 * (6 + 10 + 14) / 3 = 10: the frame at 10 ties and stays unvoiced, the one above is voiced
    e = np.asarray([6.0, 10.0, 14.0])
    assert threshold(e, 5.0, 0.5) == 10.0
    assert vad_decide(e).tolist() == [False, False, True]
    assert vad_decide(np.asarray([7.0, 7.0]), 7.0, 0.0).tolist() == [False, False]
    assert vad_decide(np.asarray([7.0, np.nextafter(7.0, 8.0)]), 7.0, 0.0).tolist() == [False, True]


def test_a_vote_equal_to_the_proportion_is_voiced():
    # context 1 at the left edge: den = 2, num = 1, and 1 >= 2 * 0.5 holds with equality
    e = np.asarray([9.0, 0.0, 0.0, 0.0])
    got = vad_decide(e, 5.0, 0.0, 1, 0.5)
    assert got.tolist() == [True, False, False, False]  # frame 1: 1 of 3 < 1.5
    # ... and just above one half it fails
    assert vad_decide(e, 5.0, 0.0, 1, np.nextafter(0.5, 1.0)).tolist() == [False] * 4
    # the right edge alike; in the middle 2 of 4 frames of context 2 at p = 0.5
    assert vad_decide(e[::-1], 5.0, 0.0, 1, 0.5).tolist() == [False, False, False, True]
    e = np.asarray([9.0, 9.0, 0.0, 0.0])
    assert vad_decide(e, 5.0, 0.0, 2, 0.5).tolist() == [True, True, True, False]  # 2/3, 2/4, 2/4, 1/3


def test_the_sum_is_the_sixty_four_interleaved_partials():
    rng = np.random.default_rng(64)
    e = rng.standard_normal(1000) * 10.0 ** rng.integers(-8, 9, size=1000)
    partial = [0.0] * 64
    for t, v in enumerate(e.tolist()):
        partial[t % 64] += v
    s = 0.0
    for p in partial:
        s += p
    assert energy_sum(e) == s
    assert s != float(np.sum(e)) or s != sum(e.tolist())  # (the order is part of the result)
    # side by side: columns are utterances
    both = energy_sum(np.stack([e, e[::-1]], axis=1))
    assert both[0] == s and both[1] == energy_sum(e[::-1])
    # a sum that starts from +0.0 is never -0.0
    assert not np.signbit(energy_sum(np.asarray([-0.0, -0.0])))


def test_non_finite_energies_and_empty_utterances():
    assert vad_decide(np.zeros(0)).shape == (0,)
    nan, inf = float("nan"), float("inf")
    # a NaN sum: a NaN threshold, nothing is above it; without the mean the NaN frame alone is unvoiced
    assert vad_decide(np.asarray([20.0, nan, 20.0])).tolist() == [False] * 3
    assert vad_decide(np.asarray([20.0, nan, 20.0]), 5.0, 0.0).tolist() == [True, False, True]
    assert vad_decide(np.asarray([20.0, inf, 20.0])).tolist() == [False] * 3  # thr = +inf, and inf > inf is false
    assert vad_decide(np.asarray([20.0, -inf, 20.0])).tolist() == [True, False, True]  # thr = -inf
    assert vad_decide(np.asarray([inf, -inf])).tolist() == [False, False]  # inf - inf: NaN


def test_rows_and_selection():
    feats = np.arange(24, dtype=np.float32).reshape(8, 3)
    feats[:, 1] = [0, 9, 9, 0, 0, 9, 0, 0]
    rows = np.asarray([1, 4, 4, 7])
    voiced, counts = vad_decide_rows(feats, rows, energy_col=1, energy_threshold=5.0, energy_mean_scale=0.0)
    assert voiced.dtype == np.uint8 and voiced.tolist() == [0, 1, 1, 0, 0, 1, 0, 0] and counts.tolist() == [2, 0, 1]
    out, offs = select_rows(feats, rows, voiced)
    assert offs.tolist() == [0, 2, 2, 3] and (out == feats[[1, 2, 5]]).all()
