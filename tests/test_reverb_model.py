"""tests/reverb_model.py on the CPU: the calibration of the error model recomputed, the restatement inside the bound
with margin 1, the plan's known answers, the counter against the three other rules', the peak's tie rule, and the
window of locality checked on the restatement by poking one sample."""
import os
import re

import numpy as np
import pytest

from tests import mix_model
from tests import reverb_model as rm
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "pydrobert-speech_amd", "csrc")


def test_calibration():
    worst = rm.calibrate()
    print("worst kappa", worst, "committed", rm.KAPPA_REF_REVERB, rm.KAPPA_REF_REVERB_SHORT)
    for which, committed in (("long", rm.KAPPA_REF_REVERB), ("short", rm.KAPPA_REF_REVERB_SHORT)):
        assert worst[which][0] <= committed, (which, worst[which])
        assert worst[which][0] >= 0.5 * committed, (which, worst[which])  # (a constant far above its measurement)
    assert rm.kappa_ref(511) == rm.KAPPA_REF_REVERB_SHORT and rm.kappa_ref(512) == rm.KAPPA_REF_REVERB


@pytest.mark.parametrize("L,d", [(1, 0), (2, 1), (7, 3), (511, 510), (512, 0), (513, 512), (1025, 511), (1537, 1536)])
def test_the_restatement_meets_the_bound_with_margin_one(L, d):
    h = rm.response(L, d)
    assert rm.peak(h) == d
    for n in (0, 1, 2, 511, 512, 513, 1023, 1024, 1025, 2049):
        for label, x in rm.signals(n, seed=n)[::3]:
            x32 = x.astype(np.float32)
            ok, k, msg = rm.check(rm.restate(x32, h, d), x32, h, d, rm.kappa_ref(n))
            assert ok, (L, d, n, label, msg)


def test_a_silent_window_gives_exact_zeros_and_a_wrong_shift_fails():
    h = rm.response(700, 100)
    x = np.zeros(6000, dtype=np.float32)
    x[5000:5100] = 1000.0
    got = rm.restate(x, h, 100)
    E = rm.window_energy(x, 100, rm.partitions(700))
    assert (E == 0).any() and not got[E == 0].any()
    assert rm.check(got, x, h, 100, rm.KAPPA_REF_REVERB)[0]
    assert not rm.check(np.roll(got, 1), x, h, 100, rm.MARGIN * rm.kappa_ref(len(x)))[0]
    assert not rm.check(got * np.float32(1.001), x, h, 100, rm.MARGIN * rm.kappa_ref(len(x)))[0]
    dust = got.copy()
    dust[np.flatnonzero(E == 0)[0]] = 1e-30
    assert not rm.check(dust, x, h, 100, rm.MARGIN * rm.kappa_ref(len(x)))[0]


def test_the_plans_known_answers():
    assert rm.draw((0xFFFFFFFF, 0, 0, 0), 7, 1.0) == (6, True)
    assert rm.draw((0, 0, 0, 0xFFFFFFFF), 7, 1.0) == (0, True)
    assert rm.draw((0, 0, 0, 0), 7, 0.0) == (0, False) and rm.draw((0, 0, 0, 0xFFFFFFFF), 7, 0.0) == (0, False)
    assert rm.draw((0, 0, 0, 0x7FFFFFFF), 1, 0.5)[1] and not rm.draw((0, 0, 0, 0x80000000), 1, 0.5)[1]
    for K in (1, 2, 64, 1000003):
        assert rm.draw((0xFFFFFFFF, 0, 0, 0), K, 1.0)[0] == K - 1
    assert mix_model.philox4x32_10((0, 0, 0, 0), 0) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    rir, applied = rm.plan([1, 2, 3, 1], 5, 0.5)
    assert rir[0] == rir[3] and applied[0] == applied[3] and ((0 <= rir) & (rir < 5)).all()


def test_the_counter_differs_from_the_other_three_rules():
    assert rm.COUNTER == (0, 0, 0, 0x52495231) and rm.COUNTER != tuple(mix_model.COUNTER)
    with open(os.path.join(CSRC, "reverb_rule.h")) as fh:
        rule = fh.read()
    assert re.search(r"REVERB_COUNTER_3 = 0x52495231u", rule)
    with open(os.path.join(CSRC, "mix_rule.h")) as fh:
        assert "MIX_COUNTER_3 = 0x4D495831u" in fh.read()
    # dither_noise.h and specaug_rule.h leave the fourth counter word zero (mix_rule.h says how they form theirs)
    for name in ("dither_noise.h", "specaug_rule.h"):
        with open(os.path.join(CSRC, name)) as fh:
            assert "0x52495231" not in fh.read()
    assert rm.draws(12345) != mix_model.philox4x32_10(mix_model.COUNTER, 12345)


def test_the_first_maximum_wins_a_tie():
    assert rm.peak([0.0, -2.0, 1.0, 2.0, -2.0]) == 1
    assert rm.peak([0.0, 0.0]) == 0 and rm.peak([3]) == 0
    assert rm.peak(np.asarray([1, -32768, 32767], dtype=np.int16)) == 1  # (compared as float64: no int16 overflow)
    assert rm.peak([0.0, 5.0, 1.0], shift_output=False) == 0
    f = np.asarray([1.0, 1.0 + 2.0 ** -40], dtype=np.float64)
    assert rm.peak(f) == 1


@pytest.mark.parametrize("L,d", [(2, 0), (513, 1), (1537, 512)])
def test_the_window_of_locality_holds_on_the_restatement(L, d):
    rng = np.random.default_rng(L)
    h = rm.response(L, d)
    P = rm.partitions(L)
    n = 6000
    x = (3000 * rng.standard_normal(n)).astype(np.float32)
    base = rm.restate(x, h, d)
    t = np.arange(n)
    for i in (0, 700, 2047, 2048, 3333, n - 1):
        poked = x.copy()
        poked[i] = np.float32(1e6)
        got = rm.restate(poked, h, d)
        b0 = rm.BLOCK * ((t + d) // rm.BLOCK)
        inside = (b0 - rm.BLOCK * (P + 2) <= i) & (i < b0 + 3 * rm.BLOCK)
        assert got[~inside].tobytes() == base[~inside].tobytes(), i
        lo, hi = rm.window_of(int(np.flatnonzero(inside)[0]), d, P)
        assert lo <= i < hi
        # ... and the window is not idle: the samples the exact sum reaches do change
        reached = (t + d - i >= 0) & (t + d - i < L)
        assert (got[reached] != base[reached]).any() and inside[reached].all()


def test_the_normalisation_model():
    rng = np.random.default_rng(3)
    x = (3000 * rng.standard_normal(20000)).astype(np.float32)
    wet = (0.25 * x).astype(np.float32)
    ps, py, c, out = rm.normalise(x, wet)
    assert c == 4.0 and out.tobytes() == x.tobytes()
    assert rm.normalise(np.zeros(5, np.float32), wet[:5])[2] == 0.0
    assert rm.normalise(x[:5], np.zeros(5, np.float32))[2] == 0.0
    bad = wet.copy()
    bad[7] = np.nan
    assert rm.normalise(x, bad)[2] == 0.0 and rm.normalise(x, bad)[3].tobytes() == bad.tobytes()
    i16 = np.asarray([100, -200, 300], dtype=np.int16)
    assert rm.copied(i16).tobytes() == np.asarray([100, -200, 300], dtype=np.float32).tobytes()
