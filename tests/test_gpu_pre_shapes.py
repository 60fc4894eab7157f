"""The pre-processor kernels of csrc/pre.hip past the sizes one grid covers: utterances longer than 4096 blocks (the
grid-stride loops of preemph_kernel and dither_packed_kernel), more than 65535 rows (two calls), integer and
non-finite samples; and the argument checks of Preemphasize.apply_packed.  Bit for bit against the oracle."""
import numpy as np
import pytest

from oracle import stft_oracle as orc
from pydrobert_speech_amd.pre import Dither, Preemphasize

pytestmark = pytest.mark.gpu

GRID = 4096 * 256  # samples (pre-emphasis) or pairs of samples (dither) one pass of the capped grid covers


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_packed_preemphasis_of_an_utterance_longer_than_the_grid(dtype):
    import torch

    lens = [5, GRID + 257, 1, 0, 300, GRID]  # the long one enters the loop's second turn; the last fills one turn exactly
    gaps = [2, 0, 3, 1, 0, 4, 5]  # in front of each utterance and behind the last
    offs = np.cumsum(np.asarray(gaps[:-1]) + np.asarray([0] + lens[:-1]))
    total = int(offs[-1] + lens[-1] + gaps[-1])
    buf = (3000 * np.random.default_rng(3).standard_normal(total)).astype(dtype)
    out = Preemphasize(0.97).apply_packed(torch.from_numpy(buf).cuda(), offs, lens)
    assert out.is_cuda and out.shape == (total,)
    out = out.cpu().numpy()
    covered = np.zeros(total, dtype=bool)
    for o, n in zip(offs, lens):
        assert same_bytes(out[o : o + n], orc.preemphasize(buf[o : o + n], 0.97)), n
        covered[o : o + n] = True
    assert (~covered).sum() == sum(gaps) and same_bytes(out[~covered], buf[~covered])
    assert not same_bytes(out[offs[1] + GRID : offs[1] + lens[1]], buf[offs[1] + GRID : offs[1] + lens[1]])


def test_preemphasis_of_more_rows_than_one_call_takes():
    rng = np.random.default_rng(4)
    x = (3000 * rng.standard_normal((65535 + 5, 3))).astype(np.float32)
    got = Preemphasize(0.9).apply(x)
    assert same_bytes(got, orc.preemphasize(x, 0.9))
    assert not same_bytes(got[65535:, 1:], x[65535:, 1:])


def test_preemphasis_of_integer_and_non_finite_samples():
    rng = np.random.default_rng(5)
    # (within +-16000: x[i] - 0.97 x[i-1] stays inside int16, whose cast of anything else numpy leaves undefined)
    pcm = np.clip(np.rint(9000 * rng.standard_normal((3, 700))), -16000, 16000).astype(np.int16)
    pcm[0, :4] = (16000, -16000, -16000, 16000)
    got = Preemphasize(0.97).apply(pcm)
    assert same_bytes(got, orc.preemphasize(pcm, 0.97))
    for dtype in (np.float32, np.float64):
        x = (3000 * rng.standard_normal((2, 600))).astype(dtype)
        x[0, 10], x[0, 300], x[1, 0], x[1, 599] = np.inf, np.nan, -np.inf, np.nan
        x[1, 100:102] = np.inf  # inf - 0.97 inf
        with np.errstate(invalid="ignore"):
            want = orc.preemphasize(x, 0.97)
        got = Preemphasize(0.97).apply(x)
        assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
        assert np.isnan(got[1, 101]) and np.isnan(got[0, 300:302]).all() and np.isfinite(got[0, 302:]).all()
        assert np.isnan(got).sum() == 4 and np.isinf(got).sum() == 6


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_packed_dither_of_an_utterance_longer_than_the_grid(dtype):
    import torch

    lens = [7, 2 * GRID + 3, 300]  # GRID + 2 pairs: the loop's second turn, and a last sample without a partner
    offs = np.array([1, 11, 2 * GRID + 20])
    seeds = [5, 2 ** 40 + 1, 9]
    total = int(offs[-1] + lens[-1] + 2)
    x = (3000 * np.random.default_rng(6).standard_normal(total)).astype(dtype)
    d = Dither(1.5, seed=77)
    got = d.apply_packed(torch.from_numpy(x).cuda(), offs, lens, seeds=seeds).cpu().numpy()
    covered = np.zeros(total, dtype=bool)
    for o, n, s in zip(offs, lens, seeds):
        want = Dither(1.5, seed=s).apply(x[o : o + n])
        assert same_bytes(got[o : o + n], want), n
        assert not same_bytes(want[-3:], x[o + n - 3 : o + n])
        covered[o : o + n] = True
    assert same_bytes(got[~covered], x[~covered])


def test_packed_preemphasis_argument_errors():
    import torch

    x = torch.zeros(100, dtype=torch.float32, device="cuda")
    p = Preemphasize(0.97)
    with pytest.raises(ValueError, match="1-D GPU tensor"):
        p.apply_packed(x.reshape(10, 10), [0], [10])
    with pytest.raises(ValueError, match="1-D GPU tensor"):
        p.apply_packed(x.cpu(), [0], [10])
    for other in (torch.int16, torch.int32, torch.float16):
        with pytest.raises(ValueError, match="float32 or float64"):
            p.apply_packed(x.to(other), [0], [10])
    with pytest.raises(ValueError, match="one offset per length"):
        p.apply_packed(x, [0], [10, 10])
    with pytest.raises(ValueError, match="one offset per length"):
        p.apply_packed(x, [0, 10], [10])
    with pytest.raises(ValueError, match="outside signal"):
        p.apply_packed(x, [95], [10])
    with pytest.raises(ValueError, match="outside signal"):
        p.apply_packed(x, [-1], [10])
    with pytest.raises(ValueError, match="outside signal"):
        p.apply_packed(x, [0], [-1])
    with pytest.raises(ValueError, match="outside signal"):
        p.apply_packed(x.to(torch.float64), [0, 50], [50, 51])
    assert p.apply_packed(x, [], []).shape == (100,)
    ones = torch.ones(100, dtype=torch.float64, device="cuda")
    got = p.apply_packed(ones, [90], [10]).cpu().numpy()  # up to the last sample
    assert got[:91].tolist() == [1.0] * 91 and np.array_equal(got[91:], np.full(9, 1.0 - 0.97))
