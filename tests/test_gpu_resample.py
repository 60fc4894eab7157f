"""``pre.Resample`` on the GPU against the numpy model of its definition (tests/resample_model.py), bit for bit: one
ragged packed batch per launch with odd offsets and poisoned gaps, ``apply`` on arrays and tensors, equal rates, NaN
and infinite samples, other dtypes and the refusals.  The model is given the object's own weight table, so the kernel
is judged on its arithmetic."""
import functools

import numpy as np
import pytest

from pydrobert_speech_amd.pre import Resample
from tests import resample_model as model

pytestmark = pytest.mark.gpu

RATE_PAIRS = [(1, 2), (2, 1), (3, 2), (2, 3), (7, 5), (44100, 16000), (16000, 11025)]
DTYPES = [np.float32, np.float64, np.int16]
GROUP = 256  # outputs a workgroup produces (csrc/resample.hip)


def rate_id(rates):
    return f"{rates[0]}to{rates[1]}"


@functools.lru_cache(maxsize=None)
def resampler(rates):
    return Resample(*rates)


def lengths_of(rs):
    """the utterance lengths of the batch: the edges of the definition, of the units and of the launch shape"""
    def giving(m):  # the shortest utterance with at least m outputs
        return -(-m * rs.in_unit // rs.out_unit)

    lens = [0, 1, 2, rs.max_taps - 1, rs.max_taps, rs.in_unit - 1, rs.in_unit, rs.in_unit + 1, giving(GROUP + 1),
            giving(3 * GROUP + 5)]
    assert GROUP < rs.num_output_samples(lens[-2]) <= GROUP + 1 + -(-rs.out_unit // rs.in_unit)
    assert 3 * GROUP < rs.num_output_samples(lens[-1]) < 4 * GROUP
    return lens


@functools.lru_cache(maxsize=None)
def batch(rates, dtype):
    """(buffer, offsets, lengths, expected outputs): utterances at odd offsets in a buffer whose gaps and two ends are
    poisoned -- NaN, or -32768 for int16, which no utterance holds -- so that a read past an utterance's bounds shows"""
    rs = resampler(rates)
    rng = np.random.default_rng(1000 * rates[0] + rates[1])
    lens = lengths_of(rs)
    utts, offs, pos = [], [], 5
    for n in lens:
        pos += 3  # a gap
        pos += pos % 2 == 0  # ... and an odd offset
        x = 3000 * rng.standard_normal(n)
        utts.append(np.rint(x).astype(np.int16) if dtype is np.int16 else x.astype(dtype))
        offs.append(pos)
        pos += n
    poison = -32768 if dtype is np.int16 else np.nan
    buf = np.full(pos + 7, poison, dtype=dtype)
    for x, o in zip(utts, offs):
        assert o % 2 == 1 and (dtype is not np.int16 or (x != poison).all())
        buf[o : o + len(x)] = x
    want = [model.resample(x, *rates, weights=rs.weights) for x in utts]
    for y in want:
        assert np.isfinite(y).all()
    for arr in [buf] + want:
        arr.flags.writeable = False
    return buf, np.asarray(offs, dtype=np.int64), np.asarray(lens, dtype=np.int64), want


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("rates", RATE_PAIRS, ids=rate_id)
def test_packed_batch_is_the_model_bit_for_bit(rates, dtype):
    import torch

    rs = resampler(rates)
    buf, offs, lens, want = batch(rates, dtype)
    d_buf = torch.from_numpy(buf.copy()).cuda()
    out, out_offs, out_lens = rs.apply_packed(d_buf, offs, lens)
    out_dtype = np.float64 if dtype is np.float64 else np.float32
    assert out.is_cuda and out.dim() == 1 and out.dtype == getattr(torch, np.dtype(out_dtype).name)
    assert isinstance(out_offs, np.ndarray) and out_offs.dtype == np.int64
    assert isinstance(out_lens, np.ndarray) and out_lens.dtype == np.int64
    assert out_lens.tolist() == [model.num_output_samples(int(n), *rates) for n in lens]
    assert out_offs.tolist() == (np.cumsum(out_lens) - out_lens).tolist() and out.numel() == int(out_lens.sum())
    assert d_buf.cpu().numpy().tobytes() == buf.tobytes()  # the input is untouched
    got = out.cpu().numpy()
    for b, y in enumerate(want):
        piece = got[out_offs[b] : out_offs[b] + out_lens[b]]
        assert model.same_bits(piece, y), (b, int(lens[b]))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("rates", RATE_PAIRS, ids=rate_id)
def test_apply_is_apply_packed_of_the_same_signal(rates, dtype):
    import torch

    rs = resampler(rates)
    buf, offs, lens, want = batch(rates, dtype)
    for b in range(len(lens)):
        x = buf[offs[b] : offs[b] + lens[b]]
        y = rs.apply(x)
        assert isinstance(y, np.ndarray) and model.same_bits(y, want[b]), b
        t = rs.apply(torch.from_numpy(x.copy()).cuda())
        assert t.is_cuda and model.same_bits(t.cpu().numpy(), want[b]), b
    assert (buf[offs[-1] : offs[-1] + lens[-1]] != 0).any()


def test_equal_rates_are_a_bit_copy():
    import torch

    rs = Resample(16000, 16000)
    rng = np.random.default_rng(3)
    for dtype in DTYPES:
        x = np.rint(3000 * rng.standard_normal(301)).astype(dtype)
        x[7] = 0
        if dtype is not np.int16:
            x[5], x[11], x[13] = np.nan, np.inf, -0.0
        want = x.astype(np.float32) if dtype is np.int16 else x
        y = rs.apply(x)
        assert y is not x and model.same_bits(y, want)
        t = torch.from_numpy(x.copy()).cuda()
        y = rs.apply(t)
        assert y.data_ptr() != t.data_ptr() and model.same_bits(y.cpu().numpy(), want)
        if dtype is not np.int16:
            assert rs.apply(t, in_place=True) is t
        buf = np.concatenate([x[:3], x, x[:5], x[:100], x[:1]])
        out, offs, lens = rs.apply_packed(torch.from_numpy(buf).cuda(), [3, 309, 409], [301, 100, 0])
        assert offs.tolist() == [0, 301, 401] and lens.tolist() == [301, 100, 0]
        assert model.same_bits(out.cpu().numpy(), np.concatenate([want, want[:100]]))


@pytest.mark.parametrize("rates", [(3, 2), (2, 3), (44100, 16000)], ids=rate_id)
def test_nan_and_infinity_reach_exactly_their_windows(rates):
    rs = resampler(rates)
    rng = np.random.default_rng(17)
    n = 4 * rs.in_unit + 10 * rs.max_taps
    for dtype in (np.float32, np.float64):
        x = (3000 * rng.standard_normal(n)).astype(dtype)
        x[n // 3], x[2 * n // 3] = np.nan, -np.inf
        want = model.resample(x, *rates, weights=rs.weights)
        marked = ~np.isfinite(want)
        got = rs.apply(x)
        assert ((~np.isfinite(got)) == marked).all() and model.same_bits(got, want)
        # the marked outputs are the two windows' worth and nothing else
        assert 2 <= marked.sum() <= 2 * (rs.max_taps * rs.out_unit // rs.in_unit + 2) < len(want) // 2
        assert np.isfinite(want[0]) and np.isfinite(want[-1])


def test_other_dtypes_are_widened_to_float64():
    import torch

    rs = resampler((3, 2))
    x = np.arange(-40, 60, dtype=np.int32) * 50
    want = model.resample(x.astype(np.float64), 3, 2, weights=rs.weights)
    assert model.same_bits(rs.apply(x), want)
    assert model.same_bits(rs.apply(torch.from_numpy(x).cuda()).cpu().numpy(), want)
    assert model.same_bits(rs.apply(x.astype(np.float16)), want)


def test_refusals():
    import torch

    rs = resampler((3, 2))
    t = torch.zeros(12, device="cuda")
    with pytest.raises(ValueError, match="in_place"):
        rs.apply(t, in_place=True)
    with pytest.raises(ValueError, match="1-D"):
        rs.apply(t.reshape(3, 4))
    with pytest.raises(ValueError, match="GPU"):
        rs.apply_packed(np.zeros(12, np.float32), [0], [12])
    with pytest.raises(ValueError, match="float32, float64 or int16"):
        rs.apply_packed(t.to(torch.int32), [0], [12])
    with pytest.raises(ValueError, match="one offset per length"):
        rs.apply_packed(t, [0, 1], [12])
    for offs, lens in (([1], [12]), ([-1], [3]), ([0], [-2])):
        with pytest.raises(ValueError, match="outside"):
            rs.apply_packed(t, offs, lens)
    out, offs, lens = rs.apply_packed(t, [], [])
    assert out.numel() == 0 and len(offs) == 0 and len(lens) == 0
    # a table just over the stated limit
    assert Resample(1, 80659).apply(np.ones(2, np.float32)).shape == (2 * 80659,)
    with pytest.raises(ValueError, match=str(Resample.MAX_TABLE)):
        Resample(1, 80663)
