"""``resample_packed_kernel`` and ``multistream_resample_kernel`` (csrc/resample.hip) at the launch shapes the first
tests do not reach, against ``tests/resample_model.py`` bit for bit.

Offline, through ``pds_resample_packed_*`` with buffers of the test's own: windows of every length modulo the four
taps a group loads, windows shorter than one group and of 291 and 581 taps, phases of different lengths within one
wave, utterance lengths around the one at which the unclamped form of the sum first applies, and 70,000 utterances of
0..3 samples with and without one of 700 among them.  Streaming, through ``ResampleBatch``: histories of 290 and 580
samples, which are rewritten in two and three passes of a block's width, with chunks around the lengths at which a
sample crosses from one pass to another; 300 streams in one tick, each with more outputs than a block has lanes.
What a kernel must not read is NaN, or -32768 for int16 (gaps between utterances, the history of a stream before its
first sample); what it must not write is random and compared afterwards."""
import functools

import numpy as np
import pytest

from pydrobert_speech_amd import _native
from pydrobert_speech_amd.multistream_resample import ResampleBatch
from pydrobert_speech_amd.pre import Resample
from tests import resample_model as model
from tests.test_gpu_resample import GROUP, lengths_of

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.int16]
AHEAD = 4  # taps a group loads (RS_AHEAD of csrc/resample.hip)
# (from_rate, to_rate, num_zeros) -> (fewest, most) taps of a phase
TAP_SHAPES = {
    (5, 2, 3): (15, 16),  # whole groups: the tap index is never clamped
    (3, 2, 5): (15, 16),
    (4, 3, 5): (13, 14),
    (1, 2, 1): (2, 3),  # less than one group
    (24, 1, 6): (291, 291),
    (48, 1, 6): (581, 581),
    (1, 24, 6): (12, 13),  # 24 phases: a wave holds lanes of both lengths
}


def poison_of(dtype):
    return -32768 if dtype is np.int16 else np.nan


def signal(rng, n, dtype):
    x = 3000 * rng.standard_normal(n)
    return np.clip(np.rint(x), -32767, 32767).astype(np.int16) if dtype is np.int16 else x.astype(dtype)


def out_dtype_of(dtype):
    return np.float64 if dtype is np.float64 else np.float32


@functools.lru_cache(maxsize=None)
def resampler(shape):
    return Resample(shape[0], shape[1], num_zeros=shape[2])


def first_group_length(rs):
    """the shortest utterance in which an output's window, rounded up to whole groups, can lie inside"""
    return -(-rs.max_taps // AHEAD) * AHEAD


def launch_packed(rs, buf, offs, lens, out_offs, before):
    """``pds_resample_packed_*`` of the utterances ``buf[offs[b] : offs[b] + lens[b]]`` to ``out_offs[b]`` of a copy of
    `before`; returns that copy"""
    import torch

    lib = _native.stages_lib()
    fn = {"float32": lib.pds_resample_packed_f32, "float64": lib.pds_resample_packed_f64,
          "int16": lib.pds_resample_packed_i16_f32}[buf.dtype.name]
    out_lens = np.asarray(rs.num_output_samples(lens), dtype=np.int64).reshape(-1)
    assert (offs >= 0).all() and int((offs + lens).max()) <= len(buf)
    assert (out_offs >= 0).all() and int((out_offs + out_lens).max()) <= len(before)
    assert before.dtype == out_dtype_of(buf.dtype.type)
    d_buf, d_out = torch.from_numpy(buf.copy()).cuda(), torch.from_numpy(before).cuda()  # (buf may be read-only)
    d_meta = torch.from_numpy(np.stack([offs, lens, out_offs]).astype(np.int64)).cuda()
    first, ntaps, weights = rs._tables(d_buf.device)
    rc = fn(d_buf.data_ptr(), d_meta[0].data_ptr(), d_meta[1].data_ptr(), d_meta[2].data_ptr(), len(lens),
            int(lens.max()), rs.in_unit, rs.out_unit, rs.max_taps, first.data_ptr(), ntaps.data_ptr(),
            weights.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _native.check_stages(rc, "pds_resample_packed")
    got = d_out.cpu().numpy()
    assert d_buf.cpu().numpy().tobytes() == buf.tobytes()  # (the input is left alone)
    return got


def assert_same_bytes(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        ints = np.uint32 if got.dtype == np.float32 else np.uint64
        bad = np.flatnonzero(got.view(ints) != want.view(ints))
        raise AssertionError((what, int(bad[0]), got[bad[0]], want[bad[0]], len(bad)))


# ---- offline ---------------------------------------------------------------------------------------------------------


def test_the_tap_shapes_are_what_they_are_there_for():
    # (no device work)
    for shape, (lo, hi) in TAP_SHAPES.items():
        rs = resampler(shape)
        assert (int(rs.ntaps.min()), int(rs.ntaps.max()), rs.max_taps) == (lo, hi, hi), shape
        t = model.table(shape[0], shape[1], shape[2])
        assert (t[0], t[1]) == (rs.in_unit, rs.out_unit) and np.array_equal(t[3], rs.ntaps)
    taps = [hi for _, hi in TAP_SHAPES.values()]
    assert {t % AHEAD for t in taps} == {0, 1, 2, 3} and min(taps) < AHEAD
    rs = resampler((1, 24, 6))
    assert rs.out_unit == 24 and len(set(rs.ntaps[:24].tolist())) == 2  # (24 adjacent lanes: both lengths)


def lengths_for(rs):
    g = first_group_length(rs)
    return lengths_of(rs) + [g - 1, g, g + 1, g + rs.in_unit]


@functools.lru_cache(maxsize=None)
def batch(shape, dtype):
    """``(buffer, offsets, lengths, expected outputs)`` like ``tests.test_gpu_resample.batch``: utterances at odd
    offsets in a buffer whose gaps and two ends are poisoned"""
    rs = resampler(shape)
    rng = np.random.default_rng(1000 * shape[0] + 10 * shape[1] + shape[2])
    lens = lengths_for(rs)
    utts, offs, pos = [], [], 5
    for n in lens:
        pos += 3  # a gap
        pos += pos % 2 == 0  # ... and an odd offset
        utts.append(signal(rng, n, dtype))
        offs.append(pos)
        pos += n
    buf = np.full(pos + 7, poison_of(dtype), dtype=dtype)
    for x, o in zip(utts, offs):
        assert o % 2 == 1 and (dtype is not np.int16 or (x != poison_of(dtype)).all())
        buf[o : o + len(x)] = x
    want = [model.resample(x, shape[0], shape[1], num_zeros=shape[2], weights=rs.weights) for x in utts]
    for arr in [buf] + want:
        assert arr is buf or np.isfinite(arr).all()
        arr.flags.writeable = False
    return buf, np.asarray(offs, dtype=np.int64), np.asarray(lens, dtype=np.int64), want


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", list(TAP_SHAPES), ids=lambda s: f"{s[0]}to{s[1]}z{s[2]}")
def test_tap_groups(shape, dtype):
    rs = resampler(shape)
    buf, offs, lens, want = batch(shape, dtype)
    g = first_group_length(rs)
    assert g % AHEAD == 0 and 0 <= g - rs.max_taps < AHEAD and {g - 1, g, g + 1, g + rs.in_unit} <= set(lens.tolist())
    rng = np.random.default_rng(5)
    out_lens = np.asarray([len(y) for y in want], dtype=np.int64)
    assert out_lens.tolist() == [model.num_output_samples(int(n), shape[0], shape[1]) for n in lens]
    out_offs = 3 + np.cumsum(out_lens + 2) - (out_lens + 2)  # (two sentinels between the utterances' outputs)
    before = rng.standard_normal(int(out_offs[-1] + out_lens[-1] + 3)).astype(out_dtype_of(dtype))
    expect = before.copy()
    for y, o in zip(want, out_offs):
        expect[o : o + len(y)] = y
    assert out_lens.max() > 3 * GROUP
    assert_same_bytes(launch_packed(rs, buf, offs, lens, out_offs, before), expect, shape)


@pytest.mark.parametrize("long_one", [False, True], ids=["short", "one_of_700"])
def test_seventy_thousand_utterances(long_one):
    """1 -> 2, float32, lengths 0, 1, 2, 3, 0, ..: one block per utterance; with one utterance of 700 samples among
    them six, of which all but the first return at once for every other utterance.

    The expected outputs come from ONE call of the model: the utterances laid out in a long signal of zeros,
    ``max_taps`` apart.  With ``in_unit == 1`` output ``2 (P + i) + p`` of the long signal has the window of output
    ``2 i + p`` of the utterance at P; the taps that fall outside the utterance meet zeros there, and a product of
    ``+-0.0`` added to a sum that started at +0.0 leaves its bits (no sample is zero, so no sum is -0.0).  Checked
    against the model of single utterances for every 500th and the long one."""
    B, dtype = 70000, np.float32
    rs = Resample(1, 2)
    assert (rs.in_unit, rs.out_unit, rs.max_taps) == (1, 2, 13)
    rng = np.random.default_rng(71 + long_one)
    lens = np.arange(B, dtype=np.int64) % 4
    if long_one:
        lens[B // 2] = 700
    assert -(-int(rs.num_output_samples(int(lens.max()))) // GROUP) == (6 if long_one else 1)
    # the device buffer: odd offsets, poisoned gaps
    offs = 5 + np.cumsum(lens + 3) - (lens + 3)
    buf = np.full(int(offs[-1] + lens[-1] + 7), np.nan, dtype=dtype)
    # the model's signal: the same utterances in zeros
    far = 5 + np.cumsum(lens + rs.max_taps) - (lens + rs.max_taps)
    spread = np.zeros(int(far[-1] + lens[-1] + rs.max_taps), dtype=dtype)
    total = int(lens.sum())
    which = np.repeat(np.arange(B), lens)
    within = np.arange(total) - np.repeat(np.cumsum(lens) - lens, lens)
    x = signal(rng, total, dtype)
    x[x == 0] = 1.0
    x[within == 0] = (1000 + rng.permutation(B)[: int((lens > 0).sum())]).astype(dtype)  # every utterance differs
    buf[offs[which] + within] = x
    spread[far[which] + within] = x
    long_want = model.resample(spread, 1, 2, weights=rs.weights)
    out_lens = 2 * lens
    out_offs = 3 + np.cumsum(out_lens + 1) - (out_lens + 1)  # (a sentinel between the utterances' outputs)
    before = rng.standard_normal(int(out_offs[-1] + out_lens[-1] + 3)).astype(np.float32)
    expect = before.copy()
    owhich = np.repeat(np.arange(B), out_lens)
    owithin = np.arange(int(out_lens.sum())) - np.repeat(np.cumsum(out_lens) - out_lens, out_lens)
    expect[out_offs[owhich] + owithin] = long_want[2 * far[owhich] + owithin]
    for b in sorted(set(range(1, B, 500)) | {B // 2, B - 1}):
        single = model.resample(buf[offs[b] : offs[b] + lens[b]], 1, 2, weights=rs.weights)
        assert model.same_bits(expect[out_offs[b] : out_offs[b] + out_lens[b]], single), b
    assert_same_bytes(launch_packed(rs, buf, offs, lens, out_offs, before), expect, long_one)


# ---- streaming -------------------------------------------------------------------------------------------------------


def poison_history(rb, sids, dtype):
    rb._hist[sids] = poison_of(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("rates", [(24, 1), (48, 1)], ids=["24to1", "48to1"])
def test_histories_of_more_than_one_pass(rates, dtype):
    """H = 290 and 580: the history is rewritten in 2 and 3 passes of 256 slots.  A chunk of c < H samples moves old
    slot i + c to slot i -- across a pass boundary where ``i < 256 k <= i + c``; the lengths are those around H - 256
    and H, none, one, and more than the whole history."""
    rs = Resample(*rates)
    H = rs.max_taps - 1
    assert H == {24: 290, 48: 580}[rates[0]] and -(-H // GROUP) == {24: 2, 48: 3}[rates[0]]
    sizes = [0, 1, H - 257, H - 256, H - 255, H - 1, H, H + 1, 2 * H + 3]
    sids = [5, 0, 3, 2]
    rng = np.random.default_rng(rates[0] + 3 * DTYPES.index(dtype))
    with ResampleBatch(rs, 6, dtype) as rb:
        for life in range(2):
            cuts = [rng.permutation(sizes).tolist() for _ in sids]  # every stream takes every length, in its own order
            sigs = [signal(rng, sum(c) + life, dtype) for c in cuts]
            for c in cuts:
                c[-1] += life
            want = [model.resample(x, *rates, weights=rs.weights) for x in sigs]
            poison_history(rb, sids, dtype)  # (a slot "below sample 0" must not be read)
            pos, outs = [0] * len(sids), [[] for _ in sids]
            for tick in range(len(sizes)):
                order = rng.permutation(len(sids)).tolist()
                chunks = [sigs[i][pos[i] : pos[i] + cuts[i][tick]] for i in order]
                for i, y in zip(order, rb.resample_chunks([sids[i] for i in order], chunks)):
                    pos[i] += cuts[i][tick]
                    outs[i].append(y)
                    assert sum(map(len, outs[i])) == model.due(pos[i], rs.in_unit, rs.out_unit, rs.first, rs.ntaps)
            for i, y in enumerate(rb.finalize(sids)):
                outs[i].append(y)
                assert pos[i] == len(sigs[i])
                got = np.concatenate(outs[i])
                assert np.isfinite(want[i]).all() and len(want[i]) > 20
                assert model.same_bits(got, want[i]), (life, i, cuts[i])


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_three_hundred_streams_with_more_outputs_than_a_block(dtype):
    """1 -> 24 with chunks of 20 samples: 480 outputs per stream and tick, two strides of a block's 256 lanes"""
    rs = Resample(1, 24)
    n, ticks, chunk = 300, 3, 20
    rng = np.random.default_rng(24 + DTYPES.index(dtype))
    sigs = [signal(rng, ticks * chunk, dtype) for _ in range(n)]
    want = [model.resample(x, 1, 24, weights=rs.weights) for x in sigs]
    outs = [[] for _ in range(n)]
    with ResampleBatch(rs, n, dtype) as rb:
        poison_history(rb, list(range(n)), dtype)
        for tick in range(ticks):
            order = rng.permutation(n)
            assert n - 1 in order and not (order == np.arange(n)).all()
            chunks = [sigs[i][tick * chunk : (tick + 1) * chunk] for i in order]
            got = rb.resample_chunks(order.tolist(), chunks)  # (stream i runs on id i)
            for i, y in zip(order.tolist(), got):
                outs[i].append(y)
            if tick:
                assert {len(y) for y in got} == {chunk * 24} and chunk * 24 > GROUP
        for i, y in enumerate(rb.finalize(list(range(n)))):
            outs[i].append(y)
    for i in range(n):
        assert model.same_bits(np.concatenate(outs[i]), want[i]), i
