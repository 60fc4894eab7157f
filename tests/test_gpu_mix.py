"""``pre.AddNoise`` on the device against the numpy model of its definition (tests/mix_model.py): the segment energy,
the bank's clip powers, the gains and the mix for all nine pairs of dtypes, bit for bit; the copies at gain zero; an
utterance's independence of its batch; the launch split above 65,535 utterances; ``apply`` for arrays and tensors.

All comparisons are equalities of bytes: the definition fixes every rounding, and the float64 division and square root
of the gain are correctly rounded on the device as in numpy (the precedent is ``SlidingCMVN``'s ``1.0 / sqrt(var)``)."""
import numpy as np
import pytest

from pydrobert_speech_amd.pre import AddNoise, NoisePlan, dither_keys
from tests import mix_model as mm

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.int16]
IDS = ["f32", "f64", "i16"]
ENERGY_LENGTHS = [0, 1, 63, 64, 65, 16383, 16384, 16385, 32769]
CLIP_LENGTHS = [1, 50, 257, 2500, 1000, 7]  # clip 4 is silent, clip 5 holds a NaN (float banks) or is silent (int16)
MIX_LENGTHS = [0, 1, 63, 64, 65, 257, 1000, 4097, 9000, 1000, 257, 3]  # the apply kernel's block is 4096 samples
MIX_GAPS = [1, 0, 3, 0, 2, 1, 1, 0, 5, 2, 3, 1, 2]  # before each utterance, and behind the last
#           clip of each utterance: length 1; shorter (20 wraps); equal; longer; ...
MIX_CLIPS = [0, 0, 1, 2, 3, 2, 1, 3, 1, 0, 3, 1]
SEEDS = list(range(200, 200 + len(MIX_LENGTHS)))


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def samples(rng, n, dtype, scale=3000.0):
    x = scale * rng.standard_normal(n)
    return np.rint(x).astype(np.int16) if np.dtype(dtype) == np.int16 else x.astype(dtype)


def packing(lengths, gaps):
    offsets = np.cumsum(np.asarray(gaps[:-1]) + np.asarray([0] + list(lengths[:-1])))
    total = int(offsets[-1] + lengths[-1] + gaps[-1])
    return offsets.astype(np.int64), total


def bank(dtype, seed=7):
    rng = np.random.default_rng(seed)
    clips = [samples(rng, n, dtype, scale=800.0) for n in CLIP_LENGTHS]
    clips[4][:] = 0
    if np.dtype(dtype) == np.int16:
        clips[5][:] = 0
    else:
        clips[5][3] = np.nan
    return clips


def gpu(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---- energy ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_energy_packed_has_the_models_bits(dtype):
    gaps = [1, 0, 3, 2, 1, 5, 0, 7, 1, 2]
    offsets, total = packing(ENERGY_LENGTHS, gaps)
    assert sum(int(o) % 2 for o in offsets) >= 3
    x = samples(np.random.default_rng(1), total, dtype)
    an = AddNoise([np.ones(4, dtype)])
    got = an.energy_packed(gpu(x), offsets, ENERGY_LENGTHS)
    assert got.is_cuda and tuple(got.shape) == (len(ENERGY_LENGTHS),)
    want = np.asarray([mm.energy(x[o : o + n]) for o, n in zip(offsets, ENERGY_LENGTHS)], dtype=np.float64)
    got = got.cpu().numpy()
    print(dtype.__name__, "energies differing from the model:", int((got.view(np.int64) != want.view(np.int64)).sum()))
    assert same(got, want) and got[0] == 0.0 and (got[1:] > 0).all()
    # a chunk's sum is not the plain sum: the order is the definition's (float64 samples use every bit)
    if dtype == np.float64:
        plain = np.asarray([np.sum(x[o : o + n] ** 2) for o, n in zip(offsets, ENERGY_LENGTHS)])
        assert np.allclose(got, plain, rtol=1e-12)
    # no utterance, and a NaN sample
    assert tuple(an.energy_packed(gpu(x), [], []).shape) == (0,)
    if dtype != np.int16:
        y = x.copy()
        y[offsets[5] + 16000] = np.nan
        e = an.energy_packed(gpu(y), offsets, ENERGY_LENGTHS).cpu().numpy()
        assert np.isnan(e[5]) and same(np.delete(e, 5), np.delete(want, 5))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_clip_power_has_the_models_bits(dtype):
    rng = np.random.default_rng(2)
    clips = [samples(rng, n, dtype, scale=500.0) for n in ENERGY_LENGTHS[1:]]
    an = AddNoise(clips)
    got = an.clip_power()
    assert got.is_cuda and got.dtype.is_floating_point and tuple(got.shape) == (len(clips),)
    assert an.clip_power() is got  # computed once per device
    assert same(got.cpu().numpy(), np.asarray([mm.power(c) for c in clips], dtype=np.float64))


# ---- gains and the mix ---------------------------------------------------------------------------------------------


def batch(x_dtype, z_dtype):
    """(AddNoise, clips, signal, offsets, plan as the package draws it with the test's clips forced)"""
    clips = bank(z_dtype)
    an = AddNoise(clips, snr_db=(0.0, 15.0))
    offsets, total = packing(MIX_LENGTHS, MIX_GAPS)
    assert sum(int(o) % 2 for o, n in zip(offsets, MIX_LENGTHS) if n) >= 3  # wide accesses meet unaligned spans
    assert len({int(o) % 4 for o in offsets}) == 4
    x = samples(np.random.default_rng(3), total, x_dtype)
    plan = an.plan(len(MIX_LENGTHS), seeds=SEEDS, clips=MIX_CLIPS)
    start = plan.start.copy()
    for b in (4, 6, 7):  # the last sample of the clip first
        start[b] = CLIP_LENGTHS[MIX_CLIPS[b]] - 1
    return an, clips, x, offsets, plan._replace(start=start)


def model_plan(plan):
    return {name: getattr(plan, name) for name in NoisePlan._fields}


@pytest.mark.parametrize("z_dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("x_dtype", DTYPES, ids=IDS)
def test_the_mix_and_the_gains_have_the_models_bits(x_dtype, z_dtype):
    an, clips, x, offsets, plan = batch(x_dtype, z_dtype)
    # the plan the package drew is the model's
    drawn = mm.plan(dither_keys(SEEDS), CLIP_LENGTHS, (0.0, 15.0), 1.0, clips=MIX_CLIPS)
    assert same(plan.ratio, drawn["ratio"]) and same(plan.clip, drawn["clip"])
    out, gains = an.apply_packed(gpu(x), offsets, MIX_LENGTHS, plan=plan, return_gains=True)
    assert out.is_cuda and gains.is_cuda and out.numel() == len(x)
    want, want_gains = mm.apply_packed(x, offsets, MIX_LENGTHS, clips, model_plan(plan))
    got_gains = gains.cpu().numpy()
    differing = int((got_gains.view(np.int64) != want_gains.view(np.int64)).sum())
    print("gains differing from the model:", differing, "of", len(want_gains))
    assert same(got_gains, want_gains)
    assert got_gains[0] == 0.0 and (got_gains[1:] > 0).all()  # (the empty utterance; every other one gets noise)
    got = out.cpu().numpy()
    assert got.dtype == mm.out_dtype(x_dtype)
    for b, (o, n) in enumerate(zip(offsets, MIX_LENGTHS)):
        assert same(got[o : o + n], want[o : o + n]), (b, n)
        if n:
            assert not same(got[o : o + n], x[o : o + n].astype(got.dtype))
    if x_dtype != np.int16:
        assert same(got, want)  # gaps between utterances keep their bytes
    # without a plan: seeds draw it, and the result is the model's too
    out2, gains2 = an.apply_packed(gpu(x), offsets, MIX_LENGTHS, seeds=SEEDS, return_gains=True)
    plan2 = mm.plan(dither_keys(SEEDS), CLIP_LENGTHS, (0.0, 15.0), 1.0)
    want2, want_gains2 = mm.apply_packed(x, offsets, MIX_LENGTHS, clips, plan2)
    assert same(gains2.cpu().numpy(), want_gains2)
    got2 = out2.cpu().numpy()
    for o, n in zip(offsets, MIX_LENGTHS):
        assert same(got2[o : o + n], want2[o : o + n])
    assert (want_gains2[1:] > 0).sum() >= 4  # (the silent clip and the NaN clip, where drawn, give gain zero)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gains_that_are_exactly_zero(dtype):
    clips = bank(dtype if dtype != np.int16 else np.float32)
    an = AddNoise(clips, snr_db=10.0)
    lengths = [100, 100, 100, 100, 0, 100, 100]
    offsets, total = packing(lengths, [1] * 8)
    x = samples(np.random.default_rng(4), total, dtype)
    x[offsets[0] : offsets[0] + 100] = 0  # a silent utterance
    if dtype != np.int16:
        x[offsets[6] + 17] = np.nan  # an utterance holding a NaN
    #        silent utt, silent clip, NaN clip, not applied, empty, a plain one, NaN utt
    clip_of = [1, 4, 5, 1, 1, 1, 1]
    plan = an.plan(7, seeds=range(7), clips=clip_of)
    plan = plan._replace(applied=np.array([True, True, True, False, True, True, True]))
    out, gains = an.apply_packed(gpu(x), offsets, lengths, plan=plan, return_gains=True)
    g = gains.cpu().numpy()
    zero = [0, 1, 2, 3, 4] + ([6] if dtype != np.int16 else [])
    assert g.dtype == np.float64 and all(g[b] == 0.0 and not np.signbit(g[b]) for b in zero), g
    assert g[5] > 0 and (dtype != np.int16 or g[6] > 0)
    want, want_g = mm.apply_packed(x, offsets, lengths, clips, model_plan(plan))
    assert same(g, want_g)
    got = out.cpu().numpy()
    T = mm.out_dtype(dtype)
    for b in zero:  # copied: the input's bytes (int16 widened)
        o, n = offsets[b], lengths[b]
        assert same(got[o : o + n], x[o : o + n].astype(T))
    assert same(got[offsets[5] : offsets[5] + 100], want[offsets[5] : offsets[5] + 100])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_a_copy_keeps_nan_payloads_and_signed_zeros(dtype):
    clips = bank(np.float32)
    an = AddNoise(clips, prob=0.0)
    lengths = [1000, 9, 4100]
    offsets, total = packing(lengths, [3, 1, 2, 1])
    x = samples(np.random.default_rng(5), total, dtype)
    words = x.view(np.uint32 if dtype == np.float32 else np.uint64)
    for o, n in zip(offsets, lengths):
        x[o] = -0.0
        words[o + n // 2] = 0x7FC01234 if dtype == np.float32 else 0x7FF8000000ABCDEF  # a NaN with a payload
        words[o + n - 1] = 0xFFC00001 if dtype == np.float32 else 0xFFF8000000000001
    out, gains = an.apply_packed(gpu(x), offsets, lengths, seeds=[1, 2, 3], return_gains=True)
    assert (gains.cpu().numpy() == 0.0).all()
    assert same(out.cpu().numpy(), x)
    # ... and where the utterances cover the buffer, which is then written whole by the kernel
    y = np.concatenate([x[o : o + n] for o, n in zip(offsets, lengths)])
    tight = np.cumsum([0] + lengths[:-1])
    assert same(an.apply_packed(gpu(y), tight, lengths, seeds=[1, 2, 3]).cpu().numpy(), y)
    mixed = AddNoise(clips[:4], snr_db=5.0).apply_packed(gpu(y), tight, lengths, seeds=[1, 2, 3]).cpu().numpy()
    plan = mm.plan(dither_keys([1, 2, 3]), CLIP_LENGTHS[:4], (5.0, 5.0), 1.0)
    want, want_g = mm.apply_packed(y, tight, lengths, clips[:4], plan)
    assert (want_g == 0.0).all()  # (every utterance holds a NaN: its power is NaN, so it is copied too)
    assert same(mixed, y)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_a_nan_sample_disturbs_no_other_utterance(dtype):
    an, clips, x, offsets, plan = batch(dtype, np.float32)
    clean = an.apply_packed(gpu(x), offsets, MIX_LENGTHS, plan=plan).cpu().numpy()
    y = x.copy()
    y[offsets[6] + 500] = np.nan
    y[offsets[8] + 8999] = np.inf
    dirty = an.apply_packed(gpu(y), offsets, MIX_LENGTHS, plan=plan).cpu().numpy()
    for b, (o, n) in enumerate(zip(offsets, MIX_LENGTHS)):
        if b not in (6, 8):
            assert same(dirty[o : o + n], clean[o : o + n]), b
    assert same(dirty[offsets[6] : offsets[6] + 1000], y[offsets[6] : offsets[6] + 1000])  # copied: its power is NaN
    keep = np.ones(len(x), dtype=bool)
    for b in (6, 8):
        keep[offsets[b] : offsets[b] + MIX_LENGTHS[b]] = False
    assert same(dirty[keep], clean[keep])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_an_utterance_is_the_same_alone_and_in_other_batches(dtype):
    clips = bank(np.int16)[:4]
    an = AddNoise(clips, snr_db=(-5.0, 5.0))
    rng = np.random.default_rng(6)
    utt = samples(rng, 5000, dtype)
    alone = an.apply_packed(gpu(utt), [0], [5000], seeds=[77]).cpu().numpy()
    assert not same(alone, utt.astype(alone.dtype))
    for index, lengths, gaps in ((2, [300, 0, 5000, 17], [3, 1, 2, 5, 1]), (5, [9, 4096, 1, 64, 70, 5000], [0, 1, 1, 1, 1, 1, 0])):
        offsets, total = packing(lengths, gaps)
        x = samples(rng, total, dtype)
        x[offsets[index] : offsets[index] + 5000] = utt
        seeds = list(range(len(lengths)))
        seeds[index] = 77
        got = an.apply_packed(gpu(x), offsets, lengths, seeds=seeds).cpu().numpy()
        assert same(got[offsets[index] : offsets[index] + 5000], alone), index


def test_one_plan_on_two_views_gives_the_same_noise_segment():
    clips = bank(np.float64)[:4]
    an = AddNoise(clips, snr_db=(0.0, 10.0))
    lengths = [1000, 257, 4097]
    offsets, total = packing(lengths, [1, 2, 3, 1])
    rng = np.random.default_rng(8)
    views = [samples(rng, total, np.float64), samples(rng, total, np.float64, scale=10.0)]
    plan = an.plan(3, seeds=[4, 5, 6])
    segments = []
    for x in views:
        out, gains = an.apply_packed(gpu(x), offsets, lengths, plan=plan, return_gains=True)
        out, g = out.cpu().numpy(), gains.cpu().numpy()
        segments.append([(out[o : o + n] - x[o : o + n]) / g[b] for b, (o, n) in enumerate(zip(offsets, lengths))])
    for b, n in enumerate(lengths):
        clip = clips[plan.clip[b]]
        want = clip[(plan.start[b] + np.arange(n)) % len(clip)]
        for seg in segments:
            assert np.allclose(seg[b], want, rtol=1e-9, atol=1e-9 * np.abs(clip).max())


def test_more_utterances_than_one_launch_takes():
    """65,537 utterances of 3 samples: the apply kernel's launches split at 65,535; against the definition, taken for
    all rows at once"""
    B, n = 65537, 3
    rng = np.random.default_rng(9)
    clips = [samples(rng, L, np.float32, scale=100.0) for L in (1, 2, 5, 50)]
    an = AddNoise(clips, snr_db=(0.0, 20.0), prob=0.9)
    x = samples(rng, B * n, np.float32)
    offsets = np.arange(B, dtype=np.int64) * n
    plan = an.plan(B, seeds=range(B))
    spot = [0, 1, 65534, 65535, 65536]
    check = mm.plan(dither_keys(spot), [1, 2, 5, 50], (0.0, 20.0), 0.9)
    for name in NoisePlan._fields:
        assert same(getattr(plan, name)[spot], check[name]), name
    out, gains = an.apply_packed(gpu(x), offsets, np.full(B, n), plan=plan, return_gains=True)
    X = x.reshape(B, n)
    ps = mm.energy_rows(X) / np.float64(n)
    pn = np.asarray([mm.power(c) for c in clips])[plan.clip]
    with np.errstate(all="ignore"):
        g = np.where(plan.applied & (ps > 0) & (pn > 0), np.sqrt(ps / (pn * plan.ratio)), 0.0)
    assert same(gains.cpu().numpy(), g) and 0.05 < (g == 0).mean() < 0.15
    L = an.clip_lengths[plan.clip]
    z = an.bank[an.clip_offsets[plan.clip][:, None] + (plan.start[:, None] + np.arange(n)[None, :]) % L[:, None]]
    want = (X.astype(np.float64) + g[:, None] * z.astype(np.float64)).astype(np.float32)
    want[g == 0] = X[g == 0]
    assert same(out.cpu().numpy(), want.reshape(-1))


# ---- apply -----------------------------------------------------------------------------------------------------------


def test_apply_is_apply_packed_of_the_same_rows_and_seeds():
    import torch

    clips = bank(np.float32)[:4]
    rng = np.random.default_rng(10)
    one = samples(rng, 3000, np.float32)
    # 1-D: one utterance
    want = AddNoise(clips, seed=5).apply_packed(gpu(one), [0], [3000]).cpu().numpy()
    got = AddNoise(clips, seed=5).apply(one)
    assert isinstance(got, np.ndarray) and same(got, want) and not same(got, one)
    got = AddNoise(clips, seed=5).apply(gpu(one))
    assert got.is_cuda and same(got.cpu().numpy(), want)
    # 2-D: every vector along the axis an utterance of its own draw, in C order
    two = samples(rng, 6 * 700, np.float64).reshape(6, 700)
    rows = AddNoise(clips, seed=6).apply_packed(gpu(two.reshape(-1)), np.arange(6) * 700, [700] * 6).cpu().numpy()
    for axis in (None, -1, 1):
        assert same(AddNoise(clips, seed=6).apply(two, axis=axis), rows.reshape(6, 700)), axis
        assert same(AddNoise(clips, seed=6).apply(gpu(two), axis=axis).cpu().numpy(), rows.reshape(6, 700)), axis
    for axis in (0, -2):
        assert same(AddNoise(clips, seed=6).apply(np.ascontiguousarray(two.T), axis=axis), rows.reshape(6, 700).T), axis
        got = AddNoise(clips, seed=6).apply(gpu(two.T), axis=axis)
        assert tuple(got.shape) == (700, 6) and same(got.cpu().numpy(), rows.reshape(6, 700).T), axis
    # the sequence advances once per vector: a second call draws anew
    an = AddNoise(clips, seed=6)
    first, second = an.apply(two), an.apply(two)
    assert same(first, rows.reshape(6, 700)) and not same(first, second)
    # in place: the array, or the tensor, itself
    arr = two.copy()
    assert AddNoise(clips, seed=6).apply(arr, in_place=True) is arr and same(arr, rows.reshape(6, 700))
    t = gpu(two)
    assert AddNoise(clips, seed=6).apply(t, in_place=True) is t and same(t.cpu().numpy(), rows.reshape(6, 700))
    t = gpu(two)
    assert AddNoise(clips, seed=6).apply(t) is not t and same(t.cpu().numpy(), two)
    # another dtype goes through float64 and comes back in its own
    pcm = samples(rng, 500, np.int16)
    got = AddNoise(clips, seed=7).apply(pcm)
    wide = AddNoise(clips, seed=7).apply(pcm.astype(np.float64))
    assert got.dtype == np.int16 and same(got, wide.astype(np.int16))
    assert tuple(AddNoise(clips).apply(np.zeros((0,), np.float32)).shape) == (0,)
    assert isinstance(AddNoise(clips).apply(torch.zeros((3, 0), device="cuda")), torch.Tensor)
