"""``post.SpecAugment`` on the GPU against the numpy model of its definition (tests/specaug_model.py).

Every comparison is exact: the plan as integers, the rows byte for byte (NaN payloads and the signs of zeros
included).  Only where the interpolation itself computes a NaN (inf - inf) is a NaN all that is asked, at the places
the model has one.  Shapes: utterance lengths around the warp's threshold ``2 W + 3``, a wave and the apply kernel's
row tile (imported, not restated), widths of one column and around 64 and 256 lanes, ragged batches with empty
utterances, strided rows, 2-D and 3-D, arrays and GPU tensors.

The splitting of a batch that needs more blocks than one launch holds is not tested here: the limit is 2^31 - 1 blocks,
and the smallest batch above it (2^31 utterances) does not fit a test.  tests/test_specaug_host.py tests the split
over a fake native layer with a smaller limit."""
import functools

import numpy as np
import pytest

from pydrobert_speech_amd.post import _SPECAUG_TILE as R
from pydrobert_speech_amd.post import SpecAugment
from tests import specaug_model as sm

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
WIDTHS = (1, 40, 64, 65, 257)
TILE_LENGTHS = (1, R - 1, R, R + 1, 2 * R + 1)


def gpu(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def hard_batch(lens, C, dtype, seed=0):
    """utterances of NaNs with distinct payloads, both zeros, both infinities and denormals among normals; computed
    once, left unchanged"""
    rng = np.random.default_rng(1000 * seed + 7 * sum(lens) + C)
    utts = tuple(sm.special_values(rng, (T, C), dtype) for T in lens)
    big = np.concatenate(utts)
    if big.size > 200:
        assert np.isnan(big).any() and np.isinf(big).any() and (big == 0).any()
        assert (np.signbit(big) & (big == 0)).any() and ((big != 0) & (np.abs(big) < np.finfo(dtype).tiny)).any()
    return utts


def finite_batch(lens, C, dtype, seed=0):
    rng = np.random.default_rng(2000 * seed + 11 * sum(lens) + C)
    return [(rng.standard_normal((T, C)) * 100).astype(dtype) for T in lens]


# ---- the plan -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("W", [0, 1, 5])
def test_plan_rows_equals_the_model(W):
    lengths = [0, 1, 2, 3, 2 * W + 2, 2 * W + 3, 2 * W + 4, 63, 64, 65, 257, 1000]
    ragged = [257, 0, 2 * W + 3, 0, 0, 1000, 3]  # B = 7, empty utterances between full ones
    seen_warp = seen_none = False
    for C in (1, 13, 40, 64, 65):
        for masks in (0, 1, 16):
            for ratio in (1.0, 0.2, 1e-3):
                for freq_width in (max(C // 2, 1) if C > 1 else 0, C + 9):  # below and above C
                    post = SpecAugment(masks, freq_width, masks, 50, ratio, W, seed=C + masks)
                    for lens in (lengths, ragged):
                        seeds = [1000 * C + 10 * masks + b for b in range(len(lens))]
                        got = post.plan_rows(lens, C, seeds=seeds)
                        assert got.is_cuda and tuple(got.shape) == (len(lens), 2 + 4 * masks)
                        want = sm.plan_model(post, lens, C, sm.dither_keys(seeds))
                        assert (got.cpu().numpy() == want).all(), (C, masks, ratio, freq_width)
                        seen_warp |= bool((want[:, 0] >= 1).any())
                        seen_none |= bool((want[np.asarray(lens) > 0, 0] < 0).any())
    assert seen_warp == (W > 0) and seen_none
    # B = 1, every length by itself, from the object's own sequence
    post, twin = SpecAugment(2, 10, 2, 50, 1.0, W, seed=3), SpecAugment(2, 10, 2, 50, 1.0, W, seed=3)
    for T in lengths:
        twin._seed = key = sm._next_key(twin._seed)
        got = post.plan_rows([T], 40).cpu().numpy()
        assert (got == sm.plan_model(post, [T], 40, [key])).all(), T
    assert tuple(post.plan_rows([], 40).shape) == (0, 10)


# ---- masks only -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_masks_only_byte_for_byte(dtype, C):
    import torch

    lens = TILE_LENGTHS + (0, 3 * R)
    utts = hard_batch(lens, C, dtype)
    rows = offsets(lens)
    seeds = list(range(40, 40 + len(lens)))
    filled = 0
    for fill in (0.0, float("nan"), -float("inf"), 1.0 + 2.0 ** -30):  # (the last rounds to float32 once)
        post = SpecAugment(2, 10, 2, 50, 1.0, 0, fill, seed=0)
        want, plan = sm.augment_model(post, utts, sm.dither_keys(seeds))
        filled += sum(int(sm.masked_model(post, u.shape, plan[b]).sum()) for b, u in enumerate(utts))
        feats = gpu(np.concatenate(utts))
        out = post.apply_rows(feats, rows, seeds=seeds)
        assert out.is_cuda and out.dtype == feats.dtype and sm.same_bytes(out.cpu().numpy(), np.concatenate(want))
        assert sm.same_bytes(feats.cpu().numpy(), np.concatenate(utts))  # the input is left as it was
        # every utterance alone gives what it gives in the batch
        for b, u in enumerate(utts):
            alone = post.apply_rows(gpu(u), [0, len(u)], seeds=seeds[b:b + 1])
            assert sm.same_bytes(alone.cpu().numpy(), want[b]), (b, fill)
        # in place
        same = post.apply_rows(feats, rows, seeds=seeds, out=feats)
        assert same is feats and sm.same_bytes(feats.cpu().numpy(), np.concatenate(want))
    assert filled > 0
    # a column slice of a wider tensor, into a column slice of another: rows wider than C, the other columns untouched
    post = SpecAugment(2, 10, 2, 50, 1.0, 0, -3.0, seed=0)
    want, _ = sm.augment_model(post, utts, sm.dither_keys(seeds))
    wide = np.full((rows[-1] + 3, C + 5), 7.0, dtype=dtype)
    wide[2:-1, 3:3 + C] = np.concatenate(utts)
    src, dst = gpu(wide), gpu(np.full((rows[-1] + 3, C + 2), 9.0, dtype=dtype))
    got = post.apply_rows(src[:, 3:3 + C], rows + 2, seeds=seeds, out=dst[:, 1:1 + C])
    assert got.data_ptr() == dst[:, 1:].data_ptr()
    expect = np.full((rows[-1] + 3, C + 2), 9.0, dtype=dtype)
    expect[2:-1, 1:1 + C] = np.concatenate(want)
    assert sm.same_bytes(dst.cpu().numpy(), expect) and sm.same_bytes(src.cpu().numpy(), wide)
    inplace = src[:, 3:3 + C]
    post.apply_rows(inplace, rows + 2, seeds=seeds, out=inplace)
    wide[2:-1, 3:3 + C] = np.concatenate(want)
    assert sm.same_bytes(src.cpu().numpy(), wide)
    assert isinstance(out, torch.Tensor)


# ---- the mean -------------------------------------------------------------------------------------------------------

MEAN_SHAPES = ((1, 1), (1, 63), (63, 1), (7, 9), (64, 1), (8, 8), (1, 64), (65, 1), (5, 13), (4097, 1), (17, 241),
               (1, 4097), (1000, 40))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_mean_rows_equals_the_models_bits(dtype):
    rng = np.random.default_rng(5)
    post = SpecAugment(fill="mean", seed=0)
    for T, C in MEAN_SHAPES:
        x = (rng.standard_normal((T, C)) * 10.0 ** rng.integers(-3, 4, (T, C))).astype(dtype)
        got = post.mean_rows(gpu(x), [0, T])
        assert got.is_cuda and got.dtype.is_floating_point and tuple(got.shape) == (1,)
        got = got.cpu().numpy()
        assert got.dtype == np.float64 and got[0].tobytes() == sm.mean_model(x).tobytes(), (T, C)
        wide = gpu(np.pad(x, ((1, 2), (2, 3))))  # strided rows, an offset
        assert post.mean_rows(wide[:, 2:2 + C], [1, 1 + T]).cpu().numpy()[0].tobytes() == sm.mean_model(x).tobytes()
    # a ragged batch: an utterance with a NaN, an all-zero one, an empty one
    C = 40
    utts = [(rng.standard_normal((T, C)) * 50).astype(dtype) for T in (70, 3, 33, 0, 129)]
    utts[1][2, 5] = np.nan
    utts[2][:] = 0
    got = post.mean_rows(gpu(np.concatenate(utts)), offsets([len(u) for u in utts])).cpu().numpy()
    assert np.isnan(got[1]) and np.isnan(got[3]) and got[2].tobytes() == np.float64(0.0).tobytes()
    for b in (0, 2, 4):
        assert got[b].tobytes() == sm.mean_model(utts[b]).tobytes(), b


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_fill_mean_holds_the_mean_rounded_once(dtype):
    rng = np.random.default_rng(6)
    lens, C = (70, 0, 33, 129, 2), 40
    utts = [(rng.standard_normal((T, C)) * 50 + 3).astype(dtype) for T in lens]
    seeds = [3, 4, 5, 6, 7]
    post = SpecAugment(2, 10, 2, 50, 1.0, 0, "mean", seed=0)
    want, plan = sm.augment_model(post, utts, sm.dither_keys(seeds))
    got = post.apply_rows(gpu(np.concatenate(utts)), offsets(lens), seeds=seeds).cpu().numpy()
    assert sm.same_bytes(got, np.concatenate(want))
    rows = offsets(lens)
    for b, u in enumerate(utts):
        if not len(u):
            continue
        masked = sm.masked_model(post, u.shape, plan[b])
        assert masked.any() and not masked.all(), b  # the model masks something in every utterance relied on
        value = np.float64(sm.mean_model(u)).astype(dtype)
        assert (got[rows[b]:rows[b + 1]][masked].view(value.dtype) == value).all()
        assert sm.same_bytes(got[rows[b]:rows[b + 1]][masked], np.full(int(masked.sum()), value, dtype=dtype))


# ---- the warp -------------------------------------------------------------------------------------------------------


def with_infinities(x, rng):
    x = x.copy()
    pick = rng.random(x.shape)
    x[pick < 0.1] = np.inf
    x[pick > 0.9] = -np.inf
    return x


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_hand_written_plans_at_the_extremes(dtype):
    import torch

    rng = np.random.default_rng(8)
    post = SpecAugment(1, 10, 1, 50, 1.0, 5, 0.5, seed=0)  # plan rows of w0, w1, (f0, f), (t0, t)
    cases = []
    for T in (3, 13, R, R + 1, 2 * R + 1, 100):
        mid = (T - 1) // 2
        cases += [(T, [mid, 1, 0, 0, 0, 0]), (T, [mid, T - 2, 0, 0, 0, 0]), (T, [1, T - 2, 0, 0, 0, 0]),
                  (T, [T - 2, 1, 0, 0, 0, 0]), (T, [mid, mid, 0, 0, 0, 0])]
    cases += [(13, [6, 6, 0, 0, 0, 0]),  # T = 2 W + 3: the one centre the draw admits
              (40, [20, 17, 3, 9, 15, 6]),  # a time mask and a frequency mask across the centre
              (40, [11, 30, 0, 40, 0, 0]),  # every column masked
              (40, [0, 5, 0, 0, 0, 0]), (40, [5, 39, 0, 0, 0, 0]), (40, [-1, -1, 2, 3, 38, 2])]  # no warp
    mixed_somewhere = nan_somewhere = False
    for C in (1, 40, 65):
        lens = [T for T, _ in cases]
        plan = np.asarray([p for _, p in cases], dtype=np.int64)
        plan[:, 2] = np.minimum(plan[:, 2], C - 1)
        plan[:, 3] = np.minimum(plan[:, 3], C - plan[:, 2])
        finite = finite_batch(lens, C, dtype)
        for utts, exact in ((finite, True), ([with_infinities(u, rng) for u in finite], False)):
            out = post.apply_rows(gpu(np.concatenate(utts)), offsets(lens), plan=gpu(plan)).cpu().numpy()
            rows = offsets(lens)
            for b, u in enumerate(utts):
                want = sm.apply_model(post, u, plan[b])
                got = out[rows[b]:rows[b + 1]]
                # NaNs where the model has them (inf - inf), every other element bit for bit
                assert sm.same_bits(got, want), (C, b, cases[b])
                if exact:
                    assert np.isfinite(want).all() and sm.same_bytes(got, want), (C, b, cases[b])
                    mixed_somewhere |= not sm.same_bytes(want, u)
                else:
                    nan_somewhere |= bool(np.isnan(want).any())
                if plan[b, 0] == plan[b, 1] and plan[b, 5] == 0 and plan[b, 3] == 0:
                    assert sm.same_bytes(got, u)  # the identity: every a == 0
    assert mixed_somewhere and nan_somewhere
    # the identity copies byte for byte, NaN payloads included
    hard = hard_batch((R + 3,), 65, dtype)[0]
    ident = gpu(np.asarray([[9, 9, 0, 0, 0, 0]], dtype=np.int64))
    assert sm.same_bytes(post.apply_rows(gpu(hard), [0, R + 3], plan=ident).cpu().numpy(), hard)
    assert isinstance(ident, torch.Tensor)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_drawn_warps_equal_the_model(dtype):
    rng = np.random.default_rng(9)
    for W, C in ((1, 40), (5, 65), (5, 1), (40, 257)):
        lens = (2 * W + 2, 2 * W + 3, 2 * W + 4, 0, R, 2 * R + 1, 300)
        seeds = list(range(70, 70 + len(lens)))
        for fill in (0.0, "mean"):
            post = SpecAugment(2, 10, 2, 50, 1.0, W, fill, seed=0)
            finite = finite_batch(lens, C, dtype, seed=W)
            want, plan = sm.augment_model(post, finite, sm.dither_keys(seeds))
            assert (plan[1:3, 0] >= 1).all() and plan[0, 0] == -1
            assert any(not sm.same_bytes(w, u) for w, u in zip(want, finite))
            got = post.apply_rows(gpu(np.concatenate(finite)), offsets(lens), seeds=seeds).cpu().numpy()
            assert sm.same_bytes(got, np.concatenate(want)), (W, C, fill)
            # the plan the call drew is the plan plan_rows gives, and a given plan gives the same rows
            drawn = post.plan_rows(lens, C, seeds=seeds)
            assert (drawn.cpu().numpy() == plan).all()
            again = post.apply_rows(gpu(np.concatenate(finite)), offsets(lens), plan=drawn).cpu().numpy()
            assert sm.same_bytes(again, got)
        inf = [with_infinities(u, rng) for u in finite]
        post = SpecAugment(2, 10, 2, 50, 1.0, W, 0.0, seed=0)
        want, _ = sm.augment_model(post, inf, sm.dither_keys(seeds))
        got = post.apply_rows(gpu(np.concatenate(inf)), offsets(lens), seeds=seeds).cpu().numpy()
        assert sm.same_bits(got, np.concatenate(want)), (W, C)


# ---- independence ---------------------------------------------------------------------------------------------------


def test_an_utterance_depends_on_its_key_and_nothing_else():
    lens, C = (90, 0, 33, 200, 64), 40
    utts = finite_batch(lens, C, np.float32, seed=4)
    seeds = [11, 12, 13, 14, 15]
    kw = dict(freq_masks=2, freq_width=10, time_masks=2, time_width=50, warp=5, fill="mean")
    post = SpecAugment(seed=99, **kw)
    batch = post.apply_rows(gpu(np.concatenate(utts)), offsets(lens), seeds=seeds).cpu().numpy()
    rows = offsets(lens)
    want, plan = sm.augment_model(post, utts, sm.dither_keys(seeds))
    assert sm.same_bytes(batch, np.concatenate(want))
    for b, u in enumerate(utts):
        if not len(u):
            continue
        alone = SpecAugment(seed=seeds[b], **kw).apply(u)  # the first apply of SpecAugment(seed=s)
        assert isinstance(alone, np.ndarray) and sm.same_bytes(alone, batch[rows[b]:rows[b + 1]]), b
    # permuting the batch permutes the outputs
    order = [3, 0, 4, 1, 2]
    shuffled = post.apply_rows(gpu(np.concatenate([utts[b] for b in order])), offsets([lens[b] for b in order]),
                               seeds=[seeds[b] for b in order]).cpu().numpy()
    assert sm.same_bytes(shuffled, np.concatenate([want[b] for b in order]))
    # the same seeds agree; other seeds differ where the model says they do
    again = post.apply_rows(gpu(np.concatenate(utts)), offsets(lens), seeds=seeds).cpu().numpy()
    assert sm.same_bytes(again, batch)
    other = [21, 22, 23, 24, 25]
    want2, plan2 = sm.augment_model(post, utts, sm.dither_keys(other))
    assert (plan2 != plan).any() and not sm.same_bytes(np.concatenate(want2), np.concatenate(want))
    got2 = post.apply_rows(gpu(np.concatenate(utts)), offsets(lens), seeds=other).cpu().numpy()
    assert sm.same_bytes(got2, np.concatenate(want2)) and not sm.same_bytes(got2, batch)
    # the object's own sequence: two objects of one seed agree call by call, and a call moves it
    a, b = SpecAugment(seed=5, **kw), SpecAugment(seed=5, **kw)
    first = a.apply(utts[0])
    assert sm.same_bytes(first, b.apply(utts[0]))
    second = a.apply(utts[0])
    assert sm.same_bytes(second, b.apply(utts[0])) and not sm.same_bytes(first, second)


# ---- apply ----------------------------------------------------------------------------------------------------------


def test_apply_on_arrays_and_tensors():
    import torch

    from pydrobert_speech_amd.torch import PyTorchPostProcessorWrapper

    kw = dict(freq_masks=2, freq_width=6, time_masks=2, time_width=20, warp=3, fill=-1.0)
    rng = np.random.default_rng(12)
    T, C, B = 50, 23, 3
    x = (rng.standard_normal((B, T, C)) * 20).astype(np.float32)
    keys = []
    state = sm._seed_state(31)
    for _ in range(B):
        state = sm._next_key(state)
        keys.append(state)
    post = SpecAugment(seed=31, **kw)
    want = np.stack(sm.augment_model(post, list(x), keys)[0])
    assert not sm.same_bytes(want, x)
    # 3-D, time on axis -2 (the default): every slice an utterance with the next key
    got = SpecAugment(seed=31, **kw).apply(x)
    assert isinstance(got, np.ndarray) and sm.same_bytes(got, want)
    t = SpecAugment(seed=31, **kw).apply(gpu(x))
    assert t.is_cuda and t.dtype == torch.float32 and sm.same_bytes(t.cpu().numpy(), want)
    # ... and on the last axis: (B, C, T)
    got = SpecAugment(seed=31, **kw).apply(np.ascontiguousarray(x.transpose(0, 2, 1)), axis=-1)
    assert got.shape == (B, C, T) and sm.same_bytes(got.transpose(0, 2, 1), want)
    t = SpecAugment(seed=31, **kw).apply(gpu(x).transpose(1, 2), axis=2)
    assert tuple(t.shape) == (B, C, T) and sm.same_bytes(t.cpu().numpy().transpose(0, 2, 1), want)
    # ... and in front: (T, B, C)
    got = SpecAugment(seed=31, **kw).apply(np.ascontiguousarray(x.transpose(1, 0, 2)), axis=0)
    assert got.shape == (T, B, C) and sm.same_bytes(got.transpose(1, 0, 2), want)
    # 2-D, both orders
    assert sm.same_bytes(SpecAugment(seed=31, **kw).apply(x[0]), want[0])
    assert sm.same_bytes(SpecAugment(seed=31, **kw).apply(x[0], axis=0), want[0])
    assert sm.same_bytes(SpecAugment(seed=31, **kw).apply(np.ascontiguousarray(x[0].T), axis=-1), want[0].T)
    assert sm.same_bytes(SpecAugment(seed=31, **kw).apply(gpu(x[0]).T, axis=1).cpu().numpy(), want[0].T)
    # other types are widened to float64
    for data in ((x[0] * 100).astype(np.int16), x[0].astype(np.float16)):
        wide = sm.augment_model(post, [data.astype(np.float64)], keys[:1])[0][0]
        got = SpecAugment(seed=31, **kw).apply(data)
        assert got.dtype == np.float64 and sm.same_bytes(got, wide)
        t = SpecAugment(seed=31, **kw).apply(gpu(data))
        assert t.dtype == torch.float64 and sm.same_bytes(t.cpu().numpy(), wide)
    # in place, only without a warp
    flat = dict(kw, warp=0)
    want0 = sm.augment_model(SpecAugment(**flat), [x[0]], keys[:1])[0][0]
    mine = x[0].copy()
    assert SpecAugment(seed=31, **flat).apply(mine, in_place=True) is mine and sm.same_bytes(mine, want0)
    dev = gpu(x[0])
    assert SpecAugment(seed=31, **flat).apply(dev, in_place=True) is dev and sm.same_bytes(dev.cpu().numpy(), want0)
    with pytest.raises(ValueError, match="in_place under warp"):
        SpecAugment(seed=31, **kw).apply(dev, in_place=True)
    with pytest.raises(ValueError, match="2-D or 3-D"):
        SpecAugment(seed=31).apply(np.zeros(5, dtype=np.float32))
    assert SpecAugment(seed=31, **kw).apply(np.zeros((0, C), dtype=np.float32)).shape == (0, C)
    # the torch module wraps it unchanged
    module = PyTorchPostProcessorWrapper.from_postprocessor(SpecAugment(seed=31, **kw))
    out = module(torch.from_numpy(x))
    assert not out.is_cuda and out.dtype == torch.float32 and sm.same_bytes(out.numpy(), want)


# ---- argument errors ------------------------------------------------------------------------------------------------


def test_argument_errors_of_the_packed_calls():
    import torch

    post, warped = SpecAugment(seed=0), SpecAugment(warp=2, seed=0)
    feats = torch.zeros((9, 4), device="cuda")
    for call in (post.apply_rows, post.mean_rows):
        with pytest.raises(ValueError, match="GPU tensor"):
            call(torch.zeros((9, 4)), [0, 9])
        with pytest.raises(ValueError, match="GPU tensor"):
            call(feats.to(torch.float16), [0, 9])
        with pytest.raises(ValueError, match="GPU tensor"):
            call(feats[0], [0, 1])
        for bad in ([0, 10], [3, 2], [-1, 4], []):
            with pytest.raises(ValueError, match="row_offsets"):
                call(feats, bad)
    with pytest.raises(ValueError, match="plan and seeds"):
        post.apply_rows(feats, [0, 9], seeds=[1], plan=post.plan_rows([9], 4, seeds=[1]))
    with pytest.raises(ValueError, match="one seed per utterance"):
        post.apply_rows(feats, [0, 4, 9], seeds=[1])
    with pytest.raises(ValueError, match="plan must be"):
        post.apply_rows(feats, [0, 4, 9], plan=post.plan_rows([9], 4, seeds=[1]))
    with pytest.raises(ValueError, match="plan must be"):
        post.apply_rows(feats, [0, 9], plan=post.plan_rows([9], 4, seeds=[1]).cpu())
    with pytest.raises(ValueError, match="plan must be"):
        post.apply_rows(feats, [0, 9], plan=SpecAugment(1, 1, 1, 1).plan_rows([9], 4, seeds=[1]))
    with pytest.raises(ValueError, match="out is feats under warp"):
        warped.apply_rows(feats, [0, 9], out=feats)
    with pytest.raises(ValueError, match="shares feats' memory"):
        warped.apply_rows(feats, [0, 9], out=feats[:])
    with pytest.raises(ValueError, match="out must be"):
        post.apply_rows(feats, [0, 9], out=torch.zeros((9, 4)))
    with pytest.raises(ValueError, match="out must be"):
        post.apply_rows(feats, [0, 9], out=torch.zeros((8, 4), device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        post.apply_rows(feats, [0, 9], out=torch.zeros((9, 4), device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError, match="out must be"):
        post.apply_rows(feats, [0, 9], out=torch.zeros((4, 9), device="cuda").T)
    with pytest.raises(ValueError, match="row count"):
        post.plan_rows([5, -1], 4)
    with pytest.raises(ValueError, match="row count"):
        post.plan_rows([1 << 31], 4)
    with pytest.raises(ValueError, match="C must be"):
        post.plan_rows([5], 0)
    with pytest.raises(ValueError, match="one seed per utterance"):
        post.plan_rows([5, 6], 4, seeds=[1])
    # what is allowed: no utterance, empty utterances, no column
    assert tuple(post.apply_rows(feats, [4]).shape) == (9, 4)
    assert tuple(post.apply_rows(feats, [2, 2, 2]).shape) == (9, 4)
    assert tuple(post.apply_rows(feats[:, :0], [0, 9]).shape) == (9, 0)
    assert tuple(post.mean_rows(feats, [4]).shape) == (0,)
    assert np.isnan(post.mean_rows(feats[:, :0], [0, 9]).cpu().numpy()).all()
    # a plan a caller wrote with words that lead nowhere changes nothing outside the utterance
    wild = torch.tensor([[1 << 62, -(1 << 62), -(1 << 62), (1 << 63) - 1, 1 << 62, 1 << 62, 0, 0, 0, 0]], device="cuda")
    guard = torch.full((11, 4), 3.0, device="cuda")
    out = post.apply_rows(guard, [1, 10], plan=wild, out=torch.full((11, 4), 5.0, device="cuda")).cpu().numpy()
    assert (out[0] == 5).all() and (out[10] == 5).all() and (out[1:10] == 0).all()  # (every column masked)
