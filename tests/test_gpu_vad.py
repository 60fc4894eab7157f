"""``post.EnergyVAD`` on the GPU against ``tests/vad_model.py``: decisions are equal and selected rows are the same
bytes -- ``decide`` over arrays and tensors, 2-D and 3-D, ``decide_rows`` / ``select_rows`` / ``apply_rows`` over packed
ragged batches (strided rows, another energy column, masks of every accepted kind), ``apply``, and non-finite
energies with and without the mean in the threshold."""
import functools

import numpy as np
import pytest

from pydrobert_speech_amd import post as post_module
from pydrobert_speech_amd.post import EnergyVAD
from tests.vad_model import select_rows, vad_decide, vad_decide_rows

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
SETTINGS = [dict(), dict(frames_context=2, proportion_threshold=0.5), dict(energy_mean_scale=0.0, energy_threshold=14.0,
                                                                           frames_context=5, proportion_threshold=0.3)]


def rule(vad):
    return dict(energy_threshold=vad.energy_threshold, energy_mean_scale=vad.energy_mean_scale,
                frames_context=vad.frames_context, proportion_threshold=vad.proportion_threshold)


@functools.lru_cache(maxsize=None)
def _features(T, C, dtype, col, seed):
    rng = np.random.default_rng(1000 * T + C + seed)
    x = rng.standard_normal((T, C)).astype(dtype)
    x[:, col] = (12.0 + 6.0 * rng.standard_normal(T)).astype(dtype)
    return x


def features(T, C, dtype, col=0, seed=0):
    """``(T, C)`` rows whose column `col` holds energies on both sides of Kaldi's default threshold (the caller's own
    copy of rows drawn once)"""
    return _features(T, C, dtype, col, seed).copy()


def same_bytes(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("kwargs", SETTINGS, ids=["kaldi", "context2", "fixed_threshold"])
def test_decide_arrays_and_tensors_2d_and_3d(kwargs, dtype):
    import torch

    vad = EnergyVAD(**kwargs)
    x = features(300, 5, dtype)
    want = vad_decide(x[:, 0], **rule(vad))
    assert 30 < want.sum() < 270
    got = vad.decide(x)
    assert isinstance(got, np.ndarray) and got.dtype == bool and got.shape == (300,) and (got == want).all()
    got = vad.decide(torch.from_numpy(x.copy()).cuda())
    assert got.is_cuda and got.dtype == torch.bool and tuple(got.shape) == (300,) and (got.cpu().numpy() == want).all()
    # coefficients first
    got = vad.decide(np.ascontiguousarray(x.T), axis=0)
    assert got.shape == (300,) and (got == want).all()
    # a batch: every utterance decided by itself
    batch = np.stack([features(130, 4, dtype, seed=s) for s in range(3)])
    batch[1, :, 0] -= 9.0  # (a quiet utterance has its own, lower threshold)
    want3 = np.stack([vad_decide(u[:, 0], **rule(vad)) for u in batch])
    got = vad.decide(batch)
    assert got.dtype == bool and got.shape == (3, 130) and (got == want3).all()
    got = vad.decide(torch.from_numpy(batch).cuda())
    assert got.dtype == torch.bool and tuple(got.shape) == (3, 130) and (got.cpu().numpy() == want3).all()
    got = vad.decide(np.ascontiguousarray(batch.transpose(0, 2, 1)), axis=1)
    assert got.shape == (3, 130) and (got == want3).all()
    with pytest.raises(ValueError):
        vad.decide(x[:, 0])


def test_other_dtypes_are_widened_to_float64():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 25, size=(200, 3)).astype(np.int32)
    vad = EnergyVAD(frames_context=1)
    want = vad_decide(x[:, 0].astype(np.float64), **rule(vad))
    assert (vad.decide(x) == want).all() and 20 < want.sum() < 180
    out = vad.apply(x)
    assert out.dtype == np.float64 and same_bytes(out, x.astype(np.float64)[want])
    half = x.astype(np.float16)
    assert (vad.decide(half) == vad_decide(half[:, 0].astype(np.float64), **rule(vad))).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("kwargs", SETTINGS, ids=["kaldi", "context2", "fixed_threshold"])
def test_rows_of_a_packed_ragged_batch(kwargs, dtype):
    import torch

    vad = EnergyVAD(**kwargs)
    lens = [70, 0, 1, 200, 3, 64, 0]
    offsets = np.concatenate([[2], 2 + np.cumsum(lens)]).astype(np.int64)  # two rows of no utterance in front, three behind
    R, C = int(offsets[-1]) + 3, 6
    feats = features(R, C, dtype, seed=3)
    feats[:2, 0] = feats[-3:, 0] = 1e6  # (read by mistake they would move a threshold)
    want_voiced, want_counts = vad_decide_rows(feats, offsets, **rule(vad))
    want_out, want_offs = select_rows(feats, offsets, want_voiced)
    assert 0 < want_counts[0] < 70 and 0 < want_counts[3] < 200 and want_counts[1] == 0
    d = torch.from_numpy(feats).cuda()
    voiced, counts = vad.decide_rows(d, offsets)
    assert voiced.is_cuda and voiced.dtype == torch.uint8 and tuple(voiced.shape) == (R,)
    assert isinstance(counts, np.ndarray) and counts.dtype == np.int64 and counts.tolist() == want_counts.tolist()
    assert (voiced.cpu().numpy() == want_voiced).all()  # (0 in rows of no utterance)
    for mask in (voiced, voiced.bool(), voiced * 255, voiced.cpu().numpy(), voiced.cpu().numpy().astype(bool)):
        out, offs = vad.select_rows(d, offsets, mask)
        assert out.is_cuda and isinstance(offs, np.ndarray) and offs.dtype == np.int64
        assert offs.tolist() == want_offs.tolist() and same_bytes(out.cpu().numpy(), want_out)
    # any mask selects: a mask set in rows of no utterance too keeps the utterances' rows alone
    every = torch.ones(R, dtype=torch.bool, device="cuda")
    out, offs = vad.select_rows(d, offsets, every)
    assert offs.tolist() == (offsets - 2).tolist() and same_bytes(out.cpu().numpy(), feats[2:-3])
    out, offs = vad.select_rows(d, offsets, torch.zeros(R, dtype=torch.uint8, device="cuda"))
    assert offs.tolist() == [0] * len(offsets) and tuple(out.shape) == (0, C) and out.dtype == d.dtype
    out, offs = vad.apply_rows(d, offsets)
    assert offs.tolist() == want_offs.tolist() and same_bytes(out.cpu().numpy(), want_out)
    assert same_bytes(d.cpu().numpy(), feats)  # (the input is left alone)
    for bad in (voiced[:-1], voiced.to(torch.int32), voiced.cpu().numpy().astype(np.int64)):
        with pytest.raises(ValueError):
            vad.select_rows(d, offsets, bad)
    for bad in ([0, R + 1], [3, 2], [-1, 4]):
        with pytest.raises(ValueError):
            vad.decide_rows(d, bad)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_strided_column_slice_and_another_energy_column(dtype):
    import torch

    offsets = np.asarray([0, 90, 90, 300], dtype=np.int64)
    wide = features(300, 12, dtype, col=5).copy()
    wide[:, 3] = np.nan  # the slice's column 0: not the energy
    d_wide = torch.from_numpy(wide).cuda()
    d = d_wide[:, 3:9]  # rows 12 elements apart, 6 wide; the energy is column 2 of the slice
    assert d.stride(0) == 12 and not d.is_contiguous()
    for kwargs in SETTINGS:
        vad = EnergyVAD(energy_col=2, **kwargs)
        want_voiced, want_counts = vad_decide_rows(wide[:, 3:9], offsets, energy_col=2, **rule(vad))
        want_out, want_offs = select_rows(wide[:, 3:9], offsets, want_voiced)
        assert 0 < want_counts[0] < 90 and 0 < want_counts[2] < 210
        voiced, counts = vad.decide_rows(d, offsets)
        assert (voiced.cpu().numpy() == want_voiced).all() and counts.tolist() == want_counts.tolist()
        out, offs = vad.apply_rows(d, offsets)
        assert out.is_contiguous() and offs.tolist() == want_offs.tolist() and same_bytes(out.cpu().numpy(), want_out)
        assert (vad.decide(d) == torch.from_numpy(vad_decide(wide[:, 5], **rule(vad))).cuda()).all()
        got = vad.apply(d)
        assert same_bytes(got.cpu().numpy(), wide[:, 3:9][vad_decide(wide[:, 5], **rule(vad))])
    with pytest.raises(ValueError, match="energy_col"):
        EnergyVAD(energy_col=6).decide_rows(d, offsets)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_without_the_mean_nan_energies_elsewhere_do_not_matter(dtype):
    """``energy_mean_scale == 0``: nothing is summed, so a NaN energy makes its own frame unvoiced (and counts as not
    above the threshold in its neighbours' windows) and nothing else -- other utterances, other frames, other columns"""
    import torch

    offsets = np.asarray([0, 100, 230, 300], dtype=np.int64)
    x = features(300, 4, dtype).copy()
    x[:, 1:] = np.nan
    x[[3, 50, 99, 100, 299], 0] = np.nan
    x[130:200, 0] = np.nan
    clean = np.where(np.isnan(x[:, 0]), -1e30, x[:, 0])  # a NaN energy votes like a very low one
    d = torch.from_numpy(x).cuda()
    for context in (0, 3):
        vad = EnergyVAD(11.0, 0.0, context, 0.5)
        want_voiced, want_counts = vad_decide_rows(x, offsets, **rule(vad))
        assert (want_voiced == vad_decide_rows(clean[:, None], offsets, **rule(vad))[0]).all()
        assert (context or not want_voiced[[3, 50, 99, 100, 299]].any()) and want_counts.min() > 10
        voiced, counts = vad.decide_rows(d, offsets)
        assert (voiced.cpu().numpy() == want_voiced).all() and counts.tolist() == want_counts.tolist()
        out, offs = vad.apply_rows(d, offsets)
        want_out, want_offs = select_rows(x, offsets, want_voiced)
        assert offs.tolist() == want_offs.tolist() and same_bytes(out.cpu().numpy(), want_out)  # (NaN columns pass)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_non_finite_energies_under_a_mean_scaled_threshold(dtype):
    """a NaN or infinite sum makes every comparison of its utterance false or true as IEEE says, and leaves the
    utterances beside it alone"""
    import torch

    nan, inf = np.nan, np.inf
    T = 150
    poison = [(nan,), (inf,), (-inf,), (inf, -inf), (), (nan, inf), (-inf, -inf)]
    offsets = np.arange(len(poison) + 1, dtype=np.int64) * T
    x = np.concatenate([features(T, 3, dtype, seed=s) for s in range(len(poison))]).copy()
    for b, values in enumerate(poison):
        for i, v in enumerate(values):
            x[b * T + 7 + 64 * i, 0] = v  # (in different partial sums and in the same one)
    d = torch.from_numpy(x).cuda()
    for context in (0, 2):
        vad = EnergyVAD(frames_context=context)
        want_voiced, want_counts = vad_decide_rows(x, offsets, **rule(vad))
        # NaN sum: nothing; +inf: nothing; -inf: every finite frame (the -inf frame itself is not above -inf)
        assert want_counts[0] == want_counts[1] == want_counts[3] == want_counts[5] == 0
        assert 0 < want_counts[4] < T and (want_counts[2] == T - 1 or context) and want_counts[2] >= T - 1
        voiced, counts = vad.decide_rows(d, offsets)
        assert (voiced.cpu().numpy() == want_voiced).all() and counts.tolist() == want_counts.tolist()
        out, offs = vad.apply_rows(d, offsets)
        want_out, want_offs = select_rows(x, offsets, want_voiced)
        assert offs.tolist() == want_offs.tolist() and same_bytes(out.cpu().numpy(), want_out)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_apply_gives_the_voiced_rows(dtype):
    import torch

    x = features(333, 7, dtype)
    for kwargs in SETTINGS:
        vad = EnergyVAD(**kwargs)
        want = x[vad_decide(x[:, 0], **rule(vad))]
        got = vad.apply(x)
        assert isinstance(got, np.ndarray) and same_bytes(got, want) and 0 < len(want) < 333
        got = vad.apply(torch.from_numpy(x.copy()).cuda())
        assert got.is_cuda and same_bytes(got.cpu().numpy(), want)
        got = vad.apply(np.ascontiguousarray(x.T), axis=0)  # coefficients first: frames are the columns
        assert same_bytes(got, want.T)
    # nothing voiced, and no frames at all
    none = EnergyVAD(1e9, 0.0).apply(x)
    assert none.shape == (0, 7) and none.dtype == dtype
    empty = EnergyVAD().apply(np.zeros((0, 7), dtype=dtype))
    assert empty.shape == (0, 7) and empty.dtype == dtype
    assert EnergyVAD().decide(np.zeros((0, 7), dtype=dtype)).shape == (0,)
    assert EnergyVAD().decide(np.zeros((2, 0, 7), dtype=dtype)).shape == (2, 0)


def test_a_batch_too_large_for_one_grid_is_split(monkeypatch):
    """``select_rows`` splits a batch whose blocks (utterances x tiles of 256 rows) exceed a grid; with the limit
    lowered to a few blocks the same split gives the same rows"""
    import torch

    lens = [600, 0, 257, 1, 900, 256, 30, 512, 2, 700]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x = features(int(offsets[-1]), 5, np.float32, seed=9)
    d = torch.from_numpy(x.copy()).cuda()
    vad = EnergyVAD()
    want_out, want_offs = vad.apply_rows(d, offsets)
    ref_voiced, _ = vad_decide_rows(x, offsets, **rule(vad))
    assert same_bytes(want_out.cpu().numpy(), select_rows(x, offsets, ref_voiced)[0])
    launches = []
    real = post_module._native.stages_lib()

    class Counting:
        def __getattr__(self, name):
            return getattr(real, name)

        def pds_select_rows_w32(self, *args):
            launches.append(args[5])  # (B of the call)
            return real.pds_select_rows_w32(*args)

    for limit, expect in ((4, [1] * 10), (9, [2] * 5), (13, [3, 3, 3, 1])):
        del launches[:]
        monkeypatch.setattr(post_module, "_SELECT_MAX_BLOCKS", limit)
        monkeypatch.setattr(post_module._native, "stages_lib", lambda: Counting())
        out, offs = vad.apply_rows(d, offsets)
        monkeypatch.undo()
        assert launches == expect and offs.tolist() == want_offs.tolist() and same_bytes(out.cpu().numpy(), want_out.cpu().numpy())
