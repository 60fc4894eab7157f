"""``post.Cepstra`` and ``pds_cepstra_rows_*`` on the GPU against numpy, byte for byte.

The arithmetic is fixed (post.py Cepstra): a float64 accumulator from +0.0, ``acc = acc + M[k, f] * float64(x[f])`` with
f ascending, product and sum rounded separately, one rounding to the rows' dtype.  numpy does exactly that in
:func:`emulate`, so every comparison here is an equality of bytes."""
import functools

import numpy as np
import pytest

from pydrobert_speech_amd import _native
from pydrobert_speech_amd.post import Cepstra

pytestmark = pytest.mark.gpu

# (F, K, copy_cols): one column; odd widths; the usual 40 -> 13; K = F; an energy column; the widths around the tile's
# 64 KB (127: 64 rows per block, 128: 32) and the widest row served (255 + 1: 16 rows per block)
SHAPES = [(1, 1, 0), (2, 2, 0), (23, 13, 0), (40, 13, 0), (40, 40, 0), (40, 12, 1), (80, 79, 1), (127, 5, 0),
          (128, 128, 0), (255, 3, 1)]
ROWS = [0, 1, 63, 64, 65, 257, 4099]
DTYPES = [np.float32, np.float64]


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def emulate(x, M, copy_cols, dtype=None):
    """the kernel's arithmetic over the rows of the 2-D `x` with the host matrix `M` (``[K, F]``)"""
    dtype = x.dtype if dtype is None else dtype
    acc = np.zeros((x.shape[0], M.shape[0]), dtype=np.float64)
    for f in range(M.shape[1]):
        acc = acc + M[:, f][None, :] * x[:, copy_cols + f].astype(np.float64)[:, None]
    return np.concatenate([x[:, :copy_cols].astype(dtype), acc.astype(dtype)], axis=1)


def cepstra_of(F, K, copy_cols):
    """the object whose matrix for rows of ``copy_cols + F`` columns has K rows"""
    return Cepstra(K + copy_cols, lifter=22.0, energy=bool(copy_cols))


@functools.lru_cache(maxsize=None)
def case(F, K, copy_cols, dtype):
    """(input rows, expected output rows) of the largest row count, computed once and left unchanged: the smaller
    ones are its prefixes"""
    rng = np.random.default_rng(1000 * F + 10 * K + copy_cols)
    x = (20 * rng.standard_normal((max(ROWS), copy_cols + F)) - 5).astype(dtype)
    M, copy = cepstra_of(F, K, copy_cols).matrix(copy_cols + F)
    assert copy == copy_cols and M.shape == (K, F)
    return x, emulate(x, M, copy_cols)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F,K,copy_cols", SHAPES)
def test_rows_equal_the_numpy_emulation(F, K, copy_cols, dtype):
    x, want = case(F, K, copy_cols, dtype)
    post = cepstra_of(F, K, copy_cols)
    for R in ROWS:
        got = post.apply(x[:R])
        assert got.dtype == dtype and got.shape == (R, copy_cols + K), R
        assert same_bytes(got, want[:R]), (R, float(np.abs(got - want[:R]).max()) if R else 0.0)


def test_norm_and_lifter_reach_the_kernel():
    x, _ = case(40, 13, 0, np.float32)
    for kwargs in (dict(norm=None), dict(lifter=0), dict(lifter=None, norm=None), dict(lifter=3.5)):
        post = Cepstra(13, **kwargs)
        assert same_bytes(post.apply(x[:65]), emulate(x[:65], post.matrix(40)[0], 0)), kwargs


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_column_slice_of_a_wider_tensor(dtype):
    import torch

    rng = np.random.default_rng(3)
    W = 41
    wide = rng.standard_normal((130, 50)).astype(dtype)
    post = Cepstra(13, energy=True)
    d_wide = torch.from_numpy(wide).cuda()
    view = d_wide[:, 3 : 3 + W]
    assert view.stride(0) == 50 and not view.is_contiguous()
    got = post.apply(view)
    assert got.is_cuda and same_bytes(got.cpu().numpy(), emulate(wide[:, 3 : 3 + W], post.matrix(W)[0], 1))
    assert same_bytes(d_wide.cpu().numpy(), wide)  # (the input is left alone)


@pytest.mark.parametrize("dtype", DTYPES)
def test_output_into_a_wider_buffer_leaves_the_other_columns(dtype):
    import torch

    lib = _native.lib()
    fn = lib.pds_cepstra_rows_f32 if dtype == np.float32 else lib.pds_cepstra_rows_f64
    rng = np.random.default_rng(4)
    R, F, K, copy_cols, lead, width = 131, 40, 12, 1, 2, 20
    x = rng.standard_normal((R, copy_cols + F)).astype(dtype)
    M, _ = Cepstra(13, energy=True).matrix(copy_cols + F)
    before = rng.standard_normal((R, width)).astype(dtype)
    d_x, d_M, d_out = torch.from_numpy(x).cuda(), torch.from_numpy(M).cuda(), torch.from_numpy(before).cuda()
    rc = fn(d_x.data_ptr(), d_x.stride(0), R, F, d_M.data_ptr(), K, copy_cols,
            d_out.data_ptr() + lead * d_out.element_size(), width, torch.cuda.current_stream().cuda_stream)
    _native.check(rc, "pds_cepstra_rows")
    after = d_out.cpu().numpy()
    assert same_bytes(after[:, lead : lead + copy_cols + K], emulate(x, M, copy_cols))
    assert same_bytes(after[:, :lead], before[:, :lead])
    assert same_bytes(after[:, lead + copy_cols + K :], before[:, lead + copy_cols + K :])


def test_apply_forms():
    import torch

    rng = np.random.default_rng(6)
    post = Cepstra(13)
    M, _ = post.matrix(40)
    # a 3-D numpy array with the coefficients on axis 1: the other axes are kept
    x = rng.standard_normal((3, 40, 5)).astype(np.float32)
    got = post.apply(x, axis=1)
    assert isinstance(got, np.ndarray) and got.shape == (3, 13, 5)
    want = emulate(np.moveaxis(x, 1, -1).reshape(-1, 40), M, 0).reshape(3, 5, 13)
    assert same_bytes(got, np.moveaxis(want, -1, 1))
    assert same_bytes(post.apply(x, axis=-2, in_place=True), got)  # (in_place is accepted and ignored)
    # a GPU tensor in, a GPU tensor out, the same dtype and device
    d_x = torch.from_numpy(np.ascontiguousarray(np.moveaxis(x, 1, -1))).cuda().to(torch.float64)
    d_got = post.apply(d_x)
    assert d_got.is_cuda and d_got.dtype == torch.float64 and tuple(d_got.shape) == (3, 5, 13)
    assert same_bytes(d_got.cpu().numpy(), emulate(d_x.cpu().numpy().reshape(-1, 40), M, 0).reshape(3, 5, 13))
    # anything but float32 / float64 is computed and returned as float64
    pcm = rng.integers(-3000, 3000, size=(7, 40)).astype(np.int16)
    got = post.apply(pcm)
    assert got.dtype == np.float64 and same_bytes(got, emulate(pcm.astype(np.float64), M, 0))
    # a single vector
    assert same_bytes(post.apply(x[0, :, 0]), emulate(x[0, :, 0][None], M, 0)[0])
    # no rows: an empty result of the right shape (no launch: nothing could have written it)
    for empty in (np.zeros((0, 40), np.float32), np.zeros((4, 0, 40), np.float64), np.zeros((40, 0), np.float32)):
        axis = 0 if empty.shape[0] == 40 else -1
        got = post.apply(empty, axis=axis)
        shape = list(empty.shape)
        shape[axis] = 13
        assert got.dtype == empty.dtype and got.shape == tuple(shape)
    assert tuple(post.apply(torch.zeros((0, 40), device="cuda")).shape) == (0, 13)
    # the energy alone: nothing to transform
    only = Cepstra(1, energy=True).apply(x[0].T.copy())
    assert same_bytes(only, x[0].T[:, :1])
    # the matrix is built once per width and device
    assert len(post._device_matrix) == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_rows_stay_where_they_are(dtype):
    rng = np.random.default_rng(7)
    post = Cepstra(13, energy=True)
    W = 41
    M, _ = post.matrix(W)
    x = rng.standard_normal((130, W)).astype(dtype)
    clean = post.apply(x)
    x[5, 7] = np.nan
    x[64, 40] = np.inf
    x[65, 1] = -np.inf
    x[66, 3], x[66, 4] = np.inf, -np.inf  # inf - inf
    x[9, 0], x[10, 0], x[11, 0], x[12, 0], x[13, 0] = np.nan, -0.0, 0.0, -np.inf, np.inf  # the energy column
    x[129] = 0.0
    x[128] = -0.0
    with np.errstate(invalid="ignore"):
        want = emulate(x, M, 1)
    got = post.apply(x)
    dirty = [5, 9, 10, 11, 12, 13, 64, 65, 66, 128, 129]
    assert np.isnan(want[5, 1:]).all() and np.isnan(want[66, 1]) and np.isinf(want[64, 1:]).any()
    assert np.array_equal(got, want, equal_nan=True)
    finite = ~np.isnan(want)  # (a NaN that arithmetic makes has no agreed sign)
    assert np.array_equal(np.signbit(got)[finite], np.signbit(want)[finite])
    # the copied energy column: NaN stays NaN, the zeros keep their signs
    assert np.array_equal(got[:, 0], x[:, 0], equal_nan=True)
    assert np.array_equal(np.signbit(got[:, 0]), np.signbit(x[:, 0]))
    # the neighbours' bytes are what they were
    others = np.setdiff1d(np.arange(130), dirty)
    assert same_bytes(got[others], clean[others])
    assert same_bytes(got[[9, 10, 11, 12, 13]][:, 1:], clean[[9, 10, 11, 12, 13]][:, 1:])


def test_torch_wrapper_on_a_cpu_tensor():
    import torch

    from pydrobert_speech_amd.torch import PyTorchPostProcessorWrapper

    x = np.random.default_rng(8).standard_normal((70, 40)).astype(np.float32)
    module = PyTorchPostProcessorWrapper.from_postprocessor(Cepstra(13))
    got = module(torch.from_numpy(x))
    assert not got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (70, 13)
    assert same_bytes(got.numpy(), emulate(x, Cepstra(13).matrix(40)[0], 0))


@pytest.mark.slow
def test_byte_offsets_past_32_bits():
    import torch

    R, stride, F, K = 70000, 16384, 40, 13
    assert (R - 1) * stride * 4 > 1 << 32
    lib = _native.lib()
    rng = np.random.default_rng(9)
    picks = [0, 34999, 69999]
    post = Cepstra(K)
    M, _ = post.matrix(F)
    buf = torch.empty(R * stride, dtype=torch.float32, device="cuda")  # (only the F used columns are filled)
    rows = buf.view(R, stride)[:, :F]
    x = rng.standard_normal((len(picks), F)).astype(np.float32)
    rows.zero_()
    rows[picks] = torch.from_numpy(x).cuda()
    got = post.apply(rows)  # the strided view as it is
    assert tuple(got.shape) == (R, K)
    assert same_bytes(got[picks].cpu().numpy(), emulate(x, M, 0))
    assert not got[1].any() and not got[69998].any()
    # ... and a strided output through the C call
    out = torch.empty(R * stride, dtype=torch.float32, device="cuda")
    d_M = torch.from_numpy(M).cuda()
    rc = lib.pds_cepstra_rows_f32(rows.data_ptr(), stride, R, F, d_M.data_ptr(), K, 0, out.data_ptr(), stride,
                                  torch.cuda.current_stream().cuda_stream)
    _native.check(rc, "pds_cepstra_rows")
    assert same_bytes(out.view(R, stride)[picks][:, :K].cpu().numpy(), emulate(x, M, 0))
