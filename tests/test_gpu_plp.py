"""``post.PLP`` on the GPU against the numpy model of its definition (tests/plp_model.py), one kernel shape at a time.

Everything behind the ``pow`` of step 3 is plain IEEE arithmetic: with the auxiliary output the test runs steps 5 to 7
on the device's own ``d`` and must get the device's ``E`` and cepstra bit for bit.  ``d`` itself and the ``log`` of
column 0 go through device functions and are compared under the package's standing tolerances (``1e-5 + 1e-4 |ref|``
for float32 rows, ``rtol = atol = 1e-9`` for float64), as is the whole output against the model, no element exempted;
``apply`` equals ``apply_rows`` bit for bit.  Inputs are ``exp(N(0, 2))`` scaled per row by 1e-8, 1 or 1e6 with a few
exact zeros; a 2-ulp change of ``d`` moves no output of such rows by a thousandth of the float64 tolerance
(tests/test_plp_host.py), so the tolerance tests the kernel, not the conditioning.

Shapes: row counts 1, 2, 63, 64, 65 and below, at and above one and two blocks' rows; F of 1, 2, 23, 40 and 65 with
and without the energy column, float32 and float64; p of 1, 2, 12 and min(F + 1, 32) with K of 1, 2 and p + 1; strided
rows and a strided ``out``; 2-D and 3-D arrays and tensors; an integer dtype."""
import functools

import numpy as np
import pytest

from pydrobert_speech_amd import _native
from pydrobert_speech_amd.post import PLP
from tests.plp_model import (energies, plp_from_spectrum, plp_model, plp_spectrum, plp_tables, same_bits,
                             tolerance_ratio, within_tolerance)

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
WIDTHS = (1, 2, 23, 40, 65)  # F


def centers(F):
    return [60.0 + 7900.0 * (f + 0.5) / F for f in range(F)]


@functools.lru_cache(maxsize=None)
def rows_of(R, W, dtype, seed=0):
    """the tests' input of `R` rows of `W` columns; computed once, left unchanged (a test that changes rows copies)"""
    return energies(np.random.default_rng(100000 * seed + 300 * R + W), (R, W), dtype)


def close(got, ref):
    """float64 ``rtol = atol = 1e-9``"""
    return bool((np.abs(got - ref) <= 1e-9 + 1e-9 * np.abs(ref)).all())


def check(post, x, what=""):
    """the four assertions of a case for the rows `x` (host, R x W); returns the output (host)"""
    import torch

    x = np.asarray(x)
    R, W = x.shape
    dtype = x.dtype if x.dtype in (np.float32, np.float64) else np.dtype(np.float64)
    F, K = W - int(post.energy), post.num_ceps
    D = F + 2
    w, B, L = plp_tables(post, W)
    d_x = torch.from_numpy(np.ascontiguousarray(x).astype(dtype)).cuda()
    assert post.aux_width(W) == D + 1
    aux = torch.full((R, D + 1), -7.0, dtype=torch.float64, device="cuda")
    out = post.apply_rows(d_x, aux=aux)
    assert out.is_cuda and tuple(out.shape) == (R, K)
    got, aux = out.cpu().numpy(), aux.cpu().numpy()
    assert got.dtype == dtype
    # 1. steps 5 to 7 on the device's own d: E and the cepstra bit for bit, column 0 within the tolerance of the log
    q, E = plp_from_spectrum(aux[:, :D], B)
    assert same_bits(aux[:, D], E), what
    assert same_bits(got[:, 1:], (L[None, 1:] * q[:, : K - 1]).astype(dtype)), what
    if post.energy:
        e0 = x[:, 0].astype(np.float64)
        col0 = np.log(np.where(e0 < post.floor, post.floor, e0))
    else:
        col0 = L[0] * np.log(aux[:, D])
    assert within_tolerance(got[:, 0], col0.astype(dtype)), what
    # 2. the device's d against the model's
    assert close(aux[:, :D], plp_spectrum(post, x, w)), what
    # 3. the whole output against the model, no element exempted
    ref = plp_model(post, x)
    print(f"{what} R={R} F={F} p={post.lpc_order} K={K} {np.dtype(dtype).name}: worst error "
          f"{tolerance_ratio(got, ref):.3g} of the tolerance")
    assert within_tolerance(got, ref), what
    # 4. apply equals apply_rows bit for bit, and the input is left as it was
    applied = post.apply(x)
    assert isinstance(applied, np.ndarray) and same_bits(applied, got), what
    assert same_bits(d_x.cpu().numpy(), np.ascontiguousarray(x).astype(dtype)), what
    return got


def block_rows():
    return int(_native.stages4_lib().pds_plp_block_rows())


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_row_count_around_the_blocks_edges(dtype):
    n = block_rows()
    assert n == 64
    counts = sorted({1, 2, 63, 64, 65, n - 1, n, n + 1, 2 * n - 1, 2 * n, 2 * n + 1})
    post = PLP(centers_hz=centers(23))
    whole = check(post, rows_of(counts[-1], 23, dtype), "all rows")
    for R in counts:
        got = check(post, rows_of(counts[-1], 23, dtype)[:R], f"{R} rows")
        assert same_bits(got, whole[:R])  # a row's bits do not depend on the rows around it


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("energy", [False, True], ids=["statics", "energy"])
@pytest.mark.parametrize("F", WIDTHS)
def test_every_width_order_and_output_width(F, energy, dtype):
    W = F + int(energy)
    x = rows_of(65, W, dtype)
    for p in sorted({1, 2, 12, min(F + 1, 32)}):
        if p > min(F + 1, 32):
            continue
        for K in sorted({1, 2, p + 1}):
            post = PLP(num_ceps=K, lpc_order=p, centers_hz=centers(F), energy=energy)
            got = check(post, x, f"p={p} K={K}")
            assert np.isfinite(got).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kwargs", [{"equal_loudness": False}, {"compress_factor": 0.5}, {"lifter": 0},
                                    {"scale": 0.1}, {"lifter": None, "scale": 0.1, "floor": 1e-10}],
                         ids=["flat", "sqrt", "unliftered", "scaled", "all"])
def test_the_other_arguments(kwargs, dtype):
    for F, energy in ((23, False), (40, True)):
        post = PLP(centers_hz=centers(F), energy=energy, **kwargs)
        default = PLP(centers_hz=centers(F), energy=energy)
        x = rows_of(65, F + int(energy), dtype)
        got = check(post, x, str(kwargs))
        assert not same_bits(got, check(default, x))  # (the argument arrives)


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_rows_and_a_strided_out(dtype):
    import torch

    tdtype = torch.float32 if dtype == np.float32 else torch.float64
    F, K, R = 23, 13, 70
    post = PLP(centers_hz=centers(F))
    x = rows_of(R, F, dtype)
    want = check(post, x)
    # a column slice of a wider tensor: a row stride wider than the row
    wide = torch.full((R, F + 9), float("nan"), dtype=tdtype, device="cuda")
    wide[:, 4: 4 + F] = torch.from_numpy(x.copy()).cuda()
    view = wide[:, 4: 4 + F]
    assert view.stride(0) == F + 9
    before = wide.clone()
    assert same_bits(post.apply_rows(view).cpu().numpy(), want)
    assert same_bits(post.apply(view).cpu().numpy(), want)  # (no copy on this path either)
    assert same_bits(wide.cpu().numpy(), before.cpu().numpy())
    # out= with a wider stride, and only the rows of the offsets: everything else keeps its bits
    big = torch.full((R, K + 5), -3.0, dtype=tdtype, device="cuda")
    out = big[:, 2: 2 + K]
    aux = torch.full((R, post.aux_width(F)), -5.0, dtype=torch.float64, device="cuda")
    back = post.apply_rows(view, row_offsets=[3, 10, 10, R - 2], out=out, aux=aux)
    assert back is out
    host = big.cpu().numpy()
    assert same_bits(host[3: R - 2, 2: 2 + K], want[3: R - 2])
    assert (host[:3] == -3.0).all() and (host[R - 2:] == -3.0).all()  # rows outside the offsets
    assert (host[:, :2] == -3.0).all() and (host[:, 2 + K:] == -3.0).all()  # columns past K
    aux = aux.cpu().numpy()
    assert (aux[:3] == -5.0).all() and (aux[R - 2:] == -5.0).all() and (aux[3: R - 2] > 0).all()
    # no rows: nothing is launched, nothing is written
    assert post.apply_rows(view, row_offsets=[5, 5], out=out) is out
    assert tuple(post.apply_rows(view[:0]).shape) == (0, K)
    with pytest.raises(ValueError, match="out must be"):
        post.apply_rows(view, out=big)
    with pytest.raises(ValueError, match="share"):
        post.apply_rows(view, out=wide[:, :K])  # (nothing is done in place)
    with pytest.raises(ValueError, match="aux must be"):
        post.apply_rows(view, aux=torch.zeros((R, F + 2), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="row_offsets"):
        post.apply_rows(view, row_offsets=[0, R + 1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_arrays_and_tensors_of_two_and_three_dimensions(dtype):
    import torch

    F, K = 23, 13
    post = PLP(centers_hz=centers(F))
    x = rows_of(60, F, dtype)
    want = check(post, x)
    cube = x.reshape(3, 20, F)
    for arr, axis, back in ((x, -1, lambda y: y), (x.T, 0, lambda y: y.T), (cube, 2, lambda y: y.reshape(60, K)),
                            (cube.transpose(0, 2, 1), 1, lambda y: y.transpose(0, 2, 1).reshape(60, K)),
                            (cube.transpose(2, 0, 1), 0, lambda y: y.transpose(1, 2, 0).reshape(60, K))):
        got = post.apply(arr, axis=axis)
        assert isinstance(got, np.ndarray) and got.dtype == dtype
        assert got.shape == arr.shape[:axis % arr.ndim] + (K,) + arr.shape[axis % arr.ndim + 1:]
        assert same_bits(back(got), want)
        t = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        got_t = post.apply(t, axis=axis)
        assert got_t.is_cuda and same_bits(got_t.cpu().numpy(), got)
    assert same_bits(post.apply(x[0]), want[0])  # one row, one dimension


def test_an_integer_dtype_is_computed_as_float64():
    import torch

    F = 23
    post = PLP(centers_hz=centers(F))
    x = np.random.default_rng(3).integers(0, 30000, (65, F)).astype(np.int32)
    x[3, 5] = 0
    got = post.apply(x)
    assert got.dtype == np.float64 and same_bits(got, check(post, x.astype(np.float64)))
    t = post.apply(torch.from_numpy(x).cuda())
    assert t.dtype == torch.float64 and same_bits(t.cpu().numpy(), got)
    assert within_tolerance(got, plp_model(post, x))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("energy", [False, True], ids=["statics", "energy"])
def test_a_nan_row_is_all_nan_and_its_neighbours_keep_their_bits(energy, dtype):
    F = 23
    W = F + int(energy)
    post = PLP(centers_hz=centers(F), energy=energy)
    x = rows_of(130, W, dtype).copy()
    clean = post.apply(x)
    for row, col in ((0, W - 1), (64, int(energy)), (77, W // 2)):
        x[row, col] = np.nan
    x[5] = 0.0  # a row of zeros is finite, because of the floor
    got = post.apply(x)
    for row in (0, 64, 77):
        assert np.isnan(got[row, int(energy):]).all()  # every computed column
        if energy:
            assert got[row, 0] == clean[row, 0]  # (the energy column holds no NaN: its log is as before)
    keep = np.ones(130, dtype=bool)
    keep[[0, 5, 64, 77]] = False
    assert same_bits(got[keep], clean[keep])
    assert np.isfinite(got[5]).all()
    assert within_tolerance(got, plp_model(post, x))
    # an infinite energy does not disturb the other rows either
    x[9, W - 2 if W > 1 else 0] = np.inf
    keep[9] = False
    with np.errstate(all="ignore"):
        assert same_bits(post.apply(x)[keep], clean[keep])


def test_the_torch_wrapper_takes_it():
    import torch

    from pydrobert_speech_amd.torch import PyTorchPostProcessorWrapper

    post = PLP(centers_hz=centers(23))
    x = rows_of(20, 23, np.float32)
    module = PyTorchPostProcessorWrapper(post)
    got = module(torch.from_numpy(x.copy()))
    assert tuple(got.shape) == (20, 13) and same_bits(got.cpu().numpy(), post.apply(x))
