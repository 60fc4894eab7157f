"""``cepstra_rows_kernel`` (csrc/post.hip) at every launch shape it takes, against :func:`tests.test_gpu_cepstra.emulate`
byte for byte.

The kernel is driven through ``pds_cepstra_rows_f32`` / ``_f64`` with buffers of the test's own, so that shapes the
``Cepstra`` class never makes run too (a matrix that is no DCT, ``K > F``, ``copy_cols`` up to ``W - 1``): every row
width ``W = copy + F`` in 1..256 for both row types -- every divisor ``wd`` in 1..512 of the staging index, whose
proof is ``tests/test_cepstra_host.py`` --, two full blocks and one row of a third, and the row counts around a
block's rows at the widths where the rows per block change.  What the kernel must not read is NaN (pad columns of a
strided input, the row behind the last); what it must not write is random and compared afterwards."""
import numpy as np
import pytest

from pydrobert_speech_amd import _native
from tests.test_gpu_cepstra import emulate

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
LEAD, TRAIL = 2, 3  # columns of the output buffer on either side of the kernel's


def rows_per_block(W):
    """launch_cepstra's: 64 rows, halved until the float64 tile at the odd pitch ``W | 1`` fits 64 KB"""
    rb = 64
    while rb * (W | 1) * 8 > 64 * 1024:
        rb >>= 1
    return rb


def sweep_case(W, d):
    """``(copy, K)`` of width `W` and row type `d` (0: float32, 1: float64) in the sweep"""
    copies = sorted({0, min(1, W - 1), W - 1})
    copy = copies[(W + d) % len(copies)]
    F = W - copy
    Ks = [1, 2, 3, 4, F + 3 if F <= 24 else 6, 13, F if F <= 64 else 7, 5]
    return copy, Ks[(W // 3 + 3 * d) % len(Ks)]


def run(W, copy, K, R, dtype, stride, rng):
    """one launch: `R` rows of `W` columns at row stride `stride`, a random ``[K][W - copy]`` matrix, the output in
    columns ``LEAD .. LEAD + copy + K`` of a wider buffer with a row behind the last.  Asserts every byte."""
    import torch

    lib = _native.lib()
    fn = lib.pds_cepstra_rows_f32 if dtype == np.float32 else lib.pds_cepstra_rows_f64
    F = W - copy
    x = (20 * rng.standard_normal((R, W)) - 5).astype(dtype)
    M = rng.standard_normal((K, F))
    buf = np.full((R + 1, stride), np.nan, dtype=dtype)  # pad columns and the row behind the last: NaN
    buf[:R, :W] = x
    width = LEAD + copy + K + TRAIL
    before = rng.standard_normal((R + 1, width)).astype(dtype)
    d_in, d_M, d_out = torch.from_numpy(buf).cuda(), torch.from_numpy(M).cuda(), torch.from_numpy(before).cuda()
    rc = fn(d_in.data_ptr(), stride, R, F, d_M.data_ptr(), K, copy, d_out.data_ptr() + LEAD * d_out.element_size(),
            width, torch.cuda.current_stream().cuda_stream)
    _native.check(rc, "pds_cepstra_rows")
    want = before.copy()
    want[:R, LEAD : LEAD + copy + K] = emulate(x, M, copy)
    assert np.isfinite(want).all()
    got = d_out.cpu().numpy()
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint8).reshape(R + 1, -1) != want.view(np.uint8).reshape(R + 1, -1))
        r, c = int(bad[0][0]), int(bad[0][1]) // got.itemsize
        raise AssertionError(f"W={W} copy={copy} K={K} R={R} {np.dtype(dtype).name} stride={stride}: first difference "
                             f"at row {r}, buffer column {c}: {got[r, c]!r} for {want[r, c]!r}; "
                             f"{len({(int(a), int(b) // got.itemsize) for a, b in bad})} elements differ")
    assert d_in.cpu().numpy().tobytes() == buf.tobytes()  # (the input is left alone)


def test_the_sweep_reaches_every_case_it_is_there_for():
    # (no device work: the cases of test_every_width, counted)
    assert [rows_per_block(W) for W in (1, 127, 128, 255, 256)] == [64, 64, 32, 32, 16]
    cases = [(W,) + sweep_case(W, d) for W in range(1, 257) for d in (0, 1)]
    assert all(0 <= copy < W and K >= 1 for W, copy, K in cases)
    assert {copy + K for _, copy, K in cases} >= {1, 2, 3} and {(copy + K) % 4 for _, copy, K in cases} == {0, 1, 2, 3}
    assert {(W - copy) % 4 for W, copy, _ in cases} == {0, 1, 2, 3}
    assert sum(K > W - copy for W, copy, K in cases) >= 20
    for d in (0, 1):
        mine = [(W,) + sweep_case(W, d) for W in range(1, 257)]
        assert any(copy == 0 for _, copy, _ in mine) and any(copy == 1 < W - 1 for W, copy, _ in mine)
        assert any(copy == W - 1 > 1 for W, copy, _ in mine)
        for rb in (64, 32):  # (16: the one width 256)
            assert {sweep_case(W, d)[0] == 0 for W in range(1, 256) if rows_per_block(W) == rb} == {False, True}


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_every_width(dtype):
    """W = 1..256: two full blocks and the first row of a third; rows at stride W and at stride W + 3"""
    d = DTYPES.index(dtype)
    rng = np.random.default_rng(11 + d)
    launches = 0
    for W in range(1, 257):
        rb = rows_per_block(W)
        assert rb == (64 if W <= 127 else 32 if W <= 255 else 16)
        copy, K = sweep_case(W, d)
        for stride in (W, W + 3):
            run(W, copy, K, 2 * rb + 1, dtype, stride, rng)
            launches += 1
    assert launches == 512


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_row_counts_around_a_block(dtype):
    """rb - 1, rb and rb + 1 rows where rb changes: 64 rows per block at W = 127, 32 at 128 and 255, 16 at 256"""
    rng = np.random.default_rng(13 + DTYPES.index(dtype))
    for W, rb in ((127, 64), (128, 32), (255, 32), (256, 16)):
        assert rows_per_block(W) == rb
        for R in (rb - 1, rb, rb + 1):
            for copy, K in ((0, 5), (1, 6)):
                run(W, copy, K, R, dtype, W + 3, rng)
