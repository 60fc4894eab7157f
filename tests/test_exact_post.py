"""The references of tests/test_gpu_post_shapes.py (tests/exact_post.py) checked on their own: CPU only."""
import numpy as np
import pytest

from oracle import stft_oracle as orc
from tests import exact_post as ex

# the shapes of the global CMVN tests: rows (terms per coefficient, times `inner`) and C * inner
ROWS = (1, 63, 64, 65, 128, 129, 8192, 8193)
WIDTHS = (1, 63, 64, 65, 130)
LARGE = 262144 * 256 + 1000  # elements of the two `slow` cases, standardised as (LARGE / 8, 8)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32, np.int16])
@pytest.mark.parametrize("K,W", [(1, 1), (2, 2), (3, 2), (2, 5)])
def test_deltas_ref_reproduces_the_oracle_bit_for_bit(dtype, K, W):
    rng = np.random.default_rng(10 * K + W)
    filts = ex.delta_filters(K, W)
    for want, got in zip(orc.delta_filters(K, W)[1:], filts):
        assert np.array_equal(want, got)
    for shape, axis, target in [((1, 3), 0, 1), ((3, 1), 0, 1), ((20, 50), 0, 1), ((7, 2 * K * W + 1), 1, 0),
                                ((3, 33, 5), 1, 2), ((3, 33, 5), 1, 0)]:
        x = (rng.random(shape) * 200 - 100).astype(dtype)
        got = ex.deltas_layout(ex.deltas_ref(x, axis, filts), target, True)
        want = orc.deltas(x, axis=axis, num_deltas=K, context_window=W, target_axis=target)
        assert got.dtype == want.dtype == np.dtype(dtype) and np.array_equal(got, want), (shape, axis)
        got = ex.deltas_layout(ex.deltas_ref(x, axis, filts, "edge"), target, False)
        want = orc.deltas(x, axis=axis, num_deltas=K, context_window=W, target_axis=target, concatenate=False)
        assert np.array_equal(got, want), (shape, axis)


@pytest.mark.parametrize("mode", ["reflect", "symmetric", "wrap"])
def test_padding_once_by_the_widest_reach_gives_every_order_its_own_padding(mode):
    """what Deltas.apply relies on for the modes that copy samples: a narrower numpy.pad is a slice of a wider one"""
    for T in (1, 2, 3, 8, 9, 21, 257):
        x = np.arange(T, dtype=np.float64) + 1
        for widest in (1, 4, 6, 10):
            wide = np.pad(x, (widest, widest), mode)
            for reach in range(1, widest + 1):
                assert np.array_equal(np.pad(x, (reach, reach), mode), wide[widest - reach : widest + T + reach])


def test_integer_sums_are_exact_in_float64_at_every_shape_of_the_tests():
    for rows in ROWS:
        assert ex.exactness_holds(2 * rows * 10)  # (inner up to 10, statistics accumulated twice)
    assert ex.exactness_holds(2)  # 65535 * 64 columns of two rows
    assert LARGE % 8 == 0 and ex.exactness_holds(LARGE // 8)
    assert ex.exactness_holds(2 ** 24) and not ex.exactness_holds(2 ** 31)
    # the largest shape: numpy's own float64 sums, in its pairwise order, equal the integer sums
    rng = np.random.default_rng(0)
    x = rng.integers(-ex.MAX_ABS, ex.MAX_ABS + 1, size=(8193, 130)).astype(np.float64)
    x[0, 0], x[1, 0] = ex.MAX_ABS, -ex.MAX_ABS
    s1, s2 = ex.exact_sums(x, axis=1)
    assert all(isinstance(v, int) for v in s1 + s2)
    assert np.array_equal(x.sum(axis=0), np.array(s1, dtype=np.float64))
    assert np.array_equal((x * x).sum(axis=0), np.array(s2, dtype=np.float64))
    assert np.array_equal(np.cumsum(x[:, 3])[-1:], [float(s1[3])])  # ... and in sequential order
    with pytest.raises(AssertionError):
        ex.exact_sums(x + 0.5, axis=1)
    # inner > 1: the coefficient axis in the middle
    x3 = rng.integers(-ex.MAX_ABS, ex.MAX_ABS + 1, size=(130, 7, 9))
    s1, s2 = ex.exact_sums(x3, axis=1)
    assert s1 == [int(x3[:, c].sum()) for c in range(7)] and s2 == [int((x3[:, c] ** 2).sum()) for c in range(7)]


def test_numpys_own_sums_of_random_inputs_stay_within_the_any_order_bound():
    rng = np.random.default_rng(1)
    for rows, width in [(1, 65), (2, 130), (65, 65), (129, 130), (8193, 130)]:
        x = (rng.standard_normal((rows, width)) * 3 + 1).astype(np.float32)
        s1, s2, a1, n = ex.fsum_columns(x, axis=1)
        assert n == rows
        wide = x.astype(np.float64)
        for got, want, mass in ((wide.sum(axis=0), s1, a1), ((wide * wide).sum(axis=0), s2, s2),
                                (np.cumsum(wide, axis=0)[-1], s1, a1)):
            err, bound = np.abs(got - want), ex.sum_bound(n, mass)
            assert (err <= bound).all(), (rows, width, float((err / bound).max()))
    # a float32 accumulator is far outside it
    x = (rng.standard_normal((8193, 4)) * 3 + 1).astype(np.float32)
    s1, _, a1, n = ex.fsum_columns(x, axis=1)
    assert (np.abs(np.cumsum(x, axis=0, dtype=np.float32)[-1].astype(np.float64) - s1) > ex.sum_bound(n, a1)).all()


def test_cmvn_from_sums_is_the_oracles_normalisation():
    rng = np.random.default_rng(2)
    x = rng.integers(-ex.MAX_ABS, ex.MAX_ABS + 1, size=(65, 4, 3)).astype(np.float32)
    x[:, 2] = 7.0  # a constant coefficient: variance 0 -> 1, output 0
    s1, s2 = ex.exact_sums(x, axis=1)
    for norm_var in (True, False):
        got = ex.cmvn_from_sums(x, s1, s2, 65 * 3, norm_var, axis=1)
        want = orc.cmvn_local(x, axis=1, norm_var=norm_var)
        assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-12, atol=1e-12)
        assert not got[:, 2].any()
    assert ex.scale_shift(s1, s2, 65 * 3)[2].tolist() == [False, False, True, False]
    # packed rows: one count per utterance, empty utterances, and the pairs counted
    rows = np.array([0, 0, 1, 18, 18, 65])
    flat = x[:, :, 0].copy()
    flat[18:, 1] = 5.0
    y, zeros, r1, r2 = ex.cmvn_rows_ref(flat, rows)
    assert zeros == 4 + 1 + 2  # every column of the one-row utterance, column 2 of the next, columns 1 and 2 of the last
    for b in range(5):
        part = flat[rows[b] : rows[b + 1]]
        if len(part):
            s1, s2 = ex.exact_sums(part, axis=1)
            assert r1[b].tolist() == s1 and r2[b].tolist() == s2
            assert np.array_equal(y[rows[b] : rows[b + 1]], ex.cmvn_from_sums(part, s1, s2, len(part)))
    assert ex.cmvn_rows_ref(flat, rows, norm_var=False)[1] == 0


def test_slab_arithmetic_of_the_two_stage_sum():
    """csrc/post.hip: slabs_for gives min(ceil(rows / 64), 128) slabs, cmvn_partial_kernel ceil(rows / slabs) rows each"""
    assert ex.slabs_for(1) == (1, 1) and ex.slabs_for(63) == (1, 63) and ex.slabs_for(64) == (1, 64)
    assert ex.slabs_for(65) == (2, 33)
    assert ex.slabs_for(128) == (2, 64)
    assert ex.slabs_for(129) == (3, 43)
    assert ex.slabs_for(8192) == (128, 64)
    slabs, length = ex.slabs_for(8193)
    assert (slabs, length) == (128, 65)
    assert (slabs - 1) * length >= 8193 > (slabs - 2) * length  # the last of the 128 slabs is empty
    for rows in ROWS + (LARGE // 8,):
        slabs, length = ex.slabs_for(rows)
        assert 1 <= slabs <= 128 and slabs * length >= rows  # every row belongs to a slab
