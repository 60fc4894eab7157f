"""The offline post-processor kernels of csrc/post.hip at every launch shape they take: block, slab, phase and unroll
boundaries, grid-stride loops, batches of more than 65535 utterances, strided rows and non-finite values, bit for bit
against the separately rounded float64 restatements of tests/exact_post.py (checked on a CPU by
tests/test_exact_post.py).  Every expectation is computed here with numpy; nothing is read from a golden file."""
import contextlib

import numpy as np
import pytest

from pydrobert_speech_amd.post import Deltas, Stack, Standardize
from tests import exact_post as ex

pytestmark = pytest.mark.gpu


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def on_device(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def to_host(y):
    return y.cpu().numpy() if hasattr(y, "is_cuda") else y


# ------------------------------------------------------------------ 1. Deltas.apply -------

PADS = {"edge": {}, "reflect": {}, "symmetric": {}, "wrap": {}, "constant": {"constant_values": 0.1}}
FAMILY = [(1, 1), (2, 2), (3, 2), (2, 5)]


def delta_cases(K, W):
    """``(shape, time axis, target axis, concatenate)``: T in {1, 2, 2 K W, 2 K W + 1, 257}, and outer x T x inner at
    255, 256, 257 (the ends of a 256-thread block) and about 5000 (twenty blocks) in each of the three layouts"""
    r = 2 * K * W
    cases = []
    for T, F in [(1, 1), (1, 255), (2, 128), (257, 1), (r, 7), (r + 1, 5), (257, 19)]:
        cases.append(((T, F), 0, 1, True))  # (T, F) -> (T, (K + 1) F): outer = 1, inner = F, written in place
    for F, T in [(255, 1), (128, 2), (1, 257), (3, r), (5, r + 1), (19, 257)]:
        cases.append(((F, T), 1, 0, True))  # (F, T) -> ((K + 1) F, T): outer = F, inner = 1
    for T in (1, 2, r, r + 1, 17, 18, 257, 333):  # 15 T elements: 255 and 270 around a block's end, 3855, 4995
        cases.append(((3, T, 5), 1, 2, True))  # outer = 3, inner = 5, stacked by the kernel and laid out by torch
        cases.append(((3, T, 5), 1, 0, False))
    return cases


@pytest.mark.parametrize("pad", sorted(PADS))
@pytest.mark.parametrize("K,W", FAMILY)
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32, np.int16], ids=["f32", "f64", "i32", "i16"])
def test_deltas_apply_is_the_sequential_float64_sum(dtype, K, W, pad):
    """edge: the kernel clamps; reflect / symmetric / wrap: padded once by the widest reach; constant with a value:
    every order padded by its own reach on a float64 copy, one launch each"""
    rng = np.random.default_rng(1000 * K + 10 * W + len(pad))
    filts = ex.delta_filters(K, W)
    floating = np.dtype(dtype).kind == "f"
    for shape, axis, target, concatenate in delta_cases(K, W):
        x = (rng.standard_normal(shape) * 300 + 10).astype(dtype)
        want = ex.deltas_layout(ex.deltas_ref(x, axis, filts, pad, **PADS[pad]), target, concatenate)
        d = Deltas(K, context_window=W, target_axis=target, concatenate=concatenate, pad_mode=pad, **PADS[pad])
        got = d.apply(x, axis=axis)
        assert got.dtype == want.dtype and got.shape == want.shape, (shape, axis)
        assert np.array_equal(got, want), (shape, axis, target, "host array")
        if floating:  # (GPU tensors are float32 or float64)
            got = d.apply(on_device(x), axis=axis)
            assert got.is_cuda and same_bytes(got.cpu().numpy(), want), (shape, axis, target, "GPU tensor")


@pytest.mark.parametrize("pad", ["edge", "reflect", "constant"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_deltas_apply_carries_non_finite_samples_through_their_stencils_only(dtype, pad):
    K, W, T = 2, 2, 60
    reach = K * W
    filts = ex.delta_filters(K, W)
    rng = np.random.default_rng(5)
    clean = (rng.standard_normal((T, 6)) * 3 + 1).astype(dtype)
    x = clean.copy()
    x[10, 0] = np.nan
    x[25, 1] = np.inf
    x[40, 2], x[42, 2] = np.inf, -np.inf  # both inside the stencils of rows 38 .. 44: inf - inf
    touched = np.zeros((T, 6), dtype=bool)
    for t, c in ((10, 0), (25, 1), (40, 2), (42, 2)):
        touched[t - reach : t + reach + 1, c] = True
    d = Deltas(K, context_window=W, target_axis=1, pad_mode=pad, **PADS[pad])
    want = ex.deltas_layout(ex.deltas_ref(x, 0, filts, pad, **PADS[pad]), 1, True)
    want_clean = ex.deltas_layout(ex.deltas_ref(clean, 0, filts, pad, **PADS[pad]), 1, True)
    assert np.isnan(want[41, 2 * 6 + 2]) and np.isnan(want[10, 6]) and np.isinf(want[24, 6 + 1])
    for got in (d.apply(x, axis=0), d.apply(on_device(x), axis=0).cpu().numpy()):
        assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
        for k in range(K + 1):  # outside every affected stencil: the bits of the clean signal's result
            part, ref = got[:, k * 6 : (k + 1) * 6], want_clean[:, k * 6 : (k + 1) * 6]
            assert same_bytes(part[~touched], ref[~touched]) and np.isfinite(part[~touched]).all()


# ------------------------------------------------------------------ 2. global CMVN --------

ROWS = (1, 63, 64, 65, 128, 129, 8192, 8193)  # 64 rows per slab up to 128 slabs, then longer slabs
WIDTHS = (1, 63, 64, 65, 130)  # C * inner: 64 columns per block
SPLIT = {63: (7, 9), 64: (8, 8), 65: (5, 13), 130: (13, 10)}  # the same width as C coefficients x inner


def cmvn_cases():
    cases = []
    for rows in ROWS:
        for width in WIDTHS:
            cases.append(((rows, width), 1))
            if width in SPLIT:
                cases.append(((rows,) + SPLIT[width], 1))
    cases.append(((130, 7, 9), 1))
    return cases


def case_id(case):
    return "x".join(str(n) for n in case[0])


def integers(rng, shape):
    x = rng.integers(-ex.MAX_ABS, ex.MAX_ABS + 1, size=shape)
    x.reshape(-1)[:2] = (ex.MAX_ABS, -ex.MAX_ABS)[: x.size]
    return x


def zero_variance_warning(expected):
    return pytest.warns(UserWarning, match="0 variance encountered") if expected else contextlib.nullcontext()


@pytest.mark.parametrize("case", cmvn_cases(), ids=case_id)
def test_global_cmvn_of_integer_valued_input_is_exact(case):
    """accumulate (two chunks), apply with accumulated statistics and apply with the tensor's own: integer sums are
    exact in float64 in any order, so the statistics and every output bit are fixed whatever the slabs and phases"""
    shape, axis = case
    rng = np.random.default_rng(sum(shape))
    ints = integers(rng, shape)
    extra = ints[: max(1, shape[0] // 3)]
    count, extra_count = ints.size // shape[axis], extra.size // shape[axis]
    assert ex.exactness_holds(count + extra_count)  # (from the reference alone)
    s1, s2 = ex.exact_sums(ints, axis)
    e1, e2 = ex.exact_sums(extra, axis)
    t1, t2 = [a + b for a, b in zip(s1, e1)], [a + b for a, b in zip(s2, e2)]
    C = shape[axis]
    for dtype in (np.float32, np.float64, np.int16):
        for put in (np.asarray, on_device):
            x, x_extra = put(ints.astype(dtype)), put(extra.astype(dtype))
            for norm_var in (True, False):
                st = Standardize(norm_var=norm_var)
                st.accumulate(x, axis=axis)
                assert st._stats.shape == (2, C + 1) and st._stats[0, -1] == count
                assert st._stats[0, :-1].tolist() == s1 and st._stats[1, :-1].tolist() == s2, (dtype, "first chunk")
                st.accumulate(x_extra, axis=axis)
                assert st._stats[0, -1] == count + extra_count and st.have_stats
                assert st._stats[0, :-1].tolist() == t1 and st._stats[1, :-1].tolist() == t2, (dtype, "both chunks")
                flat = norm_var and bool(ex.scale_shift(t1, t2, count + extra_count)[2].any())
                with zero_variance_warning(flat):
                    got = st.apply(x, axis=axis)
                want = ex.cmvn_from_sums(ints, t1, t2, count + extra_count, norm_var, axis)
                assert same_bytes(to_host(got), want), (dtype, norm_var, "accumulated statistics")
                if count == 1:
                    continue  # (a lone vector has no statistics of its own: tests/test_gpu_post.py)
                flat = norm_var and bool(ex.scale_shift(s1, s2, count)[2].any())
                with zero_variance_warning(flat):
                    got = Standardize(norm_var=norm_var).apply(x, axis=axis)
                want = ex.cmvn_from_sums(ints, s1, s2, count, norm_var, axis)
                assert same_bytes(to_host(got), want), (dtype, norm_var, "own statistics")


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("rows", ROWS)
def test_global_cmvn_sums_of_random_input_stay_within_the_any_order_bound(rows, width):
    """float32 values (their squares are exact in float64): the two-stage sums against math.fsum within
    n * 2**-52 * sum |term|, the same bits on a second call, and the output from the kernel's own sums to the bit"""
    rng = np.random.default_rng(rows * 131 + width)
    x32 = (rng.standard_normal((rows, width)) * 3 + 1).astype(np.float32)
    f1, f2, a1, n = ex.fsum_columns(x32, axis=1)
    assert n == rows
    for dtype in (np.float32, np.float64):
        x = x32.astype(dtype)
        st, again = Standardize(), Standardize()
        st.accumulate(x)
        again.accumulate(on_device(x))
        g1, g2 = st._stats[0, :-1], st._stats[1, :-1]
        assert same_bytes(st._stats, again._stats)
        used = max(float((np.abs(g1 - f1) / ex.sum_bound(n, a1)).max()), float((np.abs(g2 - f2) / ex.sum_bound(n, f2)).max()))
        print(f"summation bound used at {rows} x {width} {np.dtype(dtype).name}: {used:.4f}")
        assert used <= 1.0, (rows, width, used)
        if rows > 1:
            got = Standardize().apply(x)
            assert same_bytes(got, ex.cmvn_from_sums(x, g1, g2, rows))
            assert same_bytes(Standardize().apply(on_device(x)).cpu().numpy(), got)
            assert same_bytes(st.apply(x), got)  # accumulated from the same tensor: the same sums, the same bits


def test_global_cmvn_in_place_on_a_contiguous_float64_gpu_tensor():
    rng = np.random.default_rng(7)
    ints = integers(rng, (129, 5, 13))
    s1, s2 = ex.exact_sums(ints, 1)
    want = ex.cmvn_from_sums(ints, s1, s2, 129 * 13, True, 1)
    x = on_device(ints.astype(np.float64))
    got = Standardize().apply(x, axis=1, in_place=True)
    assert got.data_ptr() == x.data_ptr() and same_bytes(x.cpu().numpy(), want)
    # a float32 tensor is not overwritten
    x = on_device(ints.astype(np.float32))
    got = Standardize().apply(x, axis=1, in_place=True)
    assert got.data_ptr() != x.data_ptr() and same_bytes(got.cpu().numpy(), want)
    assert same_bytes(x.cpu().numpy(), ints.astype(np.float32))


@pytest.mark.parametrize("put", [np.asarray, on_device], ids=["host", "gpu"])
def test_global_cmvn_constant_and_nan_coefficients_stay_alone(put):
    rng = np.random.default_rng(8)
    ints = integers(rng, (65, 6, 11))
    ints[:, 4] = 7  # a constant coefficient: variance 0 -> 1 with a warning, output 0
    s1, s2 = ex.exact_sums(ints, 1)
    want = ex.cmvn_from_sums(ints, s1, s2, 65 * 11, True, 1)
    assert ex.scale_shift(s1, s2, 65 * 11)[2].tolist() == [False] * 4 + [True, False]
    with pytest.warns(UserWarning, match="0 variance encountered"):
        got = to_host(Standardize().apply(put(ints.astype(np.float32)), axis=1))
    assert same_bytes(got, want) and not got[:, 4].any()
    x = ints.astype(np.float64)
    x[33, 2, 5] = np.nan  # one NaN sample: its coefficient is NaN everywhere, the others do not notice
    for norm_var in (True, False):
        with pytest.warns(UserWarning, match="0 variance encountered") if norm_var else contextlib.nullcontext():
            got = to_host(Standardize(norm_var=norm_var).apply(put(x), axis=1))
        keep = [0, 1, 3, 4, 5]
        want = ex.cmvn_from_sums(ints, s1, s2, 65 * 11, norm_var, 1)
        assert np.isnan(got[:, 2]).all() and same_bytes(got[:, keep], want[:, keep])


def test_global_cmvn_at_the_widest_tensor_the_grid_takes():
    """C * inner = 65535 * 64 fills the grid's y dimension; one more column is refused before any launch"""
    import torch

    Q = 65535 * 64
    base = torch.arange(Q, dtype=torch.int64, device="cuda")
    ints = torch.stack([base % 4001 - 2000, base % 4001 - 2000 + 1 + base % 7])  # (never two equal rows)
    x = ints.to(torch.float32)
    host = ints.cpu().numpy()
    assert ex.exactness_holds(2)
    s1, s2 = ex.exact_sums(host, 1)
    st = Standardize()
    st.accumulate(x)
    assert np.array_equal(st._stats[0, :-1], np.array(s1, dtype=np.float64))
    assert np.array_equal(st._stats[1, :-1], np.array(s2, dtype=np.float64)) and st._stats[0, -1] == 2
    got = Standardize().apply(x).cpu().numpy()
    assert same_bytes(got, ex.cmvn_from_sums(host, s1, s2, 2))
    del st, got
    wider = torch.zeros((2, Q + 1), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="too large"):
        Standardize().accumulate(wider)
    with pytest.raises(ValueError, match="too large"):
        Standardize().apply(wider)
    del x, wider, ints, base
    torch.cuda.empty_cache()  # (the sums' scratch is 128 slabs x 2 x Q float64)


# ------------------------------------------------------------------ 3. Standardize.apply_rows ----

RAGGED = [0, 1, 2, 15, 16, 17, 127, 128, 129, 255, 256, 257, 1000]  # 16 row phases, 8 loads of a thread in flight


def ragged_integers(C, seed):
    rng = np.random.default_rng(seed)
    rows = np.concatenate([[0], np.cumsum(RAGGED)])
    ints = integers(rng, (rows[-1], C))
    # constant columns: variance 0.  (Every column of the one-row utterance has it by itself.)
    ints[rows[5] : rows[6], 0] = -3
    ints[rows[8] : rows[9], C - 1] = 2048
    ints[rows[12] : rows[13], C // 2] = 0
    return ints, rows


@pytest.mark.parametrize("layout", ["contiguous", "column slice"])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 129])
def test_standardize_rows_is_exact_and_counts_zero_variances(C, layout):
    import torch

    ints, rows = ragged_integers(C, C)
    if layout == "contiguous":
        feats = on_device(ints.astype(np.float32))
    else:
        wide = torch.full((len(ints), C + 5), float("nan"), dtype=torch.float32, device="cuda")
        wide[:, 2 : 2 + C] = on_device(ints.astype(np.float32))
        feats = wide[:, 2 : 2 + C]
        assert feats.stride(0) == C + 5 and (feats.stride(1) == 1 or C == 1)
    for norm_var in (True, False):
        want, zeros, s1, s2 = ex.cmvn_rows_ref(ints, rows, norm_var)
        assert zeros >= (C + (3 if C > 1 else 1)) * norm_var
        for out_dtype, cast in ((None, np.float64), (torch.float64, np.float64), (torch.float32, np.float32)):
            st = Standardize(norm_var=norm_var)
            got = st.apply_rows(feats, rows, out_dtype=out_dtype)
            assert got.shape == (len(ints), C)
            got, ref = got.cpu().numpy(), want.astype(cast)
            wrong = [T for b, T in enumerate(RAGGED) if not same_bytes(got[rows[b] : rows[b + 1]], ref[rows[b] : rows[b + 1]])]
            assert not wrong, (norm_var, cast, "utterances of these lengths differ", wrong)
            assert st._last_zero_var.item() == zeros, (norm_var, cast)


def test_standardize_rows_nan_column_stays_alone_and_is_not_counted():
    C = 65
    ints, rows = ragged_integers(C, 99)
    want, zeros, _, _ = ex.cmvn_rows_ref(ints, rows)
    x = ints.astype(np.float32)
    x[rows[9] + 100, 64] = np.nan  # utterance 9 (255 rows), the one column of the second 64-column block
    x[rows[5] + 3, 0] = np.nan  # ... and in a column that had zero variance: no longer counted
    st = Standardize()
    got = st.apply_rows(on_device(x), rows).cpu().numpy()
    hit = np.zeros(x.shape, dtype=bool)
    hit[rows[9] : rows[10], 64] = True
    hit[rows[5] : rows[6], 0] = True
    assert np.isnan(got[hit]).all() and same_bytes(got[~hit], want[~hit])
    assert st._last_zero_var.item() == zeros - 1


def many_short(F, seed, longest=3):
    rng = np.random.default_rng(seed)
    B = 65535 + 3
    nrows = rng.integers(1, longest + 1, size=B)
    nrows[-3:] = (longest, 1, 2)  # the second call's utterances
    rows = np.concatenate([[0], np.cumsum(nrows)])
    return integers(rng, (rows[-1], F)), rows


def test_standardize_rows_beyond_one_calls_utterances():
    ints, rows = many_short(3, 31)
    want, zeros, _, _ = ex.cmvn_rows_ref(ints, rows)
    st = Standardize()
    got = st.apply_rows(on_device(ints.astype(np.float32)), rows)
    assert same_bytes(got.cpu().numpy(), want) and st._last_zero_var.item() == zeros
    assert zeros > 3 * 20000  # (the one-row utterances)


# ------------------------------------------------------------------ 4. Deltas.apply_rows --------


def deltas_rows_ref(feats, rows, filts):
    """edge-padded deltas per utterance, appended per row; utterances of one length go through deltas_ref together"""
    feats = np.asarray(feats)
    rows = np.asarray(rows, dtype=np.int64)
    nrows = np.diff(rows)
    out = np.zeros((feats.shape[0], (len(filts) + 1) * feats.shape[1]), dtype=feats.dtype)
    for T in np.unique(nrows):
        if T == 0:
            continue
        at = rows[:-1][nrows == T][:, None] + np.arange(T)[None, :]
        out[at] = np.concatenate(ex.deltas_ref(feats[at], 1, filts), axis=2)
    return out


def test_deltas_rows_beyond_one_calls_utterances():
    ints, rows = many_short(5, 41)
    feats = (ints / 8).astype(np.float32)
    got = Deltas(2).apply_rows(on_device(feats), rows)
    assert same_bytes(got.cpu().numpy(), deltas_rows_ref(feats, rows, ex.delta_filters(2, 2)))


def test_deltas_rows_long_utterance_over_many_workgroup_groups():
    """5000 rows x 40 coefficients: 98 workgroups of 8-row threads, launched as 13 groups of 8 and renumbered so that
    a group's workgroups cover one stretch of rows; beside a short utterance whose spare workgroups leave at once"""
    rng = np.random.default_rng(43)
    rows = np.array([0, 9, 5009, 5010])
    feats = (rng.standard_normal((rows[-1], 40)) * 3 + 1).astype(np.float32)
    got = Deltas(2).apply_rows(on_device(feats), rows)
    assert same_bytes(got.cpu().numpy(), deltas_rows_ref(feats, rows, ex.delta_filters(2, 2)))


@pytest.mark.parametrize("K,W,F", [(3, 3, 323), (4, 2, 361)])
def test_deltas_rows_tiled_kernel_at_its_width_limit(K, W, F):
    """no register-window form: the LDS tile of 24 KB holds 2 K W + 1 rows of F floats and no more"""
    import torch

    rng = np.random.default_rng(F)
    rows = np.concatenate([[0], np.cumsum([1, 2, 2 * K * W, 2 * K * W + 1, 45])])
    feats = (rng.standard_normal((rows[-1], F + 1)) * 3 + 1).astype(np.float32)
    d = Deltas(K, context_window=W)
    got = d.apply_rows(on_device(feats[:, :F].copy()), rows)
    assert same_bytes(got.cpu().numpy(), deltas_rows_ref(feats[:, :F], rows, ex.delta_filters(K, W)))
    out = torch.full((rows[-1], (K + 1) * (F + 1)), float("nan"), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="rows too wide"):
        d.apply_rows(on_device(feats), rows, out=out)
    assert bool(torch.isnan(out).all())


def test_deltas_rows_refuses_an_out_it_would_overrun():
    import torch

    K, F, R = 2, 6, 20
    rows = [0, 7, 20]
    feats = torch.ones((R, F), dtype=torch.float32, device="cuda")
    d = Deltas(K)
    width = (K + 1) * F
    good = torch.full((R + 2, width + 3), -7.0, dtype=torch.float32, device="cuda")
    assert d.apply_rows(feats, rows, out=good) is good
    want = deltas_rows_ref(np.ones((R, F), dtype=np.float32), rows, ex.delta_filters(K, 2))
    host = good.cpu().numpy()
    assert same_bytes(host[:R, :width], want) and (host[R:] == -7.0).all() and (host[:, width:] == -7.0).all()
    bad = {
        "float64": torch.zeros((R, width), dtype=torch.float64, device="cuda"),
        "host tensor": torch.zeros((R, width), dtype=torch.float32),
        "numpy array": np.zeros((R, width), dtype=np.float32),
        "too few rows": torch.zeros((R - 1, width), dtype=torch.float32, device="cuda"),
        "too few columns": torch.zeros((R, width - 1), dtype=torch.float32, device="cuda"),
        "one dimension": torch.zeros(R * width, dtype=torch.float32, device="cuda"),
        "strided columns": torch.zeros((width, R), dtype=torch.float32, device="cuda").t(),
        "overlapping rows": torch.zeros(R * width, dtype=torch.float32, device="cuda").as_strided((R, width), (width - 1, 1)),
        "repeated row": torch.zeros((1, width), dtype=torch.float32, device="cuda").expand(R, width),
    }
    for what, out in bad.items():
        with pytest.raises(ValueError, match="out must be"):
            d.apply_rows(feats, rows, out=out)
        if hasattr(out, "is_cuda"):
            assert not bool(out.any()), what


def test_deltas_rows_carry_non_finite_samples_through_their_stencils_only():
    K, W, F = 2, 2, 6
    reach = K * W
    filts = ex.delta_filters(K, W)
    rng = np.random.default_rng(6)
    rows = np.array([0, 5, 65, 72])
    clean = (rng.standard_normal((rows[-1], F)) * 3 + 1).astype(np.float32)
    x = clean.copy()
    base = rows[1]
    x[base + 10, 0] = np.nan
    x[base + 25, 1] = np.inf
    x[base + 40, 2], x[base + 42, 2] = np.inf, -np.inf
    x[base + 58, 3] = np.inf  # near the utterance's end: must not reach the next utterance
    touched = np.zeros(x.shape, dtype=bool)
    for t, c in ((10, 0), (25, 1), (40, 2), (42, 2), (58, 3)):
        touched[base + max(t - reach, 0) : min(base + t + reach + 1, rows[2]), c] = True
    want, want_clean = deltas_rows_ref(x, rows, filts), deltas_rows_ref(clean, rows, filts)
    got = Deltas(K, context_window=W).apply_rows(on_device(x), rows).cpu().numpy()
    assert np.array_equal(got, want, equal_nan=True) and np.isnan(want[base + 41, 2 * F + 2])
    for k in range(K + 1):
        part, ref = got[:, k * F : (k + 1) * F], want_clean[:, k * F : (k + 1) * F]
        assert same_bytes(part[~touched], ref[~touched]) and np.isfinite(part[~touched]).all()


# ------------------------------------------------------------------ 5. Stack.apply_rows ---------


@pytest.mark.parametrize("pad_mode", [None, "constant", "edge"])
def test_stack_rows_beyond_one_calls_utterances_moves_bytes(pad_mode):
    nv, F = 3, 4
    rng = np.random.default_rng(51)
    B = 65535 + 3
    nrows = rng.integers(0, 8, size=B)  # (empty utterances among them)
    planted = ((0, 0x7FC12345), (1, 0xFF800001), (2, 0x80000000), (B - 1, 0x7FC00BAD), (B - 3, 0x80000000))
    nrows[[b for b, _ in planted]] = (6, 7, 6, 7, 6)
    rows = np.concatenate([[0], np.cumsum(nrows)])
    words = integers(rng, (rows[-1], F)).astype(np.float32).view(np.uint32).copy()
    # bits an arithmetic instruction would not keep: NaNs with payloads (one signalling) and negative zeros, in the
    # first utterances and in the second call's, in first rows and in last rows (which "edge" repeats for 7 rows)
    for b, word in planted:
        words[rows[b + 1] - 1, b % F] = word
        words[rows[b], (b + 1) % F] = word
    feats = words.view(np.float32)
    got, new_rows = Stack(nv, pad_mode=pad_mode).apply_rows(on_device(feats), rows)
    out_rows = (nrows + nv - 1) // nv if pad_mode else nrows // nv
    assert np.array_equal(new_rows, np.concatenate([[0], np.cumsum(out_rows)]))
    want = np.zeros((new_rows[-1], nv * F), dtype=np.uint32)
    for T in np.unique(nrows):
        which = nrows == T
        if not out_rows[which][0]:
            continue
        t = np.arange(out_rows[which][0] * nv)
        src = words[rows[:-1][which][:, None] + np.minimum(t, T - 1)[None, :]]  # (n, padded T, F)
        if pad_mode == "constant":
            src[:, t >= T] = 0
        at = new_rows[:-1][which][:, None] + np.arange(out_rows[which][0])[None, :]
        want[at] = src.reshape(len(src), -1, nv * F)
    got = got.cpu().numpy()
    assert same_bytes(got.view(np.uint32), want)
    assert (want == 0x7FC12345).sum() >= 1 and (want == 0x80000000).sum() >= 2


# ------------------------------------------------------------------ the 262144-block loops ------

LARGE = 262144 * 256 + 1000  # one more than the grid's cap of 256-thread blocks: the grid-stride loops turn once
SLICES = (0, 262144 * 256 - 3600, LARGE - 4096)  # the start, a span straddling the loop's first stride, the end
assert all(lo % 8 == 0 and lo + 4096 <= LARGE for lo in SLICES)


def large_vector():
    import torch

    return (torch.arange(LARGE, dtype=torch.int64, device="cuda") % 4001 - 2000).to(torch.float32)


@pytest.mark.slow
def test_deltas_apply_beyond_the_grid_cap():
    import torch

    x = large_vector()
    got = Deltas(1, context_window=1).apply(x)
    assert got.shape == (2 * LARGE,) and got.dtype == torch.float32
    filts = ex.delta_filters(1, 1)
    for lo in SLICES:
        a, b = max(lo - 1, 0), min(lo + 4096 + 1, LARGE)  # the slice with its halo; "edge" only at the vector's ends
        ref = ex.deltas_ref(x[a:b].cpu().numpy(), 0, filts)[1][lo - a : lo - a + 4096]
        assert same_bytes(got[LARGE + lo : LARGE + lo + 4096].cpu().numpy(), ref), lo
        assert torch.equal(got[lo : lo + 4096], x[lo : lo + 4096])
    del got, x
    torch.cuda.empty_cache()


@pytest.mark.slow
def test_global_cmvn_apply_beyond_the_grid_cap():
    """the vector as (LARGE / 8, 8): 2**23 terms per coefficient, 128 slabs of 65537 rows, integer sums exact"""
    import torch

    x = large_vector().reshape(-1, 8)
    assert ex.exactness_holds(len(x)) and len(x) < 2 ** 24
    s1 = x.to(torch.int64).sum(0).tolist()
    s2 = (x.to(torch.int64) ** 2).sum(0).tolist()
    st = Standardize(norm_var=False)
    st.accumulate(x)
    assert st._stats[0, :-1].tolist() == s1 and st._stats[1, :-1].tolist() == s2 and st._stats[0, -1] == len(x)
    got = st.apply(x)
    assert got.shape == x.shape and got.dtype == torch.float64
    flat = got.reshape(-1)
    for lo in SLICES:
        assert lo % 8 == 0
        rows = x[lo // 8 : lo // 8 + 512].cpu().numpy()
        want = ex.cmvn_from_sums(rows, s1, s2, len(x), norm_var=False)
        assert same_bytes(flat[lo : lo + 4096].cpu().numpy(), want.reshape(-1)), lo
    del got, flat, x
    torch.cuda.empty_cache()
