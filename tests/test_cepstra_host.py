"""``post.Cepstra`` without a device: aliases, the host-built DCT-II / lifter matrix, the argument checks of
``pds_cepstra_rows_*`` (which come before any HIP call)."""
import numpy as np
import pytest

from pydrobert_speech_amd import _native
from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg
from pydrobert_speech_amd.post import Cepstra, PostProcessor

EPS = np.finfo(np.float64).eps
SHAPES = [(1, 1), (2, 2), (23, 13), (40, 13), (40, 40), (80, 80), (128, 128), (255, 3), (255, 255)]  # (F, K)


@pytest.mark.parametrize("alias", ["cepstra", "dct", "mfcc"])
def test_aliases_resolve(alias):
    post = alias_factory_subclass_from_arg(PostProcessor, alias)
    assert type(post) is Cepstra
    assert (post.num_ceps, post.lifter, post.norm, post.energy) == (13, 22.0, "ortho", False)
    post = alias_factory_subclass_from_arg(
        PostProcessor, {"name": alias, "num_ceps": 5, "lifter": None, "norm": None, "energy": True})
    assert (post.num_ceps, post.lifter, post.norm, post.energy) == (5, 0.0, None, True)


def test_exported_like_the_other_postprocessors():
    import pydrobert_speech_amd as ps

    assert "Cepstra" in ps.post.__all__ and ps.post.Cepstra is Cepstra


@pytest.mark.parametrize("norm", ["orth", "backward", 1, True])
def test_bad_norm_raises(norm):
    with pytest.raises(ValueError):
        Cepstra(norm=norm)


@pytest.mark.parametrize("num_ceps", [0, -1, 2.5, "13", None, True])
def test_bad_num_ceps_raises(num_ceps):
    with pytest.raises(ValueError):
        Cepstra(num_ceps=num_ceps)


@pytest.mark.parametrize("lifter", [-1.0, float("nan"), float("inf"), "22"])
def test_bad_lifter_raises(lifter):
    with pytest.raises(ValueError):
        Cepstra(lifter=lifter)


def test_width_bounds_are_checked_at_apply_before_any_device_work():
    # (the width is only known at apply; the check needs no device)
    with pytest.raises(ValueError, match="num_ceps"):
        Cepstra(13).apply(np.zeros((3, 12), dtype=np.float32))
    with pytest.raises(ValueError, match="num_ceps"):
        Cepstra(13, energy=True).apply(np.zeros((3, 13), dtype=np.float32))  # 12 filters beside the energy
    with pytest.raises(ValueError, match="num_ceps"):
        Cepstra(1).apply(np.zeros((3, 0), dtype=np.float32))
    with pytest.raises(ValueError, match="256"):
        Cepstra(13).apply(np.zeros((3, 257), dtype=np.float32))
    with pytest.raises(ValueError, match="num_ceps"):
        Cepstra(13).apply(np.zeros((5, 40), dtype=np.float32), axis=0)
    assert Cepstra(13).matrix(13)[0].shape == (13, 13)
    assert Cepstra(13, energy=True).matrix(14)[0].shape == (12, 13)


@pytest.mark.parametrize("norm", ["ortho", None])
@pytest.mark.parametrize("F,K", SHAPES)
def test_host_matrix_against_scipy(F, K, norm):
    fft = pytest.importorskip("scipy.fft")
    M, copy_cols = Cepstra(K, lifter=0, norm=norm).matrix(F)
    S = fft.dct(np.eye(F), type=2, norm=norm, axis=0)[:K]
    assert copy_cols == 0 and M.dtype == np.float64 and M.shape == S.shape == (K, F) and M.flags.c_contiguous
    # the cosine's argument reaches pi K and carries a few ulps of it
    bound = 8 * EPS * np.pi * K * np.abs(S).max()
    err = np.abs(M - S).max()
    print(f"F={F} K={K} norm={norm}: max |M - S| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("Q", [22.0, 22, 1.5, 100.0])
@pytest.mark.parametrize("norm", ["ortho", None])
def test_lifter_scales_the_rows(Q, norm):
    F, K = 40, 13
    plain, _ = Cepstra(K, lifter=0, norm=norm).matrix(F)
    lifted, _ = Cepstra(K, lifter=Q, norm=norm).matrix(F)
    k = np.arange(K, dtype=np.float64)
    lift = 1.0 + 0.5 * float(Q) * np.sin(np.pi * k / float(Q))
    assert np.array_equal(lifted, lift[:, None] * plain)
    assert np.array_equal(lifted[0], plain[0])  # (row 0 is never liftered: sin(0) = 0)
    none, _ = Cepstra(K, lifter=None, norm=norm).matrix(F)
    assert np.array_equal(none, plain)


@pytest.mark.parametrize("F", [1, 2, 23, 40, 128, 255])
def test_ortho_matrix_is_orthonormal(F):
    M, _ = Cepstra(F, lifter=0).matrix(F)
    assert np.abs(M @ M.T - np.eye(F)).max() <= 1e-13


@pytest.mark.parametrize("norm", ["ortho", None])
def test_energy_matrix_is_the_rows_behind_c0_of_the_narrower_table(norm):
    W, K = 41, 13
    M, copy_cols = Cepstra(K, lifter=22.0, norm=norm, energy=True).matrix(W)
    table, zero = Cepstra(K, lifter=22.0, norm=norm).matrix(W - 1)
    assert copy_cols == 1 and zero == 0 and M.shape == (K - 1, W - 1)
    assert np.array_equal(M, table[1:])
    only, copy_cols = Cepstra(1, energy=True).matrix(W)  # the energy alone: nothing to transform
    assert copy_cols == 1 and only.shape == (0, W - 1)


@pytest.mark.parametrize("name", ["pds_cepstra_rows_f32", "pds_cepstra_rows_f64"])
def test_c_entry_points_validate_arguments_without_a_device(name):
    lib = _native.lib()
    fn = getattr(lib, name)
    null = None
    one = np.zeros(1)  # (never dereferenced: every call below is refused, or has no rows)
    ptr = one.ctypes.data

    def refused(what, *args):
        assert fn(*args) == -1
        msg = lib.pds_last_error()
        assert msg.startswith(b"cepstra_rows: ") and what in msg, msg

    # d_in, in_stride, R, F, d_matrix, K, copy_cols, d_out, out_stride, stream
    refused(b"negative", ptr, 40, -1, 40, ptr, 13, 0, ptr, 13, null)
    refused(b"F / K", ptr, 40, 4, 0, ptr, 13, 0, ptr, 13, null)
    refused(b"F / K", ptr, 40, 4, 40, ptr, 0, 0, ptr, 13, null)
    refused(b"F / K", ptr, 40, 4, 40, ptr, 13, -1, ptr, 13, null)
    refused(b"stride", ptr, 39, 4, 40, ptr, 13, 0, ptr, 13, null)
    refused(b"stride", ptr, 40, 4, 40, ptr, 13, 1, ptr, 14, null)  # copy_cols + F = 41 in
    refused(b"stride", ptr, 40, 4, 40, ptr, 13, 0, ptr, 12, null)
    refused(b"stride", ptr, 41, 4, 40, ptr, 13, 1, ptr, 13, null)  # copy_cols + K = 14 out
    refused(b"wider", ptr, 300, 4, 257, ptr, 13, 0, ptr, 13, null)
    refused(b"wider", ptr, 300, 4, 256, ptr, 13, 1, ptr, 14, null)
    refused(b"wider", ptr, 1 << 40, 4, 2 ** 31 - 1, ptr, 13, 2 ** 31 - 1, ptr, 1 << 40, null)  # (no int32 wrap)
    refused(b"null pointer", null, 40, 4, 40, ptr, 13, 0, ptr, 13, null)
    refused(b"null pointer", ptr, 40, 4, 40, null, 13, 0, ptr, 13, null)
    refused(b"null pointer", ptr, 40, 4, 40, ptr, 13, 0, null, 13, null)
    # no rows: nothing to do, the pointers are not looked at -- but the sizes still are
    assert fn(null, 40, 0, 40, null, 13, 0, null, 13, null) == 0
    assert fn(null, 256, 0, 255, null, 255, 1, null, 256, null) == 0
    refused(b"F / K", null, 40, 0, 0, null, 13, 0, null, 13, null)


def test_the_staging_index_of_the_kernel_is_an_exact_integer_division():
    """``cepstra_rows_kernel`` fills its tile through ``lr = (unsigned)(((float)e + 0.5f) * rcpf(wd))`` and takes that
    for ``e / wd``: word e of a block's ``rows * wd`` staged words, ``wd`` = ``W`` 32-bit words per float32 row and
    ``2 W`` per float64 row, ``W <= 256``, at most 64 rows per block.  Swept here in float32 as the device computes it
    (``e + 0.5`` is exact below 2^23; one rounding of the product; truncation), for every ``wd`` in 1..512, every ``e``
    in ``[0, 64 wd)`` and every reciprocal within 2 ulp of the correctly rounded one -- the hardware's is specified
    to about 1 ulp."""
    checked = 0
    for wd in range(1, 513):
        e = np.arange(64 * wd, dtype=np.int64)
        half = e.astype(np.float32) + np.float32(0.5)
        assert half.dtype == np.float32 and (half.astype(np.float64) == e + 0.5).all()
        exact = np.float32(1.0) / np.float32(wd)  # (IEEE division: correctly rounded)
        assert exact.dtype == np.float32
        invs, lo, hi = [exact], exact, exact
        for _ in range(2):
            lo, hi = np.nextafter(lo, np.float32(0.0)), np.nextafter(hi, np.float32(2.0))
            invs += [lo, hi]
        assert len({float(v) for v in invs}) == 5 and all(v.dtype == np.float32 for v in invs)
        want = e // wd
        for inv in invs:
            prod = half * inv
            assert prod.dtype == np.float32
            lr = np.trunc(prod).astype(np.int64)
            bad = np.flatnonzero(lr != want)
            assert bad.size == 0, (wd, float(inv), int(bad[0]), int(lr[bad[0]]), int(want[bad[0]]))
            checked += len(e)
    assert checked == 5 * 64 * (512 * 513 // 2)
