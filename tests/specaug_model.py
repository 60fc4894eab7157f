"""The definition of ``post.SpecAugment`` in numpy (its class docstring and include/pds_amd_stages3.h have the text):
the reference every SpecAugment test compares with.  Philox4x32-10 on uint64 arrays that hold 32-bit words, ``U``, the
plan vectorised over utterances, the 64 interleaved partial sums of the mean, the warp and the masks.  Every float64
operation is a numpy ufunc call of its own and so rounded once.  The keys come from ``pre`` (``dither_keys``,
``_next_key``, ``_seed_state``): one rule turns a seed into a key."""
import numpy as np

from pydrobert_speech_amd.post import SpecAugment
from pydrobert_speech_amd.pre import _next_key, _seed_state, dither_keys  # noqa: F401  (re-exported for the tests)
from tests.pcen_model import same_bits  # noqa: F401  (NaNs at the same places, every other element bit for bit)

M32 = np.uint64(0xFFFFFFFF)


def philox(counter, key):
    """Philox4x32-10: `counter` ``(..., 4)`` and `key` ``(..., 2)`` of 32-bit words -> ``(..., 4)`` uint64 words"""
    c = [np.asarray(counter, dtype=np.uint64)[..., k] & M32 for k in range(4)]
    k0, k1 = (np.asarray(key, dtype=np.uint64)[..., k] & M32 for k in range(2))
    c = list(np.broadcast_arrays(*c, k0, k1)[:4])
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, axis=-1)


def draw(i, d, keys):
    """``P(i, d)`` under every key of uint64 `keys`: ``(B, 4)``"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
    zero = np.zeros_like(keys)
    counter = np.stack([zero + np.uint64(i), zero, zero + np.uint64(d), zero], axis=-1)
    return philox(counter, np.stack([keys & M32, keys >> np.uint64(32)], axis=-1))


def uniform(r, n):
    """``U(r, n)``: int64 in [0, n], elementwise"""
    r, n = np.asarray(r, dtype=np.uint64), np.asarray(n, dtype=np.int64)
    assert (n >= 0).all() and (n < (1 << 31)).all()
    return ((r * (n + 1).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)


def plan_model(post: SpecAugment, nrows, C, keys) -> np.ndarray:
    """steps 1 to 3 for B utterances: int64 ``(B, 2 + 2 F + 2 N)``"""
    T = np.asarray(nrows, dtype=np.int64).reshape(-1)
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
    B, F, N, W = len(T), post.freq_masks, post.time_masks, post.warp
    plan = np.zeros((B, 2 + 2 * F + 2 * N), dtype=np.int64)
    plan[:, :2] = -1
    live = T > 0
    Ts = np.where(live, T, 1)  # (an empty utterance is computed as one row and then left out)
    if W >= 1:
        r = draw(0, 1, keys)
        warped = live & (T >= 2 * W + 3)
        w0 = W + 1 + uniform(r[:, 0], np.where(warped, T - 3 - 2 * W, 0))
        w1 = w0 - W + uniform(r[:, 1], 2 * W)
        plan[warped, 0], plan[warped, 1] = w0[warped], w1[warped]
    for j in range(F):
        r = draw(j, 2, keys)
        f = uniform(r[:, 0], min(post.freq_width, C))
        f0 = uniform(r[:, 1], C - f)
        plan[live, 2 + 2 * j], plan[live, 3 + 2 * j] = f0[live], f[live]
    scaled = np.float64(post.time_ratio) * Ts.astype(np.float64)  # the product rounded once
    bound = np.minimum(np.int64(post.time_width), np.floor(scaled).astype(np.int64))
    for j in range(N):
        r = draw(j, 3, keys)
        t = uniform(r[:, 0], bound)
        t0 = uniform(r[:, 1], Ts - t)
        plan[live, 2 + 2 * F + 2 * j], plan[live, 3 + 2 * F + 2 * j] = t0[live], t[live]
    return plan


def mean_model(x) -> np.float64:
    """step 5 for one utterance `x` ``(T, C)``: float64 (NaN for an empty one)"""
    flat = np.asarray(x).astype(np.float64).reshape(-1)
    n = len(flat)
    with np.errstate(all="ignore"):
        # lane j owns e = j, j + 64, ...; a partial sum never is -0.0 (it starts from +0.0), so the +0.0 that pads the
        # last row of the table changes nothing
        table = np.zeros((-(-n // 64) + 1, 64), dtype=np.float64)
        table[1:].reshape(-1)[:n] = flat
        p = np.cumsum(table, axis=0)[-1]  # (accumulate adds in order, one rounding each)
        s = np.cumsum(np.concatenate([[0.0], p]))[-1]
        return np.float64(s) / np.float64(n)


def source_model(T, w0, w1):
    """step 4's ``(i, a)`` of every row of an utterance of T rows warped at (w0, w1)"""
    t = np.arange(T, dtype=np.int64)
    tf = t.astype(np.float64)
    with np.errstate(all="ignore"):
        front = (tf * np.float64(w0)) / np.float64(w1)
        back = np.float64(w0) + ((t - w1).astype(np.float64) * np.float64(T - 1 - w0)) / np.float64(T - 1 - w1)
    s = np.where(t <= w1, front, back)
    i = np.floor(s)
    return i.astype(np.int64), s - i


def apply_model(post: SpecAugment, x, plan_row, mean=None) -> np.ndarray:
    """steps 4 and 6 for one utterance `x` ``(T, C)`` of float32 or float64 under its row of the plan"""
    x = np.asarray(x)
    T, C = x.shape
    F, N = post.freq_masks, post.time_masks
    plan_row = [int(v) for v in plan_row]
    w0, w1 = plan_row[:2]
    out = x.copy()
    if T and 1 <= w0 <= T - 2 and 1 <= w1 <= T - 2:
        i, a = source_model(T, w0, w1)
        assert (i >= 0).all() and (i[a > 0] + 1 <= T - 1).all()
        out = x[i].copy()  # (a == 0: copied)
        mix = a != 0
        with np.errstate(all="ignore"):
            lo, hi = x[i[mix]].astype(np.float64), x[np.minimum(i[mix] + 1, T - 1)].astype(np.float64)
            diff = hi - lo
            part = a[mix][:, None] * diff
            out[mix] = (lo + part).astype(x.dtype)
    if post.fill == "mean":
        fill = mean_model(x) if mean is None else mean
    else:
        fill = post.fill
    with np.errstate(all="ignore"):
        fill = np.asarray(fill, dtype=np.float64).astype(x.dtype)  # rounded once to the row type
    for j in range(F):
        f0, f = plan_row[2 + 2 * j: 4 + 2 * j]
        out[:, f0: f0 + f] = fill
    for j in range(N):
        t0, t = plan_row[2 + 2 * F + 2 * j: 4 + 2 * F + 2 * j]
        out[t0: t0 + t] = fill
    return out


def masked_model(post: SpecAugment, shape, plan_row) -> np.ndarray:
    """bool ``(T, C)``: the elements step 6 fills"""
    T, C = shape
    F, N = post.freq_masks, post.time_masks
    plan_row = [int(v) for v in plan_row]
    m = np.zeros((T, C), dtype=bool)
    for j in range(F):
        m[:, plan_row[2 + 2 * j]: plan_row[2 + 2 * j] + plan_row[3 + 2 * j]] = True
    for j in range(N):
        m[plan_row[2 + 2 * F + 2 * j]: plan_row[2 + 2 * F + 2 * j] + plan_row[3 + 2 * F + 2 * j]] = True
    return m


def augment_model(post: SpecAugment, utts, keys):
    """every utterance of `utts` (a list of ``(T, C)`` arrays of one width) under its key: ``(outputs, plan)``"""
    C = utts[0].shape[1]
    plan = plan_model(post, [len(u) for u in utts], C, keys)
    return [apply_model(post, u, plan[b]) for b, u in enumerate(utts)], plan


def special_values(rng, shape, dtype) -> np.ndarray:
    """the tests' hard input: normals with NaNs of distinct payloads (quiet and signalling), both zeros, both
    infinities and denormals mixed in"""
    x = rng.standard_normal(shape).astype(dtype)
    ints = np.uint32 if dtype == np.float32 else np.uint64
    bits = x.reshape(-1).view(ints)
    n = bits.size
    if dtype == np.float32:
        exp, quiet, sign = 0x7F800000, 0x00400000, 0x80000000
    else:
        exp, quiet, sign = 0x7FF0000000000000, 0x0008000000000000, 0x8000000000000000
    pick = rng.random(n)
    nan = pick < 0.08
    payload = (np.arange(n, dtype=np.uint64) + 1).astype(ints)  # distinct, never zero, below the quiet bit
    bits[nan] = ints(exp) | payload[nan] | np.where(np.arange(n) % 2 == 0, ints(quiet), ints(0))[nan] | np.where(
        np.arange(n) % 3 == 0, ints(sign), ints(0))[nan]
    bits[(pick >= 0.08) & (pick < 0.12)] = ints(0)  # +0
    bits[(pick >= 0.12) & (pick < 0.16)] = ints(sign)  # -0
    bits[(pick >= 0.16) & (pick < 0.19)] = ints(exp)  # +inf
    bits[(pick >= 0.19) & (pick < 0.22)] = ints(exp | sign)  # -inf
    den = (pick >= 0.22) & (pick < 0.28)
    bits[den] = (payload[den] & ints(0xFFFF)) | np.where(np.arange(n) % 2 == 0, ints(sign), ints(0))[den]  # denormals
    return x


def same_bytes(a, b) -> bool:
    """equal shape, dtype and bytes: NaN payloads and the signs of zeros included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
