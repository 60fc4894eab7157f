"""``sliding_rows_kernel`` and ``multistream_sliding_kernel`` (csrc/sliding.hip) at the launch shapes the first tests
do not reach, against ``tests/sliding_model.py`` bit for bit.

Both are driven through their C entry points with buffers of the test's own.  Offline: Kaldi's default window
(600, 100), rows wider than a block (``C = 257``) and one column wide, and 70,000 utterances of 0..3 rows with and
without one longer utterance among them.  Streaming: more lanes than a block and waves that hold two streams,
``cmn_window`` 1, 4 and 300, calls that bring a stream more rows than its ring holds with a refresh frame among
them, a restart on a slot that still holds the last life's ring and sums.  What a kernel must not read is NaN (pad
columns, gap rows, the pools before a stream's first row); what it must not write is random or NaN and compared
afterwards, byte for byte."""
import functools

import numpy as np
import pytest

from pydrobert_speech_amd import _native
from pydrobert_speech_amd.post import SlidingCMVN
from tests.sliding_model import same_bits, sliding_cmvn

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
BLOCK = 256  # lanes of a workgroup (csrc/sliding.hip)


def first_difference(got, want):
    """where two arrays of one shape and dtype differ in their bytes, for a message"""
    bad = np.argwhere(got.view(np.uint8).reshape(got.shape[0], -1) != want.view(np.uint8).reshape(want.shape[0], -1))
    if not len(bad):
        return None
    r, c = int(bad[0][0]), int(bad[0][1]) // got.itemsize
    return r, c, got.reshape(got.shape[0], -1)[r, c], want.reshape(want.shape[0], -1)[r, c], len(bad)


def assert_same_bytes(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        raise AssertionError((what,) + first_difference(got, want))


# ---- offline ---------------------------------------------------------------------------------------------------------

IN_LEAD, IN_PAD, OUT_LEAD, OUT_PAD = 1, 2, 2, 3  # columns beside the C of a row: in front, and in all


def layout(lens):
    """row offsets of utterances of `lens` rows with one gap row in front of each, and the buffer's rows"""
    lens = np.asarray(lens, dtype=np.int64)
    offs = 1 + np.cumsum(lens + 1) - (lens + 1)
    return offs, int(offs[-1] + lens[-1] + 2)


def launch_rows(buf, offs, lens, C, post, before):
    """``pds_sliding_cmvn_rows_*`` over the poisoned input `buf` into a copy of `before`; returns that copy"""
    import torch

    lib = _native.stages_lib()
    fn = lib.pds_sliding_cmvn_rows_f32 if buf.dtype == np.float32 else lib.pds_sliding_cmvn_rows_f64
    d_in, d_out = torch.from_numpy(buf).cuda(), torch.from_numpy(before).cuda()
    d_meta = torch.from_numpy(np.stack([offs, lens]).astype(np.int64)).cuda()
    assert buf.shape[1] == C + IN_PAD and before.shape[1] == C + OUT_PAD and len(buf) == len(before)
    assert (offs >= 1).all() and int((offs + lens).max()) < len(buf)
    rc = fn(d_in.data_ptr() + IN_LEAD * buf.itemsize, C + IN_PAD, d_meta[0].data_ptr(), d_meta[1].data_ptr(), len(lens),
            int(lens.max()), C, post.cmn_window, post.min_window, int(post.center), int(post.norm_vars), post.refresh,
            d_out.data_ptr() + OUT_LEAD * buf.itemsize, C + OUT_PAD, torch.cuda.current_stream().cuda_stream)
    _native.check_stages(rc, "pds_sliding_cmvn_rows")
    got = d_out.cpu().numpy()
    assert d_in.cpu().numpy().tobytes() == buf.tobytes()  # (the input is left alone)
    return got


def check_rows(xs, want, post, rng, what):
    """the utterances `xs` (``(T, C)`` each) in one launch: gap rows and pad columns of the input are NaN, the output
    buffer is random beforehand and afterwards holds `want` in the utterances' rows and nothing else new"""
    C, dtype = xs[0].shape[1], xs[0].dtype
    lens = np.asarray([len(x) for x in xs], dtype=np.int64)
    offs, total = layout(lens)
    buf = np.full((total, C + IN_PAD), np.nan, dtype=dtype)
    before = rng.standard_normal((total, C + OUT_PAD)).astype(dtype)
    expect = before.copy()
    for x, y, o in zip(xs, want, offs):
        assert y.dtype == dtype and y.shape == x.shape and np.isfinite(y).all()
        buf[o : o + len(x), IN_LEAD : IN_LEAD + C] = x
        expect[o : o + len(x), OUT_LEAD : OUT_LEAD + C] = y
    assert_same_bytes(launch_rows(buf, offs, lens, C, post, before), expect, what)


KALDI_LENGTHS = [1, 99, 100, 101, 599, 600, 601, 1300]


@functools.lru_cache(maxsize=None)
def kaldi_batch(dtype):
    rng = np.random.default_rng(600)
    xs = tuple((20.0 + 5.0 * rng.standard_normal((T, 3))).astype(dtype) for T in KALDI_LENGTHS)
    for x in xs:
        x.setflags(write=False)
    return xs


@pytest.mark.parametrize("norm_vars", [False, True], ids=["mean", "meanvar"])
@pytest.mark.parametrize("center", [False, True], ids=["causal", "centred"])
def test_kaldis_default_window(center, norm_vars):
    """``SlidingCMVN()``: cmn_window 600, min_window 100, refresh 600 -- and 250 -- over lengths around both"""
    rng = np.random.default_rng(1)
    for refresh in (None, 250):
        post = SlidingCMVN(center=center, norm_vars=norm_vars, refresh=refresh)
        assert (post.cmn_window, post.min_window, post.refresh) == (600, 100, refresh or 600)
        for dtype in DTYPES:
            xs = kaldi_batch(dtype)
            want = [sliding_cmvn(x, 600, 100, center, norm_vars, post.refresh)[0] for x in xs]
            check_rows(xs, want, post, rng, (refresh, np.dtype(dtype).name))


@pytest.mark.parametrize("norm_vars", [False, True], ids=["mean", "meanvar"])
@pytest.mark.parametrize("center", [False, True], ids=["causal", "centred"])
@pytest.mark.parametrize("C", [257, 1])
def test_rows_wider_than_a_block_and_one_column_wide(C, center, norm_vars):
    """C = 257: the lanes of one (utterance, segment) lie in two blocks; C = 1: a block holds 256 segments"""
    rng = np.random.default_rng(2 + C)
    lens = [7, 0, 1, 12, 2, 5, 6]
    for W, min_window in ((4, 1), (5, 3)):
        post = SlidingCMVN(W, min_window, center, norm_vars, 3)
        assert C > BLOCK or len(lens) * 4 * C < BLOCK
        for dtype in DTYPES:
            xs = [(20.0 + 5.0 * rng.standard_normal((T, C))).astype(dtype) for T in lens]
            want = [sliding_cmvn(x, W, min_window, center, norm_vars, 3)[0] for x in xs]
            check_rows(xs, want, post, rng, (W, np.dtype(dtype).name))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("long_one", [False, True], ids=["short", "one_of_41"])
def test_seventy_thousand_utterances(long_one, dtype):
    """lengths 0, 1, 2, 3, 0, .. and one column: 70,000 x 2 lanes, most of which own a frame; with one utterance of 41
    rows in the middle every utterance gets 21 segments, and all but a few lanes find ``t0 >= Tn``.  Utterances of one
    length are the columns of one call of the model (coefficients are independent); every utterance differs in its
    first row."""
    B, W, min_window, refresh = 70000, 4, 1, 2
    rng = np.random.default_rng(70 + long_one)
    lens = np.arange(B, dtype=np.int64) % 4
    if long_one:
        lens[B // 2] = 41
    offs, total = layout(lens)
    assert -(-int(lens.max()) // refresh) == (21 if long_one else 2)
    buf = np.full((total, 1 + IN_PAD), np.nan, dtype=dtype)
    inputs, marks = {}, rng.permutation(B)
    for T in np.unique(lens[lens > 0]).tolist():
        idx = np.flatnonzero(lens == T)
        X = (20.0 + 5.0 * rng.standard_normal((T, len(idx)))).astype(dtype)
        X[0] = (10.0 + 0.001 * marks[idx]).astype(dtype)
        rows = offs[idx][None, :] + np.arange(T)[:, None]
        buf[rows, IN_LEAD] = X
        inputs[T] = (rows, X)
    firsts = np.concatenate([X[0] for _, X in inputs.values()])
    assert len(np.unique(firsts)) == len(firsts) == int((lens > 0).sum())
    for center in (False, True):
        for norm_vars in (False, True):
            post = SlidingCMVN(W, min_window, center, norm_vars, refresh)
            before = rng.standard_normal((total, 1 + OUT_PAD)).astype(dtype)
            expect = before.copy()
            for T, (rows, X) in inputs.items():
                expect[rows, OUT_LEAD] = sliding_cmvn(X, W, min_window, center, norm_vars, refresh)[0]
            got = launch_rows(buf, offs, lens, 1, post, before)
            assert_same_bytes(got, expect, (center, norm_vars))


# ---- streaming -------------------------------------------------------------------------------------------------------

CAPACITY = 40
MW_FIELDS, FLAG_FRESH = 8, 1  # int64 per entry: stream, flags, first row, rows, frames seen before (csrc/sliding.hip)


def draws(W):
    return [0, 1, W, W + 1, W + 2, 2 * (W + 1) + 1]


def schedules(n, W, rng):
    """per stream its lives, a life being the rows each tick brings it (None: the tick does not name the stream).
    Stream 0 runs two lives; stream 1 gets more rows than the ring holds in its second call; every first life passes
    frame ``W + 1``, the first that overwrites a slot of the ring"""
    if W > 4:  # (long windows: four streams and few ticks, for the model's sake)
        a, b, c, d = W, W + 1, W + 2, 2 * (W + 1) + 1
        assert n == 4
        return [[[c, None, None], [None, 1, b]], [[1, d, 0]], [[a, c, 1]], [[0, b, b]]][:n], 3
    ticks = 7
    out = []
    for i in range(n):
        life = [int(rng.choice(draws(W))) if rng.random() < 0.8 else None for _ in range(ticks)]
        if i == 1:
            life[:2] = [1, 2 * (W + 1) + 1]
        if i == 2:
            life[0], life[3] = 0, None  # a fresh stream's first tick without rows; a tick that does not name it
        if life[1] is None:
            life[1] = int(rng.choice(draws(W)))  # (the second tick names every stream)
        if sum(k or 0 for k in life) < W + 2:
            life[-1] = 2 * (W + 1) + 1
        if i == 0:
            first = life[:3] + [None] * (ticks - 3)
            if sum(k or 0 for k in first) < W + 2:
                first[2] = 2 * (W + 1) + 1
            second = [None] * 3 + [0, W + 2, 1, W + 1]
            out.append([first, second])
        else:
            out.append([life])
    return out, ticks


def run_streams(F, n, W, refresh, norm_vars, dtype, seed):
    """`n` streams of `F` coefficients over the ticks of :func:`schedules`.  Returns how many calls brought a stream
    more than ``W + 1`` rows with a refresh frame strictly inside them."""
    import torch

    lib = _native.stages_lib()
    fn = lib.pds_multistream_sliding_f32 if dtype == np.float32 else lib.pds_multistream_sliding_f64
    rng = np.random.default_rng(seed)
    plan, ticks = schedules(n, W, rng)
    sids = [0, CAPACITY - 1] + rng.permutation(np.arange(1, CAPACITY - 1))[: n - 2].tolist()
    rng.shuffle(sids)
    assert len(set(sids)) == n and {0, CAPACITY - 1} <= set(sids)
    # every life's rows, and the model of every life in ONE call: the causal window with min_window 1 is
    # [max(0, t - W), t + 1) whatever the utterance's length, so a life's rows are the first rows of any longer
    # utterance that starts with them, and lives are laid side by side as columns of the longest (coefficients are
    # independent); checked against the model of a life alone below
    lives = [(i, j, sum(k or 0 for k in life)) for i, ls in enumerate(plan) for j, life in enumerate(ls)]
    longest = max(T for _, _, T in lives)
    X = (20.0 + 5.0 * rng.standard_normal((longest, len(lives) * F))).astype(dtype)
    Y, S1, S2 = sliding_cmvn(X, W, 1, False, norm_vars, refresh)
    col = {(i, j): slice(q * F, (q + 1) * F) for q, (i, j, _) in enumerate(lives)}
    i, j, T = min(lives, key=lambda v: (v[2] == 0, v[2]))
    assert T > 0 and same_bits(Y[:T, col[i, j]], sliding_cmvn(X[:T, col[i, j]], W, 1, False, norm_vars, refresh)[0])
    assert np.isfinite(Y).all()
    # the pools: NaN until a stream's rows are written there
    ring = np.full((CAPACITY, W + 1, F), np.nan, dtype=dtype)
    sums = np.full((CAPACITY, 2, F), np.nan, dtype=np.float64)
    d_ring, d_sums = torch.from_numpy(ring).cuda(), torch.from_numpy(sums).cuda()
    seen = {key: 0 for key in col}
    lanes = hits = 0
    for tick in range(ticks):
        entries = [(i, j, life[tick]) for i, ls in enumerate(plan) for j, life in enumerate(ls) if life[tick] is not None]
        assert len({i for i, _, _ in entries}) == len(entries)  # (a stream's lives do not overlap)
        rng.shuffle(entries)
        if not entries:
            continue
        pos, first_rows = 1, []
        for _, _, k in entries:
            first_rows.append(pos)
            pos += k + 1  # (a gap row behind every entry)
        statics = np.full((pos + 1, F), np.nan, dtype=dtype)
        expect = statics.copy()
        meta = np.zeros((len(entries), MW_FIELDS), dtype=np.int64)
        for e, ((i, j, k), row) in enumerate(zip(entries, first_rows)):
            t0 = seen[i, j]
            meta[e, :5] = [sids[i], FLAG_FRESH if t0 == 0 else 0, row, k, t0]
            statics[row : row + k] = X[t0 : t0 + k, col[i, j]]
            expect[row : row + k] = Y[t0 : t0 + k, col[i, j]]
            hits += k > W + 1 and any(t % refresh == 0 for t in range(t0 + 1, t0 + k - 1))
            for t in range(t0, t0 + k):
                ring[sids[i], t % (W + 1)] = X[t, col[i, j]]
            if k:
                sums[sids[i], 0], sums[sids[i], 1] = S1[t0 + k - 1, col[i, j]], S2[t0 + k - 1, col[i, j]]
            seen[i, j] = t0 + k
        lanes = max(lanes, len(entries) * F)
        d_statics, d_meta = torch.from_numpy(statics).cuda(), torch.from_numpy(meta).cuda()
        rc = fn(d_statics.data_ptr(), d_ring.data_ptr(), d_sums.data_ptr(), CAPACITY, F, W, int(norm_vars), refresh,
                d_meta.data_ptr(), len(entries), torch.cuda.current_stream().cuda_stream)
        _native.check_stages(rc, "pds_multistream_sliding")
        what = (F, n, W, refresh, norm_vars, np.dtype(dtype).name, tick)
        assert_same_bytes(d_statics.cpu().numpy(), expect, what + ("rows",))
        # the pools hold what the model says of the streams that got rows, and what they held of every other stream:
        # those the tick did not name, those it named without rows, those nobody ever started
        assert_same_bytes(d_ring.cpu().numpy().reshape(CAPACITY, -1), ring.reshape(CAPACITY, -1), what + ("ring",))
        assert_same_bytes(d_sums.cpu().numpy().reshape(CAPACITY, -1), sums.reshape(CAPACITY, -1), what + ("sums",))
    assert all(seen[i, j] == T for i, j, T in lives)
    assert all(seen[i, 0] >= W + 2 for i in range(n))
    assert np.isnan(ring[[s for s in range(CAPACITY) if s not in sids]]).all()
    return hits, lanes


@pytest.mark.parametrize("refresh_of", [lambda W: 1, lambda W: 3, lambda W: W + 1, lambda W: 1000],
                         ids=["every_frame", "3", "window", "never"])
@pytest.mark.parametrize("W", [1, 4, 300])
def test_streams_over_ticks(W, refresh_of):
    refresh = refresh_of(W)
    # F, streams: one coefficient; waves that hold parts of two streams, and a second block; streams on wave
    # boundaries; one more
    shapes = [(13, 4)] if W > 4 else [(1, 40), (13, 37), (64, 5), (65, 5)]
    hits = 0
    for F, n in shapes:
        for norm_vars in (False, True):
            for dtype in DTYPES:
                got, lanes = run_streams(F, n, W, refresh, norm_vars, dtype, seed=1000 * W + 10 * F + refresh % 7)
                hits += got
                assert lanes == n * F and (F not in (13, 65) or W > 4 or lanes > BLOCK)
    # a rebuild that read rows the same call had written to the ring (no stream here reaches frame 1000: with that
    # refresh the only rebuild is the empty one of frame 0)
    assert hits > 0 or refresh == 1000
