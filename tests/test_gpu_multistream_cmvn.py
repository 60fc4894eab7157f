"""Running / global CMVN of batched streaming on the GPU (StreamBatch(cmvn=...), SiStreamBatch(cmvn=...)):
pds_multistream_cmvn against the reference's frame-by-frame Standardize (tests/golden/stream_cmvn.npz) and its
vectorised restatement, every stream's rows through the batch objects against the restatement of a cmvn-less object's
rows, the statistics tables, the order with deltas, independence of the streams and of the call form, and NaN.

Every comparison is exact: the sums are ordered float64 additions and the rest a fixed sequence of correctly rounded
float64 operations, rounded once to the feature type."""
import functools
import os

import numpy as np
import pytest

from oracle.stft_oracle import cmvn_local
from pydrobert_speech_amd import _native
from pydrobert_speech_amd.multistream import StreamBatch
from pydrobert_speech_amd.multistream_si import SiStreamBatch
from pydrobert_speech_amd.post import Deltas, Standardize
from tests.conftest import GOLDEN
from tests.test_gpu_multistream import build, random_schedule, run_concurrently
from tests.test_gpu_multistream_deltas import B, drive, expected_counts, plan_of
from tests.test_multistream_cmvn_host import CASES, NAMES as FIXTURE_NAMES, fixture, running_cmvn
from tests.test_multistream_host import golden_configs

pytestmark = pytest.mark.gpu
NAMES = ["c1_kaldi_fbank", "c2_tri_mel40"]
DTYPES = [np.float32, np.float64]
FLAG_FRESH = 1


# ---- 1. the kernel -------------------------------------------------------------------------------------------------


def kernel_schedule(T, seed, streams=5):
    """The calls of a direct drive of pds_multistream_cmvn: `streams` streams each walk T rows twice (a second life on
    the same slot: fresh over stale sums), starting at different calls; every call brings every live stream k rows, k
    drawn from 0 .. 40 with 0, 1 and 2 frequent, in random order.  Returns the list of calls, each a list of
    ``(stream, life, rows already walked, k)``"""
    rng = np.random.default_rng(seed)
    start = rng.integers(0, 4, size=streams)
    start[0] = 0
    at = np.zeros(streams, dtype=np.int64)
    life = np.zeros(streams, dtype=np.int64)
    calls = []
    while (life < 2).any():
        live = [i for i in range(streams) if life[i] < 2 and len(calls) >= start[i]]
        rng.shuffle(live)
        call = []
        for i in live:
            k = min(int(rng.choice([0, 1, 2, int(rng.integers(0, 41))])), T - int(at[i]))
            call.append((i, int(life[i]), int(at[i]), k))
            at[i] += k
            if at[i] == T:
                at[i], life[i] = 0, life[i] + 1
        calls.append(call)
    saw = {(a == 0, k > 0) for call in calls for _, _, a, k in call}
    assert {(True, True), (False, True), (False, False)} <= saw  # fresh and continuing streams, and k = 0
    assert any(len({a == 0 for _, _, a, _ in call}) == 2 for call in calls)  # ... in the same call
    return calls


def kernel_streams(X, dtype, prior, norm_var, running, seed, streams=5, capacity=8):
    """pds_multistream_cmvn driven directly over :func:`kernel_schedule`, the streams on permuted slots of a pool of
    `capacity` filled with stale values.  Returns per stream and life the rows it was given back and its sums in the
    pool after the life's last call"""
    import torch

    lib = _native.lib()
    fn = lib.pds_multistream_cmvn_f32 if dtype == np.float32 else lib.pds_multistream_cmvn_f64
    rng = np.random.default_rng(seed + 1)
    T, F = X.shape
    Xd = np.ascontiguousarray(X, dtype=dtype)
    slots = rng.permutation(capacity)[:streams]
    assert (slots != np.arange(streams)).any()  # (entry index != stream id)
    count0 = int(prior[0, -1]) if prior is not None else 0
    d_prior = torch.from_numpy(np.ascontiguousarray(prior[:, :F])).cuda() if prior is not None else None
    pool = torch.from_numpy(rng.standard_normal((capacity, 2, F))).cuda() if running else None
    got = [[[], []] for _ in range(streams)]
    sums = [[None, None] for _ in range(streams)]
    for call in kernel_schedule(T, seed, streams):
        ks = [k for _, _, _, k in call]
        rows = np.concatenate([[0], np.cumsum(ks)]).astype(np.int64)
        meta = np.zeros((len(call), 8), dtype=np.int64)
        for e, (i, _, a, k) in enumerate(call):
            meta[e, :5] = slots[i], FLAG_FRESH * (a == 0), rows[e], k, count0 + (a if running else 0)
        statics = torch.from_numpy(np.concatenate([Xd[a : a + k] for _, _, a, k in call])).cuda()
        d_meta = torch.from_numpy(meta).cuda()
        rc = fn(statics.data_ptr() if rows[-1] else None, pool.data_ptr() if running else None, capacity, F,
                d_prior.data_ptr() if d_prior is not None else None, int(norm_var), int(running),
                d_meta.data_ptr(), len(call), torch.cuda.current_stream().cuda_stream)
        _native.check(rc, "pds_multistream_cmvn")
        out = statics.cpu().numpy()
        for e, (i, life, a, k) in enumerate(call):
            got[i][life].append(out[rows[e] : rows[e + 1]])
            if running and a + k == T:
                sums[i][life] = pool[slots[i]].cpu().numpy()
    return [[np.concatenate(g) for g in stream] for stream in got], sums


def check_kernel(X, dtype, prior, norm_var, running, seed, want=None, want_stats=None):
    Y, stats = running_cmvn(np.asarray(X, dtype=dtype), prior, norm_var, running)
    if want is not None:
        assert np.array_equal(Y, want) and np.array_equal(stats, want_stats)  # (the reference's own)
    got, sums = kernel_streams(X, dtype, prior, norm_var, running, seed)
    F = X.shape[1]
    for stream, stream_sums in zip(got, sums):
        for rows, table in zip(stream, stream_sums):
            assert rows.dtype == dtype and rows.shape == Y.shape
            assert np.array_equal(rows, Y.astype(dtype)), float(np.abs(rows - Y).max())
            if running:
                assert np.array_equal(table, stats[:, :F])


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("tag", ["32", "64"])
@pytest.mark.parametrize("name", FIXTURE_NAMES)
def test_kernel_gives_the_references_rows_and_sums(name, tag, case):
    g = fixture()
    running, with_prior, norm_var = CASES[case]
    X = g[f"{name}/X{tag}"]
    prior = g[f"{name}/prior{tag}"] if with_prior else None
    check_kernel(X, X.dtype.type, prior, norm_var, running, seed=len(case) + int(tag),
                 want=g[f"{name}/{tag}/{case}/Y"], want_stats=g[f"{name}/{tag}/{case}/stats"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F", [1, 63, 64, 65, 81])
def test_kernel_on_synthetic_widths(F, dtype):
    rng = np.random.default_rng(F)
    X = (10 * rng.standard_normal((60, F)) + 5).astype(dtype)
    X[7] = X[6]  # a repeated frame
    X[:, F // 2] = -2.25  # a constant coefficient
    prior = running_cmvn(rng.standard_normal((9, F)))[1]
    for case, (running, with_prior, norm_var) in sorted(CASES.items()):
        check_kernel(X, dtype, prior if with_prior else None, norm_var, running, seed=F + len(case))


def test_kernel_refuses_bad_arguments():
    import torch

    lib = _native.lib()
    meta = torch.zeros((1, 8), dtype=torch.int64, device="cuda")
    x = torch.zeros((1, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for args in [(x.data_ptr(), None, 4, 4, None, 1, 1, meta.data_ptr(), 1),  # running without a pool
                 (x.data_ptr(), None, 4, 0, None, 1, 0, meta.data_ptr(), 1),  # no coefficients
                 (x.data_ptr(), None, 4, 4, None, 1, 0, None, 1),  # no metadata
                 (x.data_ptr(), None, 4, 4, None, 1, 0, meta.data_ptr(), -1)]:
        with pytest.raises(ValueError):
            _native.check(lib.pds_multistream_cmvn_f32(*args, stream), "pds_multistream_cmvn")
    _native.check(lib.pds_multistream_cmvn_f32(None, None, 4, 4, None, 1, 0, None, 0, stream), "n == 0")


# ---- 2. through StreamBatch ----------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def plain_of(name, dtype):
    """(computer, rounds, outputs of the plain object, a prior table): computed once per case and left unchanged"""
    comp = build(golden_configs()[name])
    rounds = plan_of(comp, dtype, 4, seed=23)
    with StreamBatch(comp, capacity=B, dtype=dtype) as sb:
        plain = drive(sb, rounds, seed=50)
    longest = max((np.concatenate(ref) for ref in plain[0]), key=len)  # (another stream's rows: the 40-frame one)
    acc = Standardize()
    acc.accumulate(longest)
    prior = acc._stats.copy()
    assert prior.shape == (2, comp.num_coeffs + 1) and prior[0, -1] == len(longest) >= 40
    prior.flags.writeable = False
    for rnd in plain:
        for ref in rnd:
            for o in ref:
                o.flags.writeable = False
    return comp, rounds, plain, prior


def standardize(prior, norm_var):
    cmvn = Standardize(norm_var=norm_var)
    if prior is not None:
        cmvn._stats = np.array(prior)
    return cmvn


MODES = {"running": (True, False), "running_prior": (True, True), "global": (False, True)}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("norm_var", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_rows_are_the_restatement_of_the_plain_rows(name, dtype, norm_var, mode):
    comp, rounds, plain, prior = plain_of(name, dtype)
    running, with_prior = MODES[mode]
    prior = prior if with_prior else None
    with StreamBatch(comp, capacity=B, dtype=dtype, cmvn=standardize(prior, norm_var), cmvn_running=running) as sb:
        assert sb.num_coeffs == comp.num_coeffs and sb.lookahead == 0
        got_rounds = drive(sb, rounds, seed=50)
        start = np.zeros((2, comp.num_coeffs + 1)) if prior is None else prior
        # (every stream is finalized: the prior, or zeros)
        assert np.array_equal(sb.cmvn_stats(np.arange(B)), np.broadcast_to(start, (B,) + start.shape))
    frames = 0
    for rnd, (got_round, plain_round) in enumerate(zip(got_rounds, plain)):
        for i, (got, ref) in enumerate(zip(got_round, plain_round)):
            what = (name, dtype.__name__, norm_var, mode, rnd, i)
            assert all(o.dtype == dtype for o in got), what
            assert [len(o) for o in got] == [len(o) for o in ref], what
            X, out = np.concatenate(ref), np.concatenate(got)
            Y, _ = running_cmvn(X, prior, norm_var, running)
            assert np.array_equal(out, Y.astype(dtype)), (what, len(X), float(np.abs(out - Y).max()))
            if not running and len(X):
                assert np.array_equal(out, cmvn_local(X, norm_var=norm_var, stats=prior).astype(dtype)), what
            frames += len(X)
    assert frames > 100


# ---- 3. cmvn_stats -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_cmvn_stats_follow_the_streams(dtype, with_prior):
    comp, _, _, prior = plain_of("c1_kaldi_fbank", dtype)
    prior = prior if with_prior else None
    start = np.zeros((2, comp.num_coeffs + 1)) if prior is None else prior
    L = comp.frame_length
    rng = np.random.default_rng(8)
    seen = [np.zeros((0, comp.num_coeffs), dtype) for _ in range(B)]
    live = 0
    with StreamBatch(comp, capacity=B, dtype=dtype, cmvn=standardize(prior, True)) as sb, \
            StreamBatch(comp, capacity=B, dtype=dtype) as plain:
        assert np.array_equal(sb.cmvn_stats([3, 0]), np.stack([start, start]))
        for ids, lens, fin in random_schedule(L, B, 10, rng):
            chunks = [(3000 * rng.standard_normal(n)).astype(dtype) for n in lens]
            sb.compute_chunks(ids, chunks)
            for i, x in zip(ids, plain.compute_chunks(ids, chunks)):
                seen[i] = np.concatenate([seen[i], x])
            tables = sb.cmvn_stats(np.arange(B))  # mid-stream, before any finalize
            assert tables.dtype == np.float64 and tables.shape == (B, 2, comp.num_coeffs + 1)
            for i in range(B):
                assert np.array_equal(tables[i], running_cmvn(seen[i], prior)[1]), i
                live += len(seen[i]) > 0
            sb.finalize(fin)
            plain.finalize(fin)
            for i in fin:
                seen[i] = seen[i][:0]
            assert np.array_equal(sb.cmvn_stats(fin), np.broadcast_to(start, (len(fin),) + start.shape))
    assert live > 20
    with StreamBatch(comp, capacity=2) as sb:
        with pytest.raises(ValueError):
            sb.cmvn_stats([0])


def test_global_statistics_never_move():
    comp, rounds, _, prior = plain_of("c2_tri_mel40", np.float32)
    with StreamBatch(comp, capacity=B, cmvn=standardize(prior, True), cmvn_running=False) as sb:
        x = (3000 * np.random.default_rng(1).standard_normal(5 * comp.frame_length)).astype(np.float32)
        assert len(sb.compute_chunks([2], [x])[0]) > 0
        assert np.array_equal(sb.cmvn_stats([2, 3]), np.stack([prior, prior]))


# ---- 4. with deltas ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,dtype,mode", [("c1_kaldi_fbank", np.float32, "running"),
                                             ("c2_tri_mel40", np.float64, "running_prior"),
                                             ("c2_tri_mel40", np.float32, "global")])
def test_deltas_are_taken_of_the_normalised_statics(name, dtype, mode):
    comp, rounds, plain, prior = plain_of(name, dtype)
    running, with_prior = MODES[mode]
    prior = prior if with_prior else None
    F, H = comp.num_coeffs, 4
    deltas = Deltas(2)
    with StreamBatch(comp, capacity=B, dtype=dtype, deltas=Deltas(2), cmvn=standardize(prior, True),
                     cmvn_running=running) as sb:
        assert sb.num_coeffs == 3 * F and sb.lookahead == H
        got_rounds = drive(sb, rounds, seed=50)
    for rnd, (got_round, plain_round) in enumerate(zip(got_rounds, plain)):
        for i, (got, ref) in enumerate(zip(got_round, plain_round)):
            what = (name, mode, rnd, i)
            assert [len(o) for o in got] == expected_counts([len(o) for o in ref], H), what
            X, out = np.concatenate(ref), np.concatenate(got)
            Y = running_cmvn(X, prior, True, running)[0].astype(dtype)
            assert out.dtype == dtype and out.shape == (len(X), 3 * F), what
            if len(X):
                assert np.array_equal(out, deltas.apply(Y, axis=0)), what


# ---- 5. independence -----------------------------------------------------------------------------------------------


def test_a_stream_alone_gives_the_same_bits():
    comp, rounds, _, prior = plain_of("c1_kaldi_fbank", np.float32)
    kwargs = dict(capacity=B, cmvn=standardize(prior, True))
    with StreamBatch(comp, **kwargs) as sb:
        company = drive(sb, rounds, seed=50)
    for rnd, i in [(0, 0), (0, 9), (1, 4), (1, 12)]:
        with StreamBatch(comp, **kwargs) as sb:
            alone = drive(sb, rounds, seed=90, only=(rnd, i))[0][0]
        assert len(alone) == len(company[rnd][i])
        for a, b in zip(alone, company[rnd][i]):
            assert a.shape == b.shape and np.array_equal(a, b), (rnd, i)


@pytest.mark.parametrize("dtype,running", [(np.float32, True), (np.float64, True), (np.float32, False)])
def test_packed_equals_host_array(dtype, running):
    import torch

    comp, _, _, prior = plain_of("c2_tri_mel40", dtype)
    L, C = comp.frame_length, 3 * comp.num_coeffs
    rng = np.random.default_rng(32)
    kwargs = dict(capacity=B, dtype=dtype, deltas=Deltas(2), cmvn_running=running)
    # (running: without a prior; global: with it)
    host = StreamBatch(comp, cmvn=standardize(None if running else prior, True), **kwargs)
    dev = StreamBatch(comp, cmvn={"name": "cmvn"} if running else standardize(prior, True), **kwargs)
    rows_total = 0
    for ids, lens, fin in random_schedule(L, B, 12, rng):
        chunks = [(3000 * rng.standard_normal(n)).astype(dtype) for n in lens]
        want = host.compute_chunks(ids, chunks)
        d_samples = torch.from_numpy(np.concatenate(chunks) if len(chunks) else np.zeros(0, dtype)).cuda()
        feats, rows = dev.compute_chunks_packed(ids, d_samples, lens)
        assert feats.is_cuda and feats.shape == (rows[-1], C)
        got = feats.cpu().numpy()
        for b, w in enumerate(want):
            assert got[rows[b] : rows[b + 1]].shape == w.shape and np.array_equal(got[rows[b] : rows[b + 1]], w)
        assert np.array_equal(host.cmvn_stats(np.arange(B)), dev.cmvn_stats(np.arange(B)))
        want = host.finalize(fin)
        feats, rows = dev.finalize_packed(fin)
        got = feats.cpu().numpy()
        for b, w in enumerate(want):
            assert got[rows[b] : rows[b + 1]].shape == w.shape and np.array_equal(got[rows[b] : rows[b + 1]], w)
            rows_total += len(w)
    assert rows_total > 0
    host.close()
    dev.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_int16_chunks_with_preemphasis(dtype):
    comp, _, _, _ = plain_of("c1_kaldi_fbank", dtype)
    rng = np.random.default_rng(33)
    kwargs = dict(capacity=B, dtype=dtype, preemphasis=0.97, cmvn="cmvn")
    rows_total = 0
    with StreamBatch(comp, **kwargs) as pcm, StreamBatch(comp, **kwargs) as converted:
        for ids, lens, fin in random_schedule(comp.frame_length, B, 10, rng):
            chunks = [np.rint(3000 * rng.standard_normal(n)).astype(np.int16) for n in lens]
            got = pcm.compute_chunks(ids, chunks)
            want = converted.compute_chunks(ids, [c.astype(dtype) for c in chunks])
            got += pcm.finalize(fin)
            want += converted.finalize(fin)
            for g, w in zip(got, want):
                assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w)
                rows_total += len(g)
    assert rows_total > 0


def test_close_releases_the_sums():
    import torch

    comp = plain_of("c1_kaldi_fbank", np.float32)[0]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    sb = StreamBatch(comp, capacity=4096, cmvn="cmvn")
    plain = 2 * 4096 * comp.frame_length * 4
    sums = 2 * 4096 * comp.num_coeffs * 8
    assert torch.cuda.memory_allocated() - before >= plain + sums
    sb.close()
    assert torch.cuda.memory_allocated() - before < sums
    with pytest.raises(ValueError):
        sb.cmvn_stats([0])


# ---- 6. SiStreamBatch ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", ["f4", "f8"])
def test_short_integration_streams(dtype):
    from tests.test_gpu_multistream_si import CAPACITY, IDS, build as si_build, drive as si_drive, fixture_streams

    name = "s1_gabor_mel"
    with np.load(os.path.join(GOLDEN, "si.npz")) as z:
        master = z["master"]
    with np.load(os.path.join(GOLDEN, "si_stream_random.npz")) as z:
        chunkings = {k: z[k] for k in z.files}
    signals, cuts = fixture_streams(chunkings, master, name, dtype)
    comp = si_build(name)
    with SiStreamBatch(comp, capacity=CAPACITY, dtype=dtype) as sb:
        plain = si_drive(sb, signals, cuts, IDS)
    with SiStreamBatch(comp, capacity=CAPACITY, dtype=dtype, cmvn=Standardize()) as sb:
        got = si_drive(sb, signals, cuts, IDS, order=[4, 1, 5, 0, 3, 2])
        again = si_drive(sb, signals, cuts, IDS, packed=True)  # (the ids reused)
        assert not sb.cmvn_stats(np.arange(CAPACITY)).any()
    frames = 0
    for case, ref in enumerate(plain):
        X = np.concatenate(ref)
        Y = running_cmvn(X)[0].astype(X.dtype)
        for outs in (got[case], again[case]):
            assert [len(o) for o in outs] == [len(o) for o in ref], case
            out = np.concatenate(outs)
            assert out.dtype == np.dtype(dtype) and np.array_equal(out, Y), case
        frames += len(X)
    assert frames > 30


# ---- 7. NaN --------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_stays_in_its_stream(dtype):
    comp = plain_of("c1_kaldi_fbank", dtype)[0]
    L = comp.frame_length
    rng = np.random.default_rng(34)
    signals = [(3000 * rng.standard_normal(12 * L)).astype(dtype) for _ in range(3)]
    signals[1][5 * L] = np.nan
    pieces = [np.split(x, np.sort(rng.integers(0, len(x), size=6))) for x in signals]
    sids = [4, 1, 9]
    with StreamBatch(comp, capacity=B, dtype=dtype) as sb:
        plain = run_concurrently(sb, sids, pieces, np.random.default_rng(35))
    with StreamBatch(comp, capacity=B, dtype=dtype, cmvn="cmvn") as sb:
        got = run_concurrently(sb, sids, pieces, np.random.default_rng(35))
    with StreamBatch(comp, capacity=B, dtype=dtype, cmvn="cmvn") as sb:  # the neighbours without the poisoned stream
        clean = run_concurrently(sb, sids[::2], pieces[::2], np.random.default_rng(36))
    for i in range(3):
        X, out = np.concatenate(plain[i]), np.concatenate(got[i])
        Y = running_cmvn(X)[0].astype(dtype)
        assert np.isnan(X).any() == (i == 1)
        assert np.array_equal(out, Y, equal_nan=True), i
        if i == 1:  # from its first NaN on a coefficient stays NaN until the finalize
            assert np.array_equal(np.isnan(out), np.cumsum(np.isnan(X), axis=0) > 0) and np.isfinite(out[0]).all()
        else:
            assert np.isfinite(out).all() and np.array_equal(out, np.concatenate(clean[i // 2]))
