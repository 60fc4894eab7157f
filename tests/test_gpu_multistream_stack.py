"""Frame stacking of batched streaming on the GPU (StreamBatch(stack=...), SiStreamBatch(stack=...)): every stream's
rows against post.Stack over the rows of an identical batch built without `stack`, as raw bytes; the row count of every
call; independence of the streams and of the tick schedule; the packed form; pds_multistream_stack driven directly; and
the reference's Stack over its own streamed features (tests/golden/stream_stack.npz).

Every comparison of the stage itself is one of bytes: it moves values and computes nothing."""
import functools
import os

import numpy as np
import pytest

from oracle.stft_oracle import delta_filters
from pydrobert_speech_amd import _native
from pydrobert_speech_amd.multistream import StackState, StreamBatch
from pydrobert_speech_amd.multistream_si import SiStreamBatch
from pydrobert_speech_amd.post import Deltas, Stack, Standardize
from tests.conftest import GOLDEN, assert_features_close
from tests.test_gpu_multistream import build, random_schedule, run_concurrently
from tests.test_gpu_multistream_deltas import B, F32, cut, drive, samples_for
from tests.test_multistream_host import golden_configs
from tests.test_multistream_stack_host import FLAG_FINAL, FLAG_HALF, PAD_CONSTANT, PAD_EDGE, PAD_NONE, stack_totals

pytestmark = pytest.mark.gpu
NAMES = ["c1_kaldi_fbank", "c2_tri_mel40"]
DTYPES = [np.float32, np.float64]
NVS = [2, 3, 5]
FILL = -2.5
PADS = {"none": {}, "edge": dict(pad_mode="edge"), "constant": dict(pad_mode="constant", constant_values=FILL)}
PAD_CODES = {"none": PAD_NONE, "edge": PAD_EDGE, "constant": PAD_CONSTANT}
STAGES = {
    "plain": lambda: {},
    "deltas": lambda: dict(deltas=Deltas(2)),
    "cmvn_deltas": lambda: dict(cmvn=Standardize(), deltas=Deltas(1, context_window=3)),
}
WIDTH = {"plain": 1, "deltas": 3, "cmvn_deltas": 2}  # row width before stacking, in statics
LOOKAHEAD = {"plain": 0, "deltas": 4, "cmvn_deltas": 3}


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def plan_of(comp, dtype, nv, seed):
    """two rounds of (stream ids, chunks per stream): streams ending at each total of stack_totals(nv) -- the 40-frame
    one fed a single chunk --, cut into chunks of which 0 and 1 samples are frequent, and random ones; the second round
    reuses the ids of the first"""
    rng = np.random.default_rng(seed)
    L = comp.frame_length

    def signal(n):
        return (3000 * rng.standard_normal(n)).astype(dtype)

    rounds = []
    totals = stack_totals(nv)
    for rnd in range(2):
        order = rng.permutation(len(totals))
        pieces = [[signal(samples_for(comp, 40))] if totals[t] == 40 else cut(signal(samples_for(comp, totals[t])), L, rng)
                  for t in order]
        for _ in range(3):
            pieces.append([signal(c) for c in rng.integers(0, 3 * L + 1, size=int(rng.integers(2, 7)))])
        sids = rng.permutation(B - 1)[: len(pieces)]
        rounds.append((sids.tolist(), pieces))
    return rounds


@functools.lru_cache(maxsize=None)
def plain_of(name, dtype, stage, nv):
    """(computer, rounds, outputs of the batch without `stack`): computed once per case and left unchanged"""
    comp = build(golden_configs()[name])
    rounds = plan_of(comp, dtype, nv, seed=11 * nv + len(stage))
    with StreamBatch(comp, capacity=B, dtype=dtype, **STAGES[stage]()) as sb:
        assert sb.num_vectors == 1 and sb.num_coeffs == WIDTH[stage] * comp.num_coeffs
        plain = drive(sb, rounds, seed=50)
    for rnd in plain:
        for ref in rnd:
            for o in ref:
                o.flags.writeable = False
    return comp, rounds, plain


@functools.lru_cache(maxsize=None)
def stacked_of(name, dtype, stage, nv, pad):
    """the outputs of the batch with `stack` under the tick schedule of the plain one, and under another"""
    comp, rounds, _ = plain_of(name, dtype, stage, nv)
    out = []
    for seed in (50, 77):
        with StreamBatch(comp, capacity=B, dtype=dtype, stack=Stack(nv, **PADS[pad]), **STAGES[stage]()) as sb:
            assert sb.num_vectors == nv and sb.num_coeffs == nv * WIDTH[stage] * comp.num_coeffs
            assert sb.lookahead == LOOKAHEAD[stage]
            out.append(drive(sb, rounds, seed=seed))
            assert not sb.kstate.pending.any()  # (every stream was finalized)
    return out


def predicted_counts(plain_counts, nv, pad):
    """StackState's row count of every call from the rows every call brings (the last call is finalize)"""
    state, ids, want = StackState(1, nv, pad=pad != "none"), np.zeros(1, dtype=np.int64), []
    for j, m in enumerate(plain_counts):
        step = state.step(ids, [m], final=j == len(plain_counts) - 1)
        want.append(int(step["groups"][0]))
        state.commit(ids, step)
    return want


MATRIX = [(name, dtype, stage, nv, pad) for name in NAMES for dtype in DTYPES for stage in sorted(STAGES)
          for nv in NVS for pad in sorted(PADS)]


@pytest.mark.parametrize("name,dtype,stage,nv,pad", MATRIX)
def test_rows_are_stack_of_the_plain_rows(name, dtype, stage, nv, pad):
    comp, rounds, plain = plain_of(name, dtype, stage, nv)
    with_stack, rescheduled = stacked_of(name, dtype, stage, nv, pad)
    C = WIDTH[stage] * comp.num_coeffs
    stack = Stack(nv, **PADS[pad])
    seen_totals, partial = set(), 0
    for rnd, (got_round, plain_round, other_round) in enumerate(zip(with_stack, plain, rescheduled)):
        for i, (got, ref, other) in enumerate(zip(got_round, plain_round, other_round)):
            X = np.concatenate(ref)
            out = np.concatenate(got)
            what = (name, dtype.__name__, stage, nv, pad, rnd, i, len(X))
            assert all(o.dtype == dtype and o.shape[1:] == (nv * C,) for o in got), what
            assert [len(o) for o in got] == predicted_counts([len(o) for o in ref], nv, pad), what
            want = stack.apply(X, axis=-1)
            assert want.dtype == dtype and want.shape == (-(-len(X) // nv) if pad != "none" else len(X) // nv, nv * C)
            assert same_bytes(out, want), what
            # another tick schedule cuts the calls elsewhere and gives the same stream
            assert same_bytes(np.concatenate(other), want), what
            seen_totals.add(len(X))
            partial += len(X) % nv > 0
    assert seen_totals >= set(stack_totals(nv)) and partial >= 4


ALONE = MATRIX[::11]  # (every pair of nv and pad, every stage, dtype and name among them)


@pytest.mark.parametrize("name,dtype,stage,nv,pad", ALONE)
def test_streams_are_independent(name, dtype, stage, nv, pad):
    comp, rounds, _ = plain_of(name, dtype, stage, nv)
    with_stack = stacked_of(name, dtype, stage, nv, pad)[0]
    for rnd, (sids, pieces) in enumerate(rounds):
        for i in range(len(sids)):
            with StreamBatch(comp, capacity=B, dtype=dtype, stack=Stack(nv, **PADS[pad]), **STAGES[stage]()) as sb:
                alone = drive(sb, rounds, seed=90, only=(rnd, i))[0][0]
            assert len(alone) == len(with_stack[rnd][i])
            for a, b in zip(alone, with_stack[rnd][i]):
                assert same_bytes(a, b), (name, stage, nv, pad, rnd, i)


def test_the_independence_cases_cover_the_matrix():
    cases = ALONE
    assert {c[3:] for c in cases} == {(nv, pad) for nv in NVS for pad in PADS}
    assert {c[2] for c in cases} == set(STAGES) and {c[1] for c in cases} == set(DTYPES) and {c[0] for c in cases} == set(NAMES)


@pytest.mark.parametrize("name,dtype,stage,nv,pad", [("c1_kaldi_fbank", np.float32, "deltas", 3, "none"),
                                                     ("c2_tri_mel40", np.float32, "plain", 2, "constant"),
                                                     ("c1_kaldi_fbank", np.float64, "cmvn_deltas", 5, "edge"),
                                                     ("c2_tri_mel40", np.float64, "plain", 3, "edge")])
def test_packed_equals_host_array(name, dtype, stage, nv, pad):
    import torch

    comp = build(golden_configs()[name])
    L, C = comp.frame_length, nv * WIDTH[stage] * comp.num_coeffs
    rng = np.random.default_rng(31)
    host = StreamBatch(comp, capacity=B, dtype=dtype, stack=Stack(nv, **PADS[pad]), **STAGES[stage]())
    dev = StreamBatch(comp, capacity=B, dtype=dtype, stack=dict(name="stack", num_vectors=nv, **PADS[pad]),
                      **STAGES[stage]())
    rows_total = 0
    for ids, lens, fin in random_schedule(L, B, 14, rng):
        lens = np.where(rng.random(len(lens)) < 0.5, np.minimum(lens, L // 2), lens)  # (more one-frame ticks)
        chunks = [(3000 * rng.standard_normal(n)).astype(dtype) for n in lens]
        want = host.compute_chunks(ids, chunks)
        d_samples = torch.from_numpy(np.concatenate(chunks) if len(chunks) else np.zeros(0, dtype)).cuda()
        feats, rows = dev.compute_chunks_packed(ids, d_samples, lens)
        # (the offsets count stacked rows)
        assert feats.is_cuda and feats.shape == (rows[-1], C) and len(rows) == len(ids) + 1 and rows[0] == 0
        assert np.diff(rows).tolist() == [len(w) for w in want]
        got = feats.cpu().numpy()
        for b, w in enumerate(want):
            assert same_bytes(got[rows[b] : rows[b + 1]], w)
        want = host.finalize(fin)
        started = dev.started(fin)
        feats, rows = dev.finalize_packed(fin)
        assert feats.shape == (rows[-1], C) and len(rows) == len(fin) + 1
        got = feats.cpu().numpy()
        for b, w in enumerate(want):
            if started[b]:
                assert same_bytes(got[rows[b] : rows[b + 1]], w)
            else:  # (never started: no rows, and the host-array call says so in float64)
                assert rows[b] == rows[b + 1] and w.shape == (0, C) and w.dtype == np.float64
            rows_total += len(w)
        assert (host.started(np.arange(B)) == dev.started(np.arange(B))).all()
        assert (host.kstate.pending == dev.kstate.pending).all()
    assert rows_total > 0
    host.close()
    dev.close()


def test_one_vector_is_no_stack():
    comp = build(golden_configs()["c2_tri_mel40"])
    x = (3000 * np.random.default_rng(4).standard_normal(4 * comp.frame_length)).astype(np.float32)
    with StreamBatch(comp, capacity=2, stack=Stack(1, pad_mode="edge")) as a, StreamBatch(comp, capacity=2) as b:
        assert a.num_coeffs == comp.num_coeffs and a.num_vectors == 1 and a.kstate is None
        for u, v in zip(a.compute_chunks([1], [x]) + a.finalize([1]), b.compute_chunks([1], [x]) + b.finalize([1])):
            assert len(u) and same_bytes(u, v)


def test_close_releases_the_pending_rows():
    import torch

    comp = build(golden_configs()["c1_kaldi_fbank"])
    StreamBatch(comp, capacity=1).close()  # (what the computer itself keeps on the device is there before)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    sb = StreamBatch(comp, capacity=4096, stack=Stack(5))
    pending = 2 * 4096 * 4 * comp.num_coeffs * 4
    assert torch.cuda.memory_allocated() - before >= 2 * 4096 * comp.frame_length * 4 + pending
    sb.close()
    assert torch.cuda.memory_allocated() - before < pending
    with pytest.raises(ValueError):
        sb.compute_chunks([0], [np.zeros(3, np.float32)])


# ---- the kernel ----------------------------------------------------------------------------------------------------


def odd_values(rng, shape, dtype):
    """random values with NaNs of several payloads and signs, infinities and zeros of both signs among them"""
    x = rng.standard_normal(shape).astype(dtype)
    bits = x.view(np.uint32 if dtype == np.float32 else np.uint64).reshape(-1)
    if dtype == np.float32:
        odd = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0xFFFFFFFF, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000,
                        0x00000001, 0x80000001], dtype=np.uint32)
    else:
        odd = np.array([0x7FF8000000000000, 0x7FF8000012345678, 0xFFF8000000000001, 0xFFFFFFFFFFFFFFFF,
                        0x8000000000000000, 0, 0x7FF0000000000000, 0xFFF0000000000000, 1, 0x8000000000000001],
                       dtype=np.uint64)
    k = min(bits.size, max(len(odd), int(0.15 * bits.size)))  # (each of them at least once where there is room)
    bits[rng.permutation(bits.size)[:k]] = np.concatenate([odd, rng.choice(odd, size=max(0, k - len(odd)))])[:k]
    return x


def kernel_streams(X, nv, pad, fill, seed, streams=5, capacity=8):
    """pds_multistream_stack driven directly: `streams` streams each walk the rows of X twice (a second life on the
    same slot: over stale pending rows), starting at different calls, on permuted slots of a pool of `capacity` filled
    with stale values; every call brings every live stream m rows, m drawn from 0 .. 2 nv + 1 with 0 and 1 frequent, in
    random order, and a stream's last rows come with its final call.  Returns per stream and life the rows it was
    given, call by call"""
    import torch

    lib = _native.lib()
    dtype = X.dtype.type
    fn = lib.pds_multistream_stack_f32 if dtype == np.float32 else lib.pds_multistream_stack_f64
    rng = np.random.default_rng(seed)
    T, C = X.shape
    slots = rng.permutation(capacity)[:streams]
    assert (slots != np.arange(streams)).any()  # (entry index != stream id)
    pool = torch.from_numpy(odd_values(rng, (2, capacity, nv - 1, C), dtype)).cuda()
    start = rng.integers(0, 4, size=streams)
    start[0] = 0
    at = np.zeros(streams, dtype=np.int64)
    life = np.zeros(streams, dtype=np.int64)
    pending = np.zeros(streams, dtype=np.int64)
    half = rng.integers(0, 2, size=streams)  # (the halves need not start alike)
    got = [[[], []] for _ in range(streams)]
    calls = copies = 0
    stream = torch.cuda.current_stream().cuda_stream
    while (life < 2).any():
        live = [i for i in range(streams) if life[i] < 2 and calls >= start[i]]
        rng.shuffle(live)
        calls += 1
        # a stream within nv rows of its end, or at it, is finalized with what is left (now and then with nothing)
        last = {i for i in live if T - at[i] <= nv and rng.random() < 0.5}
        for final in (False, True):
            group = [i for i in live if (i in last) == final]
            if not group:
                continue
            m = [int(T - at[i]) if final else min(int(rng.choice([0, 1, 1, int(rng.integers(0, 2 * nv + 2))])),
                                                   int(T - at[i])) for i in group]
            new_rows = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
            meta = np.zeros((len(group), 8), dtype=np.int64)
            for e, i in enumerate(group):
                V = pending[i] + m[e]
                G = -(-V // nv) if final and pad != PAD_NONE else V // nv
                meta[e, :6] = slots[i], half[i] | (FLAG_FINAL if final else 0), pending[i], m[e], new_rows[e], G
                copies += (not final) and G == 0 and pending[i] > 0
            out_rows = np.concatenate([[0], np.cumsum(meta[:, 5])]).astype(np.int64)
            meta[:, 6] = out_rows[:-1]
            V = meta[:, 2] + meta[:, 3]
            elems = np.concatenate([[0], np.cumsum((meta[:, 5] * nv if final else V) * C)]).astype(np.int64)
            rows = torch.from_numpy(np.concatenate([X[at[i] : at[i] + m[e]] for e, i in enumerate(group)])).cuda()
            out = torch.from_numpy(odd_values(rng, (int(out_rows[-1]), nv * C), dtype)).cuda()  # (all of it is written)
            poison = out.cpu().numpy().copy()
            d_meta, d_elems = torch.from_numpy(meta).cuda(), torch.from_numpy(elems).cuda()
            rc = fn(rows.data_ptr() if new_rows[-1] else None, pool.data_ptr(), capacity, nv, C, d_meta.data_ptr(),
                    d_elems.data_ptr(), len(group), int(elems[-1]), pad, fill, out.data_ptr() if out_rows[-1] else None,
                    stream)
            _native.check(rc, "pds_multistream_stack")
            host = out.cpu().numpy()
            if host.size:
                assert not same_bytes(host, poison)
            for e, i in enumerate(group):
                got[i][life[i]].append(host[out_rows[e] : out_rows[e + 1]])
                at[i] += m[e]
                if final:
                    at[i], pending[i], life[i] = 0, 0, life[i] + 1
                else:
                    pending[i] = V[e] - meta[e, 5] * nv
                    half[i] ^= 1
    assert copies > 0
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pad", sorted(PADS))
@pytest.mark.parametrize("nv", NVS)
@pytest.mark.parametrize("C", [1, 41, 64])  # 41: rows that are not 16-byte aligned
def test_kernel_moves_every_bit(C, nv, pad, dtype):
    rng = np.random.default_rng(1000 * C + 10 * nv + len(pad))
    stack = Stack(nv, **PADS[pad])
    for T in (3 * nv + 1, 40):
        X = odd_values(rng, (T, C), dtype)
        assert np.isnan(X).any() and (np.signbit(X) & (X == 0)).any()
        want = stack.apply(X, axis=-1)
        for stream in kernel_streams(X, nv, PAD_CODES[pad], FILL, seed=C + nv + T):
            for calls in stream:
                rows = np.concatenate(calls)
                assert same_bytes(rows, want), (C, nv, pad, T)


def test_kernel_refuses_bad_arguments():
    import torch

    lib = _native.lib()
    meta = torch.zeros((1, 8), dtype=torch.int64, device="cuda")
    meta[0, 3] = 1  # one new row, no group: it becomes the pending row
    prefix = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    x = torch.zeros((1, 4), dtype=torch.float32, device="cuda")
    pool = torch.zeros((2, 4, 1, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ok = (x.data_ptr(), pool.data_ptr(), 4, 2, 4, meta.data_ptr(), prefix.data_ptr(), 1, 4, 0, 0.0, None)
    _native.check(lib.pds_multistream_stack_f32(*ok, stream), "a tick without a group has no output")
    assert np.array_equal(pool.cpu().numpy()[1, 0, 0], np.zeros(4, np.float32))
    for at, value in [(1, None),  # no pool
                      (3, 1), (3, 0),  # a "group" of one row has no pending rows
                      (4, 0),  # no coefficients
                      (5, None), (6, None),  # no metadata, no prefix
                      (7, -1), (8, -1),  # negative sizes
                      (9, 3), (9, -1)]:  # no such padding
        args = list(ok)
        args[at] = value
        with pytest.raises(ValueError):
            _native.check(lib.pds_multistream_stack_f32(*args, stream), "pds_multistream_stack")
    for fn in (lib.pds_multistream_stack_f32, lib.pds_multistream_stack_f64):
        _native.check(fn(None, None, 4, 2, 4, None, None, 0, 0, 0, 0.0, None, stream), "n == 0")
        _native.check(fn(None, None, 4, 2, 4, None, None, 3, 0, 0, 0.0, None, stream), "no elements")


# ---- SiStreamBatch -------------------------------------------------------------------------------------------------


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
    stack = Stack(3, pad_mode="edge")
    with SiStreamBatch(comp, capacity=CAPACITY, dtype=dtype) as sb:
        plain = si_drive(sb, signals, cuts, IDS)
    with SiStreamBatch(comp, capacity=CAPACITY, dtype=dtype, stack=stack) as sb:
        assert sb.num_vectors == 3 and sb.num_coeffs == 3 * comp.num_coeffs
        got = si_drive(sb, signals, cuts, IDS, order=[4, 1, 5, 0, 3, 2])
        again = si_drive(sb, signals, cuts, IDS, packed=True)  # (the ids reused)
        assert not sb.kstate.pending.any()
    frames = 0
    for case, ref in enumerate(plain):
        X = np.concatenate(ref)
        want = stack.apply(X, axis=-1)
        for outs in (got[case], again[case]):
            assert [len(o) for o in outs] == predicted_counts([len(o) for o in ref], 3, "edge"), case
            assert same_bytes(np.concatenate(outs), want), case
        frames += len(X)
    assert frames > 30


# ---- the reference's Stack -----------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", NAMES)
def test_reference_stack_of_the_random_chunkings(name, master_signal):
    """tests/golden/make_golden_stream_stack.py: the reference's Stack over its own streamed features, with and without
    its Deltas(2) underneath.

    The features underneath are the GPU's, held to the project's float32 tolerance |s - s_ref| <= 1e-5 + 1e-4 |s_ref|
    (assert_features_close), and the delta columns of the first case to the bound test_gpu_multistream_deltas.py derives
    from it for stream_deltas.npz (the sum of a delta is linear in the statics: sum_j |f_k[j]| * (1e-5 + 1e-4 |s_ref|) of
    the rows its taps read, plus 2**-22 |d_ref| for the two roundings to float32).  Stacking moves values, so an
    element's bound is the bound of the element it is a copy of; a constant fill is exact."""
    K, W = 2, 2
    with np.load(os.path.join(GOLDEN, "stream_random.npz")) as z:
        g = {k: z[k] for k in z.files if k.startswith(name + "/")}
    with np.load(os.path.join(GOLDEN, "stream_deltas.npz")) as z:
        gd = {k: z[k] for k in z.files if k.startswith(name + "/")}
    with np.load(os.path.join(GOLDEN, "stream_stack.npz")) as z:
        gs = {k: z[k] for k in z.files if k.startswith(name + "/")}
    comp = build(golden_configs()[name])
    F = comp.num_coeffs
    pieces = []
    for case in range(8):
        n = int(g[f"{name}/{case}/n"])
        pieces.append(np.split(master_signal[50 : 50 + n].astype("f4"), g[f"{name}/{case}/cuts"]))
    sids = [2 * i + 1 for i in range(8)]
    settings = {
        "deltas_stack3": (3, "none", dict(deltas=Deltas(K), stack=Stack(3))),
        "stack4_edge": (4, "edge", dict(stack=Stack(4, pad_mode="edge"))),
        "stack2_constant": (2, "constant", dict(stack=Stack(2, pad_mode="constant", constant_values=-1.0))),
    }
    filts = delta_filters(K, W)[1:]
    rows_total = 0
    for tag, (nv, pad, kwargs) in settings.items():
        with StreamBatch(comp, capacity=B, **kwargs) as sb:
            outs = run_concurrently(sb, sids, pieces, np.random.default_rng(11))
        for case in range(8):
            ref = gs[f"{name}/{case}/{tag}"].astype(np.float64)
            got = np.concatenate(outs[case])
            T = int(g[f"{name}/{case}/counts"].sum())
            what = (name, case, tag)
            assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.shape, ref.shape)
            assert len(ref) == (-(-T // nv) if pad != "none" else T // nv), what
            rows_total += len(ref)
            if tag != "deltas_stack3":
                assert_features_close(got, ref, what=what, **F32)
                if pad == "constant" and T % nv:
                    assert (got[-1, -F:] == -1.0).all() and (ref[-1, -F:] == -1.0).all(), what
                continue
            full = gd[f"{name}/{case}/deltas"].astype(np.float64)  # the reference's unstacked rows
            assert np.array_equal(ref, Stack(3).apply(full, axis=-1)), what
            G = len(ref)
            got, ref = got.reshape(G * 3, 3 * F), ref.reshape(G * 3, 3 * F)
            assert_features_close(got[:, :F], ref[:, :F], what=what, **F32)
            for k, filt in enumerate(filts, start=1):
                bound = 2.0 ** -22 * np.abs(full[:, k * F : (k + 1) * F])
                for j, w in enumerate(filt):
                    rows = np.clip(np.arange(T) + j - k * W, 0, max(T - 1, 0))
                    bound += abs(w) * (1e-5 + 1e-4 * np.abs(full[rows, :F]))
                err = np.abs(got[:, k * F : (k + 1) * F] - ref[:, k * F : (k + 1) * F])
                assert (err <= bound[: G * 3]).all(), (what, k, float(err.max()), float((err / bound[: G * 3]).max()))
    assert rows_total > 50
