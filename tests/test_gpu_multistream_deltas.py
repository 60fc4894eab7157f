"""Delta features of batched streaming on the GPU (multistream.StreamBatch(deltas=...)): every stream's rows against a
deltas-less StreamBatch and Deltas.apply bit for bit, the delayed row counts, independence of the streams, the packed
form, and the reference's Deltas(2) over its own streamed features."""
import functools
import os

import numpy as np
import pytest

from oracle.stft_oracle import delta_filters
from pydrobert_speech_amd import config
from pydrobert_speech_amd.multistream import StreamBatch, StreamState
from pydrobert_speech_amd.post import Deltas
from tests.conftest import GOLDEN, assert_features_close
from tests.test_gpu_multistream import build, random_schedule, run_concurrently
from tests.test_multistream_deltas_host import KW, totals_of
from tests.test_multistream_host import golden_configs

pytestmark = pytest.mark.gpu
F32 = dict(rtol=1e-4, atol=1e-5)
NAMES = ["c1_kaldi_fbank", "c2_tri_mel40"]
B = 16
NEVER = 15  # an id no stream uses


def total_frames(comp, n):
    """frames of compute_chunk + finalize of an n-sample stream (however it is cut)"""
    state = StreamState(1, comp.frame_length, comp.frame_shift, comp.pad_left)
    ids = np.zeros(1, dtype=np.int64)
    step = state.chunk_step(ids, np.asarray([n]))
    state.commit_chunks(ids, step)
    return int(step["k"][0] + state.finalize_step(ids)["k"][0])


def samples_for(comp, frames):
    """the fewest samples that give `frames` frames (the count does not fall as samples are added)"""
    lo, hi = 0, (frames + 2) * comp.frame_shift + comp.frame_length
    while lo < hi:
        mid = (lo + hi) // 2
        if total_frames(comp, mid) >= frames:
            hi = mid
        else:
            lo = mid + 1
    assert total_frames(comp, lo) == frames
    return lo


def cut(x, L, rng):
    """`x` in chunks of lengths in [0, 3 L], 0 and 1 frequent"""
    pieces, pos = [], 0
    while pos < len(x) or not pieces:
        r = rng.random()
        c = 0 if r < 0.2 else 1 if r < 0.4 else int(rng.integers(0, 3 * L + 1))
        pieces.append(x[pos : pos + c])
        pos += c
    return pieces + [x[:0]] * int(rng.integers(0, 3))


def plan_of(comp, dtype, H, seed):
    """two rounds of (stream ids, chunks per stream): streams ending at each total of totals_of(H), one fed a single
    40-frame chunk, random ones; the second round reuses the ids of the first"""
    rng = np.random.default_rng(seed)
    L = comp.frame_length

    def signal(n):
        return (3000 * rng.standard_normal(n)).astype(dtype)

    rounds = []
    totals = totals_of(H)
    for rnd in range(2):
        order = rng.permutation(len(totals))
        pieces = [cut(signal(samples_for(comp, totals[t])), L, rng) for t in order]
        pieces.append([signal(samples_for(comp, 40))])
        for _ in range(3):
            pieces.append([signal(c) for c in rng.integers(0, 3 * L + 1, size=int(rng.integers(2, 7)))])
        sids = rng.permutation(B - 1)[: len(pieces)]
        rounds.append((sids.tolist(), pieces))
    return rounds


def drive(sb, rounds, seed, only=None):
    """the rounds through `sb` with the tick schedule of `seed` (or, with `only` = (round, stream), that stream alone);
    per round and stream the list of per-call outputs"""
    outs = []
    for r, (sids, pieces) in enumerate(rounds):
        if only is not None:
            if only[0] != r:
                continue
            sids, pieces = [sids[only[1]]], [pieces[only[1]]]
        outs.append(run_concurrently(sb, sids, pieces, np.random.default_rng(seed + r)))
        idle = sb.finalize([NEVER])  # never started
        assert idle[0].shape == (0, sb.num_coeffs) and idle[0].dtype == np.float64
    return outs


@functools.lru_cache(maxsize=None)
def together(name, dtype, K, W):
    """(computer, rounds, outputs of the deltas object, outputs of the plain object) of one case of the matrix"""
    comp = build(golden_configs()[name])
    rounds = plan_of(comp, dtype, K * W, seed=7 * K + W)
    with StreamBatch(comp, capacity=B, dtype=dtype, deltas=Deltas(K, context_window=W)) as sb:
        assert sb.num_coeffs == (K + 1) * comp.num_coeffs and sb.lookahead == K * W
        with_deltas = drive(sb, rounds, seed=50)
    with StreamBatch(comp, capacity=B, dtype=dtype) as sb:
        assert sb.num_coeffs == comp.num_coeffs and sb.lookahead == 0
        plain = drive(sb, rounds, seed=50)
    return comp, rounds, with_deltas, plain


def expected_counts(static_counts, H):
    """the delayed row count of every call from the static frames of every call (the last call is finalize)"""
    want, n, e = [], 0, 0
    for j, k in enumerate(static_counts):
        n += k
        want.append(n - e if j == len(static_counts) - 1 else max(0, n - H) - e)
        e += want[-1]
    return want


MATRIX = [(name, dtype, K, W) for name in NAMES for dtype in (np.float32, np.float64) for K, W in KW]


@pytest.mark.parametrize("name,dtype,K,W", MATRIX)
def test_bitwise_self_consistency(name, dtype, K, W):
    comp, rounds, with_deltas, plain = together(name, dtype, K, W)
    F, H = comp.num_coeffs, K * W
    deltas = Deltas(K, context_window=W)
    seen_totals = set()
    for rnd, (got_round, plain_round) in enumerate(zip(with_deltas, plain)):
        for i, (got, ref) in enumerate(zip(got_round, plain_round)):
            X = np.concatenate(ref)
            out = np.concatenate(got)
            what = (name, dtype.__name__, K, W, rnd, i, len(X))
            assert all(o.dtype == dtype for o in got), what
            assert [len(o) for o in got] == expected_counts([len(o) for o in ref], H), what
            assert out.shape == (len(X), (K + 1) * F), what
            assert np.array_equal(out[:, :F], X), what
            want = deltas.apply(X, axis=0)
            assert want.dtype == dtype and want.shape == out.shape
            assert np.array_equal(out[:, F:], want[:, F:]), (what, float(np.abs(out - want).max()))
            seen_totals.add(len(X))
    assert seen_totals >= set(totals_of(H)) | {40}


@pytest.mark.parametrize("name,dtype,K,W", MATRIX)
def test_streams_are_independent(name, dtype, K, W):
    comp, rounds, with_deltas, _ = together(name, dtype, K, W)
    for rnd, (sids, pieces) in enumerate(rounds):
        for i in range(len(sids)):
            with StreamBatch(comp, capacity=B, dtype=dtype, deltas=Deltas(K, context_window=W)) as sb:
                alone = drive(sb, rounds, seed=90, only=(rnd, i))[0][0]
            assert len(alone) == len(with_deltas[rnd][i])
            for a, b in zip(alone, with_deltas[rnd][i]):
                assert a.shape == b.shape and np.array_equal(a, b), (name, K, W, rnd, i)


@pytest.mark.parametrize("name,dtype,K,W", [("c1_kaldi_fbank", np.float32, 2, 2), ("c2_tri_mel40", np.float32, 3, 2),
                                            ("c1_kaldi_fbank", np.float64, 2, 3), ("c2_tri_mel40", np.float64, 1, 1)])
def test_packed_equals_host_array(name, dtype, K, W):
    import torch

    comp = build(golden_configs()[name])
    L, C = comp.frame_length, (K + 1) * comp.num_coeffs
    rng = np.random.default_rng(31)
    host = StreamBatch(comp, capacity=B, dtype=dtype, deltas=Deltas(K, context_window=W))
    dev = StreamBatch(comp, capacity=B, dtype=dtype, deltas={"name": "deltas", "num_deltas": K, "context_window": W})
    rows_total = 0
    for ids, lens, fin in random_schedule(L, B, 14, rng):
        lens = np.where(rng.random(len(lens)) < 0.5, np.minimum(lens, L // 2), lens)  # (more one-frame ticks)
        chunks = [(3000 * rng.standard_normal(n)).astype(dtype) for n in lens]
        want = host.compute_chunks(ids, chunks)
        d_samples = torch.from_numpy(np.concatenate(chunks) if len(chunks) else np.zeros(0, dtype)).cuda()
        feats, rows = dev.compute_chunks_packed(ids, d_samples, lens)
        assert feats.is_cuda and feats.shape == (rows[-1], C) and len(rows) == len(ids) + 1
        got = feats.cpu().numpy()
        for b, w in enumerate(want):
            assert got[rows[b] : rows[b + 1]].shape == w.shape and np.array_equal(got[rows[b] : rows[b + 1]], w)
        want = host.finalize(fin)
        feats, rows = dev.finalize_packed(fin)
        assert feats.shape == (rows[-1], C)
        got = feats.cpu().numpy()
        for b, w in enumerate(want):
            assert got[rows[b] : rows[b + 1]].shape == w.shape and np.array_equal(got[rows[b] : rows[b + 1]], w)
            rows_total += len(w)
        assert (host.started(np.arange(B)) == dev.started(np.arange(B))).all()
    assert rows_total > 0
    host.close()
    dev.close()


def test_float32_arithmetic_takes_the_widened_statics(monkeypatch):
    monkeypatch.setattr(config, "FLOAT64_ARITHMETIC", "float32")
    comp = build(golden_configs()["c1_kaldi_fbank"])
    F = comp.num_coeffs
    rounds = plan_of(comp, np.float64, 4, seed=3)[:1]
    with StreamBatch(comp, capacity=B, dtype=np.float64, deltas=Deltas(2)) as sb:
        got = drive(sb, rounds, seed=60)[0]
    with StreamBatch(comp, capacity=B, dtype=np.float64) as sb:
        plain = drive(sb, rounds, seed=60)[0]
    for g, p in zip(got, plain):
        X, out = np.concatenate(p), np.concatenate(g)
        assert out.dtype == np.float64 and np.array_equal(X, X.astype(np.float32))  # (float32 values, widened)
        assert np.array_equal(out[:, :F], X)
        assert np.array_equal(out[:, F:], Deltas(2).apply(X, axis=0)[:, F:])


def test_num_deltas_zero_is_no_deltas():
    comp = build(golden_configs()["c2_tri_mel40"])
    x = (3000 * np.random.default_rng(4).standard_normal(4 * comp.frame_length)).astype(np.float32)
    with StreamBatch(comp, capacity=2, deltas=Deltas(0)) as a, StreamBatch(comp, capacity=2) as b:
        assert a.num_coeffs == comp.num_coeffs and a.lookahead == 0
        for u, v in zip(a.compute_chunks([1], [x]) + a.finalize([1]), b.compute_chunks([1], [x]) + b.finalize([1])):
            assert len(u) and np.array_equal(u, v)


@pytest.mark.parametrize("name", NAMES)
def test_reference_deltas_of_the_random_chunkings(name, master_signal):
    """tests/golden/make_golden_stream_deltas.py: the reference's Deltas(2) along axis 0 of its streamed features.

    Statics are held to the project's float32 tolerance, |s - s_ref| <= 1e-5 + 1e-4 |s_ref|.  The delta of order k at
    row t is d = fl32(sum_j f_k[j] * s[clamp(t + j - k W)]) with the sum in float64 (its own rounding, ~1e-16
    relative, is nothing beside the rest), and the reference's d_ref the same over s_ref.  The sum is linear in the
    statics, so the two sums differ by at most sum_j |f_k[j]| * (1e-5 + 1e-4 |s_ref[clamp(t + j - k W)]|); the
    rounding to float32 adds at most 2**-24 of each side's value, together 2**-22 |d_ref| with room for the two
    values not being equal.  Nothing here comes from what the kernel gives."""
    K, W = 2, 2
    with np.load(os.path.join(GOLDEN, "stream_random.npz")) as z:
        g = {k: z[k] for k in z.files if k.startswith(name + "/")}
    with np.load(os.path.join(GOLDEN, "stream_deltas.npz")) as z:
        gd = {k: z[k] for k in z.files if k.startswith(name + "/")}
    comp = build(golden_configs()[name])
    F = comp.num_coeffs
    pieces = []
    for case in range(8):
        n = int(g[f"{name}/{case}/n"])
        pieces.append(np.split(master_signal[50 : 50 + n].astype("f4"), g[f"{name}/{case}/cuts"]))
    with StreamBatch(comp, capacity=B, deltas=Deltas(K)) as sb:
        outs = run_concurrently(sb, [2 * i + 1 for i in range(8)], pieces, np.random.default_rng(11))
    filts = delta_filters(K, W)[1:]
    for case in range(8):
        ref = gd[f"{name}/{case}/deltas"].astype(np.float64)
        assert [len(o) for o in outs[case]] == expected_counts(g[f"{name}/{case}/counts"].tolist(), K * W), (name, case)
        got = np.concatenate(outs[case])
        assert got.dtype == np.float32 and got.shape == ref.shape, (name, case, got.shape, ref.shape)
        assert_features_close(got[:, :F], ref[:, :F], what=(name, case), **F32)
        T = len(ref)
        for k, filt in enumerate(filts, start=1):
            bound = 2.0 ** -22 * np.abs(ref[:, k * F : (k + 1) * F])
            for j, w in enumerate(filt):
                rows = np.clip(np.arange(T) + j - k * W, 0, max(T - 1, 0))
                bound += abs(w) * (1e-5 + 1e-4 * np.abs(ref[rows, :F]))
            err = np.abs(got[:, k * F : (k + 1) * F] - ref[:, k * F : (k + 1) * F])
            assert (err <= bound).all(), (name, case, k, float(err.max()), float((err / bound).max()))
