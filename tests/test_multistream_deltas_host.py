"""Delta features of batched streaming on the host, no device (multistream.DeltaState, multistream.streaming_deltas):
the delayed row count of every call, the index logic of pds_multistream_deltas (clamp, delay, history of 2 H rows)
emulated in numpy from the host bookkeeping alone against the oracle's whole-utterance deltas, and the constructor
contract."""
import json

import numpy as np
import pytest

from oracle.stft_oracle import delta_filters, deltas as oracle_deltas
from pydrobert_speech_amd.multistream import DeltaState, StreamBatch, StreamState, streaming_deltas
from pydrobert_speech_amd.post import Deltas, Stack
from tests.test_multistream_host import build, golden_configs

KW = [(1, 1), (2, 2), (3, 2), (2, 3)]
FLAG_HALF, FLAG_FINAL = 1, 2


def totals_of(H):
    """the total frame counts at which the delay, the clamp or the history changes behaviour"""
    return [0, 1, 2, H, H + 1, 2 * H, 2 * H + 1, 2 * H + 2, 5 * H]


# ---- 1. row counts ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("K,W", KW)
@pytest.mark.parametrize("name", ["c1_kaldi_fbank", "c2_tri_mel40"])
def test_row_counts_follow_the_delay_rule(name, K, W):
    comp = build(golden_configs()[name])
    L, H, B = comp.frame_length, K * W, 16
    state = StreamState(B, L, comp.frame_shift, comp.pad_left)
    dstate = DeltaState(B, H)
    rng = np.random.default_rng(21)
    n, e = [0] * B, [0] * B  # static frames produced / rows returned in the stream's current life
    lives = 0
    for _ in range(80):
        ids = np.flatnonzero(rng.random(B) < 0.5)
        rng.shuffle(ids)
        lens = rng.integers(0, 3 * L + 1, size=len(ids))
        lens[rng.random(len(ids)) < 0.3] = 0
        lens[rng.random(len(ids)) < 0.2] = 1
        step = state.chunk_step(ids, lens)
        dstep = dstate.step(ids, step["k"])
        for i, k, rows in zip(ids.tolist(), step["k"].tolist(), dstep["rows"].tolist()):
            n[i] += k
            assert rows == max(0, n[i] - H) - e[i], (i, n[i], e[i], rows)
            e[i] += rows
        state.commit_chunks(ids, step)
        dstate.commit(ids, dstep)
        fin = np.flatnonzero(rng.random(B) < 0.1)  # (ids are reused afterwards)
        rng.shuffle(fin)
        step = state.finalize_step(fin)
        dstep = dstate.step(fin, step["k"], final=True)
        for i, k, rows in zip(fin.tolist(), step["k"].tolist(), dstep["rows"].tolist()):
            n[i] += k
            assert rows == n[i] - e[i]
            n[i] = e[i] = 0  # per life, the counts sum to the stream's static frames
            lives += 1
        state.reset(fin)
        dstate.commit(fin, dstep)
        assert (dstate.seen[fin] == 0).all() and (dstate.valid[fin] == 0).all()
        assert (dstate.valid == np.minimum(dstate.seen, 2 * H)).all()
        assert (dstate.seen - dstate.emitted == np.minimum(dstate.seen, H)).all()
    assert lives > 20


# ---- 2. index logic against the oracle ----------------------------------------------------------------------------


def emulate_tick(hist, filts, dstate, ids, fresh, final):
    """pds_multistream_deltas of one tick in numpy, from the metadata DeltaState.fill_meta writes (include/pds_amd.h):
    `hist` is the pool float64[2, capacity, 2 H, F], `fresh` the list of the streams' new static rows.  Returns each
    stream's output rows and advances `hist` and `dstate`."""
    F = hist.shape[-1]
    K = len(filts)
    ids = np.asarray(ids, dtype=np.int64)
    k = np.asarray([len(x) for x in fresh], dtype=np.int64)
    statics = np.concatenate(fresh) if len(fresh) else np.zeros((0, F))
    step = dstate.step(ids, k, final=final)
    out_rows = np.concatenate([[0], np.cumsum(step["rows"])])
    static_rows = np.concatenate([[0], np.cumsum(k)])
    meta = np.zeros((len(ids), 8), dtype=np.int64)
    prefix = np.zeros(len(ids) + 1, dtype=np.int64)
    total = dstate.fill_meta(meta, prefix, ids, step, static_rows[:-1], out_rows[:-1], F)
    out = np.full((int(out_rows[-1]), (K + 1) * F), np.nan)
    new_hist = hist.copy()
    elems = 0
    for e, (s, flags, valid, kk, srow, first, rows, orow) in enumerate(meta.tolist()):
        half, fin = flags & FLAG_HALF, bool(flags & FLAG_FINAL)
        assert fin == final
        seq = np.concatenate([hist[half, s, :valid], statics[srow : srow + kk]])
        V = len(seq)
        keep = 0 if fin else min(V, hist.shape[2])
        assert prefix[e] == elems
        elems += (rows + keep) * F
        if rows:
            p = first + np.arange(rows)
            block = [seq[np.clip(p, 0, V - 1)]]
            for filt in filts:
                M = (len(filt) - 1) // 2
                acc = np.zeros((rows, F))
                for j, w in enumerate(filt):
                    acc += w * seq[np.clip(p + j - M, 0, V - 1)]
                block.append(acc)
            out[orow : orow + rows] = np.concatenate(block, axis=1)
        if keep:
            new_hist[1 - half, s, :keep] = seq[V - keep :]
    assert total == elems == prefix[-1]
    hist[...] = new_hist
    dstate.commit(ids, step)
    assert not np.isnan(out).any()
    return [out[a:b] for a, b in zip(out_rows[:-1], out_rows[1:])]


def split_total(total, H, rng, big):
    """frames per compute_chunks call of a stream of `total` frames: runs of 0-frame ticks, mostly one frame, and with
    `big` one call of more than 2 H frames where the total allows it"""
    ks, left = [0, 0], total
    if big and left > 2 * H + 1:
        ks.append(int(rng.integers(0, 2)))
        ks.append(2 * H + 1 + int(rng.integers(0, left - ks[-1] - 2 * H)))
        left = total - sum(ks)
    while left:
        if rng.random() < 0.3:
            ks += [0] * int(rng.integers(1, 4))
        k = min(left, int(rng.choice([1, 1, 1, 2, 3, H, H + 1])))
        ks.append(k)
        left -= k
    return ks + [0] * int(rng.integers(0, 3))


@pytest.mark.parametrize("K,W", KW)
def test_emulated_kernel_equals_whole_utterance_deltas(K, W):
    H, F, B = K * W, 5, 16
    rng = np.random.default_rng(100 * K + W)
    filts = delta_filters(K, W)[1:]
    dstate = DeltaState(B, H)
    assert dstate.hist_rows == 2 * H
    hist = rng.standard_normal((2, B, 2 * H, F))  # (stale rows must never be read)
    # two rounds over the same ids: every total once fed frame by frame and once with a > 2 H tick, ids reused
    plans = []
    for big in (False, True):
        order = rng.permutation(len(totals_of(H)))
        plans.append([(totals_of(H)[t], split_total(totals_of(H)[t], H, rng, big)) for t in order])
    sids = rng.permutation(B)[: len(totals_of(H))]
    saw_big = False
    for plan in plans:
        X = [rng.standard_normal((total, F)) for total, _ in plan]
        at = [0] * len(plan)  # frames fed
        nxt = [0] * len(plan)  # calls made
        got = [[] for _ in plan]
        counts = [[] for _ in plan]
        done = [False] * len(plan)
        while not all(done):
            live = [i for i in range(len(plan)) if not done[i]]
            tick = [i for i in live if rng.random() < 0.6] or live[:1]
            rng.shuffle(tick)
            feed = [i for i in tick if nxt[i] < len(plan[i][1])]
            fin = [i for i in tick if nxt[i] >= len(plan[i][1])]
            if feed:
                fresh = [X[i][at[i] : at[i] + plan[i][1][nxt[i]]] for i in feed]
                saw_big |= any(len(x) > 2 * H for x in fresh)
                for i, y in zip(feed, emulate_tick(hist, filts, dstate, sids[feed], fresh, final=False)):
                    at[i] += plan[i][1][nxt[i]]
                    nxt[i] += 1
                    assert len(y) == max(0, at[i] - H) - sum(counts[i])
                    got[i].append(y)
                    counts[i].append(len(y))
            if fin:
                empty = [np.zeros((0, F))] * len(fin)  # (the frames of finalize are covered by the tick above)
                for i, y in zip(fin, emulate_tick(hist, filts, dstate, sids[fin], empty, final=True)):
                    got[i].append(y)
                    done[i] = True
        for i, (total, ks) in enumerate(plan):
            assert at[i] == total == sum(ks)
            rows = np.concatenate(got[i])
            want = oracle_deltas(X[i], axis=0, num_deltas=K, context_window=W)
            assert rows.shape == want.shape == (total, (K + 1) * F)
            assert np.array_equal(rows, want), (K, W, total, ks, float(np.abs(rows - want).max()))
    assert saw_big


def test_finalize_brings_its_own_frames():
    # finalize of the STFT state machine usually adds frames: they join the sequence before the right edge
    K, W, F = 2, 2, 3
    H = K * W
    rng = np.random.default_rng(5)
    filts = delta_filters(K, W)[1:]
    for total, last in [(1, 1), (H + 1, 1), (2 * H + 3, 2), (3, 3)]:
        dstate = DeltaState(4, H)
        hist = rng.standard_normal((2, 4, 2 * H, F))
        X = rng.standard_normal((total, F))
        got = emulate_tick(hist, filts, dstate, [2], [X[: total - last]], final=False)
        got += emulate_tick(hist, filts, dstate, [2], [X[total - last :]], final=True)
        assert np.array_equal(np.concatenate(got), oracle_deltas(X, axis=0, num_deltas=K, context_window=W))


# ---- 3. the constructor contract ----------------------------------------------------------------------------------


def test_deltas_settings_are_checked():
    comp = build(golden_configs()["c1_kaldi_fbank"])
    bad = [
        Deltas(2, pad_mode="reflect"),
        Deltas(2, pad_mode="constant"),
        Deltas(2, pad_mode="edge", stat_length=2),  # pad kwargs
        Deltas(2, concatenate=False),
        Deltas(2, target_axis=0),
        Deltas(2, target_axis=2),
        Deltas(-1),
        Stack(2),
        {"name": "deltas", "num_deltas": 2, "pad_mode": "wrap"},
        {"name": "stack", "num_vectors": 2},
        {"num_deltas": 2},
        3,
    ]
    for d in bad:
        with pytest.raises(ValueError):
            streaming_deltas(d)
        with pytest.raises(ValueError):  # (before anything touches a device)
            StreamBatch(comp, capacity=4, deltas=d)
    for d, (K, W) in [(Deltas(2), (2, 2)), (Deltas(1, target_axis=1, context_window=3), (1, 3)),
                      ({"name": "deltas", "num_deltas": 3}, (3, 2)),
                      (json.loads('{"alias": "deltas", "num_deltas": 2, "context_window": 1}'), (2, 1))]:
        inst, k, w = streaming_deltas(d)
        assert isinstance(inst, Deltas) and (k, w) == (K, W)
    # num_deltas == 0 is accepted and means no deltas
    assert streaming_deltas(Deltas(0)) is None and streaming_deltas(None) is None
    assert streaming_deltas({"name": "deltas", "num_deltas": 0}) is None
    with pytest.raises(ValueError):
        streaming_deltas(Deltas(0, concatenate=False))  # (still checked)
    with pytest.raises(ValueError):
        DeltaState(0, 4)
    with pytest.raises(ValueError):
        DeltaState(4, 0)
