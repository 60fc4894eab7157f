"""Bookkeeping of batched streaming (multistream.StreamState) on the host, no device: the frame counts of every call of
the golden chunkings, and each tick's work spans, carries and pads against the single-stream state machine of
compute.py (STFTFrameComputer.compute_chunk / finalize) run with dummy features."""
import json
import os

import numpy as np
import pytest

from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg
from pydrobert_speech_amd.compute import FrameComputer
from pydrobert_speech_amd.multistream import StreamBatch, StreamState
from tests.conftest import GOLDEN

RANDOM_NAMES = ["c1_kaldi_fbank", "c2_tri_mel40", "v_tri_analytic_nolog", "v_gabor_nopad_mag"]
EXTRA = {
    "causal": {"name": "stft", "bank": "fbank", "frame_length_ms": 25, "frame_style": "causal"},
    "centered": {"name": "stft", "bank": "fbank", "frame_length_ms": 25, "frame_style": "centered"},
    "shift_gt_length": {"name": "stft", "bank": "fbank", "frame_length_ms": 10, "frame_shift_ms": 25},
    "shift_gt_length_causal": {"name": "stft", "bank": "fbank", "frame_length_ms": 10, "frame_shift_ms": 25,
                               "frame_style": "causal"},
}


def build(cfg):
    return alias_factory_subclass_from_arg(FrameComputer, json.loads(json.dumps(cfg)))


def golden_configs():
    with open(os.path.join(GOLDEN, "configs.json")) as fh:
        return json.load(fh)["configs"]


def state_of(comp, capacity):
    return StreamState(capacity, comp.frame_length, comp.frame_shift, comp.pad_left)


def replay(state, pieces, rng):
    """All streams of `pieces` (one list of chunk lengths each) concurrently: in every tick a random subset of the
    streams that still have chunks gets its next one, in random order; a stream whose chunks are done is finalized in
    a later random tick.  Returns the frame count of every call, per stream."""
    nxt = [0] * len(pieces)
    done = [False] * len(pieces)
    counts = [[] for _ in pieces]
    while not all(done):
        live = [i for i in range(len(pieces)) if not done[i]]
        tick = [i for i in live if rng.random() < 0.6] or live[:1]
        rng.shuffle(tick)
        feed = [i for i in tick if nxt[i] < len(pieces[i])]
        fin = [i for i in tick if nxt[i] >= len(pieces[i])]
        if feed:
            ids = np.asarray(feed)
            step = state.chunk_step(ids, np.asarray([pieces[i][nxt[i]] for i in feed]))
            state.commit_chunks(ids, step)
            for i, k in zip(feed, step["k"].tolist()):
                counts[i].append(k)
                nxt[i] += 1
        if fin:
            ids = np.asarray(fin)
            step = state.finalize_step(ids)
            state.reset(ids)
            for i, k in zip(fin, step["k"].tolist()):
                counts[i].append(k)
                done[i] = True
    return counts


@pytest.mark.parametrize("name", RANDOM_NAMES)
def test_frame_counts_of_the_random_chunkings(name):
    # tests/golden/make_golden_stream.py: the reference's frame count of every compute_chunk / finalize call
    comp = build(golden_configs()[name])
    with np.load(os.path.join(GOLDEN, "stream_random.npz")) as z:
        g = {k: z[k] for k in z.files if k.startswith(name + "/")}
    pieces = []
    for case in range(8):
        n = int(g[f"{name}/{case}/n"])
        cuts = np.concatenate([[0], g[f"{name}/{case}/cuts"], [n]])
        pieces.append(np.diff(cuts).tolist())
    counts = replay(state_of(comp, 8), pieces, np.random.default_rng(1))
    for case in range(8):
        assert counts[case] == g[f"{name}/{case}/counts"].tolist(), (name, case)


def stream_chunkings(n, L):
    """the chunkings of tests/golden/stream.npz (tests/test_gpu_stft.py): tag -> chunk lengths of an n-sample signal"""
    out = {}
    for tag, chunks in (("c7", [7] * (n // 7 + 1)), ("c1024", [1024] * (n // 1024 + 1)),
                        ("mixed", [1, 0, 3 * L, 50, 1, 10 ** 6])):
        if tag == "c7" and n > 3000:
            continue
        lens, pos = [], 0
        for c in chunks:
            if pos >= n:
                break
            lens.append(min(c, n - pos))
            pos += c
        out[tag] = lens
    return out


def test_row_totals_of_the_fixed_chunkings(golden_stream):
    rng = np.random.default_rng(2)
    for name, cfg in sorted(golden_configs().items()):
        if f"{name}/c1024" not in golden_stream:
            continue
        comp = build(cfg)
        chunkings = stream_chunkings(5 * comp.frame_length, comp.frame_length)
        tags = [t for t in chunkings if f"{name}/{t}" in golden_stream]
        counts = replay(state_of(comp, 3), [chunkings[t] for t in tags], rng)
        for tag, c in zip(tags, counts):
            assert sum(c) == len(golden_stream[f"{name}/{tag}"]), (name, tag)


class _Recorder:
    """stands in for a computer's _run_host_signal: records (samples, frames, left pad) and returns zeros"""

    def __init__(self, comp):
        self.C, self.calls = comp.num_coeffs, []

    def __call__(self, signal, nframes, pad_left):
        self.calls.append((len(signal), int(nframes), int(pad_left)))
        return np.zeros((nframes, self.C), dtype=signal.dtype)


@pytest.mark.parametrize("name", ["c1_kaldi_fbank", "c5_gammatone64_48k"] + sorted(EXTRA))
def test_ticks_follow_the_single_stream_state_machine(name):
    cfg = EXTRA.get(name) or golden_configs()[name]
    L = build(cfg).frame_length
    B = 24
    comps = [build(cfg) for _ in range(B)]
    recs = []
    for comp in comps:
        recs.append(_Recorder(comp))
        comp._run_host_signal = recs[-1]
    if name.startswith("shift_gt"):
        assert comps[0].frame_shift > comps[0].frame_length
    state = state_of(comps[0], B + 5)
    rng = np.random.default_rng(3)
    sid = rng.permutation(B + 5)[:B]  # streams live at arbitrary ids
    for _ in range(60):
        tick = np.flatnonzero(rng.random(B) < 0.5)
        rng.shuffle(tick)
        fin = tick[rng.random(len(tick)) < 0.15]
        feed = np.setdiff1d(tick, fin)
        rng.shuffle(feed)
        lens = rng.integers(0, 3 * L + 1, size=len(feed))
        lens[rng.random(len(feed)) < 0.1] = 0
        lens[rng.random(len(feed)) < 0.1] = 1
        step = state.chunk_step(sid[feed], lens)
        for j, (b, n) in enumerate(zip(feed, lens)):
            before = len(recs[b].calls)
            got = comps[b].compute_chunk(np.zeros(n, np.float32))
            assert len(got) == step["k"][j]
            if step["k"][j]:
                assert recs[b].calls[before:] == [(step["avail"][j], step["k"][j], step["cp"][j])]
        state.commit_chunks(sid[feed], step)
        for b in feed:
            s = sid[b]
            assert (state.carry_len[s], state.carry_pad[s], state.skip[s]) == (
                len(comps[b]._carry), comps[b]._carry_pad, comps[b]._skip), (name, b)
            assert state.carry_len[s] < L
        step = state.finalize_step(sid[fin])
        for j, b in enumerate(fin):
            before = len(recs[b].calls)
            assert len(comps[b].finalize()) == step["k"][j]
            if step["k"][j]:
                assert recs[b].calls[before:] == [(step["carry_len"][j], step["k"][j], step["cp"][j])]
        state.reset(sid[fin])
        assert state.started[sid].tolist() == [c.started for c in comps]


def test_stream_ids_are_checked():
    state = StreamState(10, 400, 160, 199)
    assert state.check_ids([3, 0, 9]).tolist() == [3, 0, 9]
    assert state.check_ids([]).tolist() == []
    for bad in ([1, 1], [-1], [10], [0.5], [[1, 2]]):
        with pytest.raises(ValueError):
            state.check_ids(bad)
    with pytest.raises(ValueError):
        StreamState(0, 400, 160, 199)


def test_short_integration_is_refused():
    si = build({"name": "si", "bank": {"name": "gabor", "scaling_function": "mel"}})
    with pytest.raises(TypeError):
        StreamBatch(si)
