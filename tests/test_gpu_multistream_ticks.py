"""Degenerate ticks of batched streaming on the GPU, under every stage: empty ticks, ``finalize`` of streams never used,
ticks of empty chunks and ticks of one-sample chunks, for StreamBatch and SiStreamBatch, float32 and float64, without
options and with deltas, pre-emphasis and cmvn together.

Two instances get the same live traffic; one of them also gets the degenerate ticks in between.  A degenerate tick
brings no stream a sample and no frame, so it must change no stream's rows: the two instances' outputs for the live
traffic are compared call by call with np.array_equal (and equal dtypes), the last ``finalize`` included, and the
degenerate calls themselves for their shapes and dtypes."""
import numpy as np
import pytest

from pydrobert_speech_amd.multistream import StreamBatch
from pydrobert_speech_amd.multistream_si import SiStreamBatch
from pydrobert_speech_amd.post import Deltas, Standardize
from tests.test_gpu_multistream import build as build_stft
from tests.test_gpu_multistream_si import build as build_si
from tests.test_multistream_host import golden_configs

pytestmark = pytest.mark.gpu

CAPACITY = 8
LIVE = [6, 0, 3, 5]  # the four live streams, in the order the ticks name them
IDLE = [7, 1]  # never used
KINDS = {"stft": (StreamBatch, lambda: build_stft(golden_configs()["c1_kaldi_fbank"])),
         "si": (SiStreamBatch, lambda: build_si("s1_gabor_mel"))}
OPTIONS = {"plain": lambda: {},
           "all_stages": lambda: dict(deltas=Deltas(2), preemphasis=0.97, cmvn=Standardize())}


def live_traffic(L, dtype, rng):
    """the ticks of the live traffic, each ``(ids, chunks)``: six chunks per live stream of random length in
    ``[1, 3 L]`` -- a random subset of the streams per tick, in random order -- and in the middle one tick in which
    every stream's chunk is one sample long"""
    left = {i: 6 for i in LIVE}
    ticks = []
    while any(left.values()):
        if len(ticks) == 4:
            ids = list(LIVE)
            lens = [1] * len(ids)
        else:
            live = [i for i in LIVE if left[i]]
            ids = [i for i in live if rng.random() < 0.7] or live[:1]
            rng.shuffle(ids)
            lens = rng.integers(1, 3 * L + 1, size=len(ids)).tolist()
            for i in ids:
                left[i] -= 1
        ticks.append((ids, [(3000 * rng.standard_normal(n)).astype(dtype) for n in lens]))
    assert all(len(c) == 1 for c in ticks[4][1]) and len(ticks) > 8
    return ticks


def check_empty(outs, n, C, dtype):
    assert len(outs) == n
    for o in outs:
        assert o.shape == (0, C) and o.dtype == dtype


def degenerate_ticks(sb, dtype, all_started):
    """the ticks that must change nothing, each checked for what it returns"""
    import torch

    C = sb.num_coeffs
    assert sb.compute_chunks([], []) == []
    assert sb.finalize([]) == []
    check_empty(sb.finalize(IDLE), len(IDLE), C, np.float64)  # n > 0, no stream emits
    feats, rows = sb.finalize_packed(IDLE[::-1])
    assert tuple(feats.shape) == (0, C) and rows.tolist() == [0] * (len(IDLE) + 1)
    if all_started:  # (an empty chunk starts a short-integration stream: only once each has had its first samples)
        check_empty(sb.compute_chunks(LIVE, [np.zeros(0, dtype=dtype)] * len(LIVE)), len(LIVE), C, dtype)
        none = torch.zeros(0, dtype=torch.float32 if dtype == np.float32 else torch.float64, device=sb.device)
        feats, rows = sb.compute_chunks_packed(LIVE[::-1], none, [0] * len(LIVE))
        assert tuple(feats.shape) == (0, C) and rows.tolist() == [0] * (len(LIVE) + 1)
        assert feats.dtype == none.dtype


@pytest.mark.parametrize("options", sorted(OPTIONS))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_degenerate_ticks_change_no_streams_rows(kind, dtype, options):
    Batch, build = KINDS[kind]
    comp = build()
    ticks = live_traffic(comp.frame_length, dtype, np.random.default_rng(5))
    with Batch(comp, capacity=CAPACITY, dtype=dtype, **OPTIONS[options]()) as a, \
            Batch(comp, capacity=CAPACITY, dtype=dtype, **OPTIONS[options]()) as b:
        C = a.num_coeffs
        assert C == comp.num_coeffs * (3 if options == "all_stages" else 1)
        fed = set()
        frames = 0
        for t, (ids, chunks) in enumerate(ticks):
            degenerate_ticks(b, dtype, fed == set(LIVE))
            want = a.compute_chunks(ids, chunks)
            got = b.compute_chunks(ids, chunks)
            fed |= set(ids)
            for w, g in zip(want, got):
                assert g.dtype == w.dtype == dtype and g.shape[1] == C
                assert np.array_equal(g, w), (t, float(np.abs(g - w).max()) if g.shape == w.shape else g.shape)
                frames += len(w)
        assert fed == set(LIVE) and frames > 0
        degenerate_ticks(b, dtype, True)
        assert a.started(LIVE).all() and b.started(LIVE).all() and not b.started(IDLE).any()
        want, got = a.finalize(LIVE), b.finalize(LIVE)
        for w, g in zip(want, got):
            assert g.dtype == w.dtype == dtype and g.shape[1] == C
            assert np.array_equal(g, w)
        degenerate_ticks(b, dtype, False)
        assert not b.started(LIVE).any()
