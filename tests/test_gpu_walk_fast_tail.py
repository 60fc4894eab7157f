"""The row-segment walk's straight-line tail for full items (csrc/stft_wave_kernel.h, FTAIL) against the general rounds.

An item is four consecutive frames of one utterance.  In a launch with one round of 12-bin segments and logged features
(the headline bank's), an item whose four frames all exist takes a tail without a branch; an utterance's last item with
one to three frames, and every item of every other launch, takes the general rounds as before.  PDS_STFT_FAST_TAIL=0 in
the environment (read per launch) sends every item through the general rounds: the same library, both ways.

Frame counts 1 ... 9 and 41 in packed batches of three give items of one, two, three and four frames, at an utterance's
end and in its middle, and utterances that are nothing but a partial item.  Per case: every row bit-equal between the
two launches, nothing written outside the utterances' rows and the bank's columns (sentinel-filled wider buffers), and
every utterance against oracle.stft_oracle.compute_full at the suite's float32 rule, 1e-5 + 1e-4 |ref|.

Which path a launch takes is read off its plan (PDS_DEBUG_PLAN prints the row-segment table's rounds and segment
length when the plan is created): the headline bank must have the fast shape, the 80-filter bank must not.  With
use_log off no launch has it, and the statics + deltas kernels are built without the tail.  The energy column is stored
in front of the walk and is no part of the shape: that case runs whichever path its table gives.
"""
import re

import numpy as np
import pytest

from oracle import stft_oracle as orc
from pydrobert_speech_amd import config
from tests.conftest import assert_features_close
from tests.test_gpu_walk_tail import F32, build, check_buffer, launch_into_sentinel, params

pytestmark = pytest.mark.gpu

TRI40 = {"name": "tri", "scaling_function": "mel", "num_filts": 40}
CONFIGS = {
    # the headline bank: tri / mel / 40, 25 ms frames every 10 ms at 16 kHz
    "tri_mel40": {"name": "stft", "bank": TRI40, "frame_length_ms": 25, "frame_shift_ms": 10,
                  "window_function": "hanning", "use_power": True},
    "tri_mel40_linear": {"name": "stft", "bank": TRI40, "frame_length_ms": 25, "frame_shift_ms": 10,
                         "window_function": "hanning", "use_power": True, "use_log": False},
    "fbank40_energy": {"name": "stft", "bank": {"name": "fbank", "num_filts": 40}, "frame_length_ms": 25,
                       "include_energy": True, "use_power": True},
    "fbank80": {"name": "stft", "bank": {"name": "fbank", "num_filts": 80}, "frame_length_ms": 25, "use_power": True},
}
# frames per utterance, three utterances per packed batch
BATCHES = [(1, 4, 7), (2, 5, 8), (3, 9, 41)]


def built(name, monkeypatch, capfd):
    """The computer, and (walk, rounds, segment length) of its plan's row-segment table"""
    monkeypatch.setenv("PDS_DEBUG_PLAN", "1")
    comp = build(CONFIGS[name])
    plan = comp._native_plan()
    lines = re.findall(r"rseg rounds (\d+) len (\d+) .*-> walk (\d+)", capfd.readouterr().err)
    monkeypatch.delenv("PDS_DEBUG_PLAN")
    assert lines, "the plan's creation printed its walks"
    rounds, seg_len, walk = (int(v) for v in lines[-1])
    assert plan.geometry == (32, 16, 25) and comp.kernel_kind == 512
    return comp, (walk, rounds, seg_len)


def length_of(comp, frames):
    n = max(frames * comp.frame_shift + 7, comp.frame_length // 2 + 10)  # (a signal needs half a frame to have a frame)
    assert comp.num_frames(n) == frames
    return n


def signals(comp, frames, seed):
    rng = np.random.default_rng(seed)
    return [(3000 * rng.standard_normal(length_of(comp, f))).astype("f4") for f in frames]


def both_ways(monkeypatch, run):
    """run() with the fast tail and with every item sent through the general rounds"""
    fast = run()
    monkeypatch.setenv("PDS_STFT_FAST_TAIL", "0")
    slow = run()
    monkeypatch.delenv("PDS_STFT_FAST_TAIL")
    return fast, slow


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_case(comp, sigs, monkeypatch, what):
    import torch

    C = comp.num_coeffs
    (fast, rows), (slow, _) = both_ways(
        monkeypatch, lambda: launch_into_sentinel(comp, sigs, "f4", torch.float32, extra_rows=5, width=C + 3))
    differ = np.flatnonzero((bits(fast) != bits(slow)).any(axis=1))
    assert differ.size == 0, (what, "rows differ between the two tails", differ[:8].tolist())
    check_buffer(fast, rows, C, sigs, params(comp), what)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_fast_tail_matches_the_general_rounds(name, ragged, monkeypatch, capfd):
    monkeypatch.setattr(config, "RAGGED_SCHEDULING", ragged)
    comp, (walk, rounds, seg_len) = built(name, monkeypatch, capfd)
    assert walk == 2, (name, "the row-segment walk serves this bank")
    fast_shape = rounds == 1 and seg_len == 12 and bool(comp._log)
    if name == "tri_mel40":
        assert fast_shape, (name, rounds, seg_len)
    if name in ("tri_mel40_linear", "fbank80"):
        assert not fast_shape, (name, rounds, seg_len)
    for i, frames in enumerate(BATCHES):
        check_case(comp, signals(comp, frames, 20 + i), monkeypatch, (name, ragged, frames))


def test_deltas_launch_keeps_the_general_rounds(monkeypatch, capfd):
    """Statics + deltas in one launch: kernels built without the fast tail, the same rows either way"""
    import torch

    from pydrobert_speech_amd.post import Deltas

    comp, _ = built("tri_mel40", monkeypatch, capfd)
    p, C = params(comp), comp.num_coeffs
    for i, frames in enumerate(BATCHES):
        sigs = signals(comp, frames, 30 + i)
        lens = [len(x) for x in sigs]
        dev = torch.from_numpy(np.concatenate(sigs)).cuda()
        layout = comp.prepare_layout(np.concatenate([[0], np.cumsum(lens)[:-1]]), lens, device=dev.device)
        fast, slow = both_ways(
            monkeypatch, lambda: comp.launch_with_deltas(dev, layout, Deltas(2), fused=True).cpu().numpy())
        assert fast.shape == (layout.row_offsets[-1], 3 * C) and (bits(fast) == bits(slow)).all()
        for b, x in enumerate(sigs):
            mine = fast[layout.row_offsets[b] : layout.row_offsets[b + 1]]
            assert_features_close(mine[:, :C], orc.compute_full(x, p), what=("deltas", frames, b), **F32)
            assert np.allclose(mine, orc.deltas(mine[:, :C], axis=0, num_deltas=2, target_axis=-1), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("ragged", [False, True])
def test_nan_sample_poisons_its_frames_only(ragged, monkeypatch, capfd):
    """One NaN sample in the middle of the long utterance and one in a partial item: NaN in exactly the frames the oracle
    poisons, on both tails"""
    monkeypatch.setattr(config, "RAGGED_SCHEDULING", ragged)
    comp, (_, rounds, seg_len) = built("tri_mel40", monkeypatch, capfd)
    assert (rounds, seg_len) == (1, 12)
    sigs = signals(comp, (3, 9, 41), 40)
    sigs[0][len(sigs[0]) // 2] = np.nan
    sigs[2][20 * comp.frame_shift + 5] = np.nan
    with np.errstate(all="ignore"):
        want = orc.compute_full(sigs[2], params(comp))
        poisoned = np.isnan(want).all(axis=1)
        assert 0 < poisoned.sum() < len(want) and (np.isnan(want).any(axis=1) == poisoned).all()
        check_case(comp, sigs, monkeypatch, ("nan", ragged))  # (compares the NaN positions with the oracle's)
