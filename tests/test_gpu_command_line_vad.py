"""``signals-to-torch-feat-dir`` with an ``EnergyVAD`` among the post-processors, in Kaldi's order -- MFCCs with the
energy, the decision, sliding-window CMVN over all frames, then the selection -- and with the rows dropped where the
stage stands: every file is the offline composition over the file written without post-processors, bit for bit, and an
utterance of silence is written as a ``(0, F)`` tensor."""
import json
import os

import numpy as np
import pytest

from pydrobert_speech_amd.command_line import signals_to_torch_feat_dir
from pydrobert_speech_amd.post import Cepstra, EnergyVAD, SlidingCMVN

pytestmark = pytest.mark.gpu

FBANK = {"name": "stft", "bank": {"name": "fbank", "num_filts": 40}, "frame_length_ms": 25, "use_power": True,
         "include_energy": True}
MFCC = {"name": "mfcc", "energy": True}
SLIDING = {"name": "sliding_cmvn", "cmn_window": 30}
SILENT = 2


def signals():
    """a handful of short signals with loud and quiet stretches (voiced and unvoiced frames); one is silence"""
    rng = np.random.default_rng(31)
    out = []
    for i, n in enumerate((8000, 5000, 3000, 12000, 700)):
        x = 3.0 * rng.standard_normal(n)
        for start in range(int(rng.integers(0, 1500)), n, 3000):
            x[start : start + 1400] *= 1000.0
        out.append((np.zeros(n) if i == SILENT else x).astype(np.float32))
    return out


def run_tool(tmp_path, name, post):
    out_dir = str(tmp_path / name)
    args = [str(tmp_path / "map.txt"), json.dumps(FBANK), out_dir]
    if post is not None:
        args += ["--postprocess", json.dumps(post)]
    assert signals_to_torch_feat_dir(args) == 0
    return out_dir


def test_files_are_the_offline_composition(tmp_path, monkeypatch):
    import torch

    sigs = signals()
    lines = []
    for i, x in enumerate(sigs):
        path = str(tmp_path / f"utt{i}.npy")
        np.save(path, x)
        lines.append(f"utt{i} {path}")
    (tmp_path / "map.txt").write_text("\n".join(lines) + "\n")
    plain = run_tool(tmp_path, "plain", None)
    calls = []
    for method in ("decide_rows", "select_rows", "apply_rows"):
        real = getattr(EnergyVAD, method)

        def counted(self, feats, *args, _real=real, _name=method):
            calls.append((_name, tuple(feats.shape)))
            return _real(self, feats, *args)

        monkeypatch.setattr(EnergyVAD, method, counted)
    last = run_tool(tmp_path, "last", [MFCC, dict(name="vad", select_last=True), SLIDING])
    calls_last = list(calls)
    del calls[:]
    here = run_tool(tmp_path, "here", [MFCC, "vad", SLIDING])
    calls_here = list(calls)
    monkeypatch.undo()

    statics = [torch.load(os.path.join(plain, f"utt{i}.pt"), weights_only=True).numpy() for i in range(len(sigs))]
    frames = [x.shape[0] for x in statics]
    assert [x.shape[1] for x in statics] == [41] * len(sigs) and min(frames) >= 3 and max(frames) > 60
    # the whole packed batch went through one decision and one selection
    total = sum(frames)
    assert calls_last == [("decide_rows", (total, 13)), ("select_rows", (total, 13))]
    assert calls_here[0] == ("apply_rows", (total, 13)) and [c[0] for c in calls_here] == ["apply_rows", "decide_rows"]
    ceps, vad, sliding = Cepstra(energy=True), EnergyVAD(), SlidingCMVN(30)
    kept = []
    for i, x in enumerate(statics):
        c = ceps.apply(x)
        assert c.dtype == np.float32 and c.shape == (frames[i], 13) and (c[:, 0] == x[:, 0]).all()
        voiced = vad.decide(c)
        kept.append(int(voiced.sum()))
        # Kaldi's order: normalised over all frames, then selected by the decisions taken before the normalisation
        want = sliding.apply(c)[voiced]
        got = torch.load(os.path.join(last, f"utt{i}.pt"), weights_only=True)
        assert got.dtype == torch.float32 and tuple(got.shape) == (kept[i], 13), i
        assert got.numpy().tobytes() == np.ascontiguousarray(want).tobytes(), i
        # dropped where the stage stands: the normalisation sees the voiced frames only
        want = sliding.apply(vad.apply(c))
        assert want.shape == (kept[i], 13) and (vad.apply(c) == c[voiced]).all()
        got = torch.load(os.path.join(here, f"utt{i}.pt"), weights_only=True)
        assert got.dtype == torch.float32 and tuple(got.shape) == (kept[i], 13), i
        assert got.numpy().tobytes() == np.ascontiguousarray(want).tobytes(), i
    # silence: no frame is above its own threshold; the others keep some frames and drop some
    assert kept[SILENT] == 0 and frames[SILENT] > 10
    assert all(0 < k < n for i, (k, n) in enumerate(zip(kept, frames)) if i != SILENT and n > 10)
