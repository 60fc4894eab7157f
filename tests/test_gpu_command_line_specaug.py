"""``signals-to-torch-feat-dir`` with a ``SpecAugment`` among ``--postprocess``: every file is ``apply_rows`` under
seed ``--seed`` plus the utterance's index of the file written without the stage, bit for bit; the files do not depend
on ``--batch-utts`` (nor on ``--num-workers`` or ``--staging-ring``); and behind a ``vad`` with ``select_last`` the stage
runs on all rows and the selection still drops the rows the decision named."""
import json
import os
import wave

import numpy as np
import pytest

from pydrobert_speech_amd.command_line import signals_to_torch_feat_dir
from pydrobert_speech_amd.post import Cepstra, EnergyVAD, SpecAugment
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

FBANK = {"name": "stft", "bank": {"name": "fbank", "num_filts": 40}, "frame_length_ms": 25, "use_power": True,
         "include_energy": True}
STAGE = {"name": "specaugment", "warp": 2, "fill": "mean"}
SEED = 7
LENGTHS = (None, 9000, 2345, None, 16000)  # None: the fixtures' mono wav file (1200 samples), twice: two indices


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """the map file, and the files written without the stage: once, left unchanged"""
    import torch

    root = tmp_path_factory.mktemp("specaug_cli")
    rng = np.random.default_rng(23)
    lines = []
    for i, n in enumerate(LENGTHS):
        path = os.path.join(ROOT, "tests", "golden", "sig_mono.wav")
        if n is not None:
            path = str(root / f"utt{i}.wav")
            with wave.open(path, "wb") as fh:
                fh.setnchannels(1), fh.setsampwidth(2), fh.setframerate(16000)
                fh.writeframes((rng.standard_normal(n) * 3000).astype("<i2").tobytes())
        lines.append(f"utt{i} {path}")
    map_path = root / "map.txt"
    map_path.write_text("\n".join(lines) + "\n")
    plain = str(root / "plain")
    assert signals_to_torch_feat_dir([str(map_path), json.dumps(FBANK), plain]) == 0
    statics = [torch.load(os.path.join(plain, f"utt{i}.pt"), weights_only=True) for i in range(len(LENGTHS))]
    frames = [x.shape[0] for x in statics]
    assert [tuple(x.shape)[1] for x in statics] == [41] * len(LENGTHS) and min(frames) >= 7 and max(frames) > 60
    return root, str(map_path), statics


def load(out_dir, n=len(LENGTHS)):
    import torch

    return [torch.load(os.path.join(out_dir, f"utt{i}.pt"), weights_only=True) for i in range(n)]


def test_files_are_apply_rows_of_the_plain_files_however_batched(corpus):
    import torch

    root, map_path, statics = corpus
    post = SpecAugment(warp=2, fill="mean")
    want = []
    for i, x in enumerate(statics):
        got = post.apply_rows(x.cuda(), [0, x.shape[0]], seeds=[SEED + i]).cpu()
        assert not torch.equal(got, x)  # (the stage does something to every file)
        want.append(got)
    assert not torch.equal(want[0], want[3])  # one file under two indices: two keys
    runs = {"1": ["--batch-utts", "1"], "3": ["--batch-utts", "3"], "256": ["--batch-utts", "256"],
            "workers": ["--batch-utts", "2", "--num-workers", "2"], "ring": ["--batch-utts", "3", "--staging-ring"],
            "samples": ["--batch-samples", "12000"]}
    for name, extra in runs.items():
        out_dir = str(root / f"aug_{name}")
        args = [map_path, json.dumps(FBANK), out_dir, "--postprocess", json.dumps([STAGE]), "--seed", str(SEED)]
        assert signals_to_torch_feat_dir(args + extra) == 0
        for i, got in enumerate(load(out_dir)):
            assert got.dtype == torch.float32 and tuple(got.shape) == tuple(statics[i].shape)  # row counts unchanged
            assert got.numpy().tobytes() == want[i].numpy().tobytes(), (name, i)
    # another seed, another copy of the corpus
    out_dir = str(root / "aug_other")
    args = [map_path, json.dumps(FBANK), out_dir, "--postprocess", json.dumps([STAGE]), "--seed", str(SEED + 100)]
    assert signals_to_torch_feat_dir(args) == 0
    assert any(got.numpy().tobytes() != want[i].numpy().tobytes() for i, got in enumerate(load(out_dir)))


def test_behind_a_vad_with_select_last(corpus):
    import torch

    root, map_path, statics = corpus
    out_dir = str(root / "vad")
    mfcc = {"name": "mfcc", "energy": True}
    # (the threshold is the utterance's mean log energy: some frames lie above it, some below)
    vad = {"name": "vad", "energy_threshold": 0.0, "energy_mean_scale": 1.0, "select_last": True}
    spec = json.dumps([mfcc, vad, STAGE])
    assert signals_to_torch_feat_dir([map_path, json.dumps(FBANK), out_dir, "--postprocess", spec, "--seed", str(SEED),
                                      "--batch-utts", "3"]) == 0
    ceps, decide, post = Cepstra(energy=True), EnergyVAD(0.0, 1.0), SpecAugment(warp=2, fill="mean")
    kept = 0
    for i, x in enumerate(statics):
        got = torch.load(os.path.join(out_dir, f"utt{i}.pt"), weights_only=True).numpy()
        c = ceps.apply(x.cuda(), axis=-1)
        voiced = decide.decide(c).cpu().numpy().astype(bool)  # decided on the rows as the stage found them ...
        augmented = post.apply_rows(c, [0, c.shape[0]], seeds=[SEED + i]).cpu().numpy()  # ... augmented, all of them ...
        want = augmented[voiced]  # ... and dropped behind the last stage
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), i
        kept += int(voiced.sum())
    assert 0 < kept < sum(x.shape[0] for x in statics)
