"""``signals-to-torch-feat-dir`` with a ``PCEN`` among ``--postprocess``: every file is ``PCEN.apply`` of the file
written without the stage, bit for bit, with and without ``--staging-ring``; the packed batch goes through one
``apply_rows`` call where it stands, row counts unchanged; the stage works in front of a ``vad`` with ``select_last``;
and a computer whose config takes logs is refused."""
import json
import os

import numpy as np
import pytest

from pydrobert_speech_amd.command_line import signals_to_torch_feat_dir
from pydrobert_speech_amd.post import PCEN, EnergyVAD, SlidingCMVN

pytestmark = pytest.mark.gpu

FBANK = {"name": "stft", "bank": {"name": "fbank", "num_filts": 40}, "frame_length_ms": 25, "use_power": True,
         "use_log": False, "include_energy": True}
LENGTHS = (4000, 700, 2345)  # three short files
POST = '[{"name": "pcen", "smooth": 0.025}]'


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """the map file, and the files written without the stage: once, left unchanged"""
    import torch

    root = tmp_path_factory.mktemp("pcen_cli")
    rng = np.random.default_rng(17)
    lines = []
    for i, n in enumerate(LENGTHS):
        path = str(root / f"utt{i}.npy")
        np.save(path, (3000 * rng.standard_normal(n)).astype(np.float32))
        lines.append(f"utt{i} {path}")
    map_path = root / "map.txt"
    map_path.write_text("\n".join(lines) + "\n")
    plain = str(root / "plain")
    assert signals_to_torch_feat_dir([str(map_path), json.dumps(FBANK), plain]) == 0
    statics = [torch.load(os.path.join(plain, f"utt{i}.pt"), weights_only=True) for i in range(len(LENGTHS))]
    frames = [x.shape[0] for x in statics]
    assert [tuple(x.shape)[1] for x in statics] == [41] * 3 and min(frames) >= 3 and max(frames) > 20
    assert all(bool((x >= 0).all()) for x in statics)  # linear energies
    return root, str(map_path), statics


@pytest.mark.parametrize("ring", [False, True], ids=["plain", "staging_ring"])
def test_files_are_pcen_of_the_plain_files(corpus, monkeypatch, ring):
    import torch

    root, map_path, statics = corpus
    out_dir = str(root / ("ring" if ring else "direct"))
    calls = []
    real = PCEN.apply_rows

    def counted(self, feats, row_offsets, *args, **kwargs):
        calls.append((tuple(feats.shape), [int(r) for r in row_offsets]))
        return real(self, feats, row_offsets, *args, **kwargs)

    monkeypatch.setattr(PCEN, "apply_rows", counted)
    args = [map_path, json.dumps(FBANK), out_dir, "--postprocess", POST] + (["--staging-ring"] if ring else [])
    rc = signals_to_torch_feat_dir(args)
    monkeypatch.undo()
    assert rc == 0
    frames = [x.shape[0] for x in statics]
    # the whole packed batch went through one call of the real batch, with the utterances' row offsets as they were
    # (the staging ring first sizes its buffers on a probe of 64 rows)
    batch = ((sum(frames), 41), np.concatenate([[0], np.cumsum(frames)]).tolist())
    assert [c for c in calls if c[0][0] != 64 or c == batch] == [batch]
    post = PCEN(smooth=0.025)
    for i, x in enumerate(statics):
        got = torch.load(os.path.join(out_dir, f"utt{i}.pt"), weights_only=True)
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(x.shape)  # row counts unchanged
        want = post.apply(x.numpy(), axis=0)
        assert got.numpy().tobytes() == want.tobytes(), i


def test_in_front_of_a_vad_with_select_last(corpus):
    import torch

    root, map_path, statics = corpus
    out_dir = str(root / "vad")
    # (the threshold is the utterance's mean of the normalised energy column: some frames lie above it, some below)
    vad = {"name": "vad", "energy_threshold": 0.0, "energy_mean_scale": 1.0, "select_last": True}
    spec = json.dumps([{"name": "pcen", "smooth": 0.025}, vad, {"name": "sliding_cmvn", "cmn_window": 6, "min_window": 1}])
    assert signals_to_torch_feat_dir([map_path, json.dumps(FBANK), out_dir, "--postprocess", spec]) == 0
    post, decide, sliding = PCEN(smooth=0.025), EnergyVAD(0.0, 1.0), SlidingCMVN(6, 1)
    kept = 0
    for i, x in enumerate(statics):
        got = torch.load(os.path.join(out_dir, f"utt{i}.pt"), weights_only=True).numpy()
        normed = post.apply(x.numpy(), axis=0)
        voiced = decide.decide(normed)  # decided on the rows as the PCEN left them ...
        want = sliding.apply(normed)[voiced]  # ... and dropped behind the last stage
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), i
        kept += int(voiced.sum())
    assert 0 < kept < sum(x.shape[0] for x in statics)


def test_a_config_that_takes_logs_is_refused(corpus):
    root, map_path, _ = corpus
    for cfg in (dict(FBANK, use_log=True), {k: v for k, v in FBANK.items() if k != "use_log"}):
        with pytest.raises(ValueError, match="PCEN takes linear energies"):
            signals_to_torch_feat_dir([map_path, json.dumps(cfg), str(root / "refused"), "--postprocess", POST])
