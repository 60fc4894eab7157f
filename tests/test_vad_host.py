"""The host side of the energy VAD (CPU only): the ``EnergyVAD`` arguments and aliases, the ``ValueError`` s of ``apply``
and of the command-line chain (exercised with stubs in the place of the device calls), and the stages library's header
and exports."""
import ctypes
import os
import re

import numpy as np
import pytest

from pydrobert_speech_amd import _native
from pydrobert_speech_amd import post as post_module
from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg
from pydrobert_speech_amd.command_line import FeatureDirWriter
from pydrobert_speech_amd.post import EnergyVAD, PostProcessor, SlidingCMVN
from tests.conftest import ROOT
from tests.vad_model import select_rows, vad_decide_rows

# ---- 1. the post-processor's arguments ----------------------------------------------------------------------------


def settings(v):
    return (v.energy_threshold, v.energy_mean_scale, v.frames_context, v.proportion_threshold, v.energy_col, v.select_last)


def test_aliases_and_json_construction():
    assert "EnergyVAD" in post_module.__all__
    for alias in ("vad", "energy_vad", "vad_energy"):
        inst = alias_factory_subclass_from_arg(PostProcessor, alias)
        assert type(inst) is EnergyVAD and settings(inst) == (5.0, 0.5, 0, 0.6, 0, False)  # Kaldi's defaults
    inst = alias_factory_subclass_from_arg(
        PostProcessor, {"name": "vad", "energy_threshold": 5.5, "energy_mean_scale": 0, "frames_context": 2,
                        "proportion_threshold": 0.12, "energy_col": 3, "select_last": True})
    assert settings(inst) == (5.5, 0.0, 2, 0.12, 3, True)
    inst = alias_factory_subclass_from_arg(PostProcessor, {"alias": "energy_vad", "frames_context": np.int64(5)})
    assert settings(inst) == (5.0, 0.5, 5, 0.6, 0, False)
    assert EnergyVAD(np.float32(-3), np.int32(2)).energy_mean_scale == 2.0
    # the sliding normalisation keeps its aliases
    assert type(alias_factory_subclass_from_arg(PostProcessor, "sliding")) is SlidingCMVN


@pytest.mark.parametrize("kwargs", [
    dict(energy_mean_scale=-0.5), dict(energy_mean_scale=float("nan")), dict(energy_mean_scale="0.5"),
    dict(energy_mean_scale=True), dict(energy_threshold=None), dict(energy_threshold=float("inf")),
    dict(energy_threshold="5"), dict(frames_context=-1), dict(frames_context=1.0), dict(frames_context=True),
    dict(frames_context=1 << 31), dict(proportion_threshold=0), dict(proportion_threshold=0.0),
    dict(proportion_threshold=1), dict(proportion_threshold=1.0), dict(proportion_threshold=-0.2),
    dict(proportion_threshold=1.5), dict(proportion_threshold=float("nan")), dict(proportion_threshold=None),
    dict(energy_col=-1), dict(energy_col=0.0), dict(energy_col=False), dict(select_last=1), dict(select_last="yes")])
def test_arguments_are_validated_in_the_constructor(kwargs):
    with pytest.raises(ValueError):
        EnergyVAD(**kwargs)


def test_the_edges_of_the_ranges_are_accepted():
    assert EnergyVAD(energy_mean_scale=0).energy_mean_scale == 0.0
    assert EnergyVAD(frames_context=0, energy_col=0, energy_threshold=-40).energy_threshold == -40.0
    assert EnergyVAD(proportion_threshold=np.nextafter(0.0, 1.0)).proportion_threshold > 0.0
    assert EnergyVAD(proportion_threshold=np.nextafter(1.0, 0.0)).proportion_threshold < 1.0


# ---- 2. what apply refuses (before anything touches a device) -----------------------------------------------------


def test_apply_refuses_batches_and_in_place():
    vad = EnergyVAD()
    with pytest.raises(ValueError, match="ragged"):
        vad.apply(np.zeros((2, 5, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="ragged"):
        vad.apply(np.zeros(5, dtype=np.float32))
    with pytest.raises(ValueError, match="in_place"):
        vad.apply(np.zeros((5, 3), dtype=np.float32), in_place=True)
    with pytest.raises(ValueError, match="in_place"):
        vad.apply(np.zeros((2, 5, 3), dtype=np.float32), in_place=True)


# ---- 3. the command-line chain, with the model in the place of the device calls -----------------------------------


class Double(PostProcessor):
    """keeps the rows"""

    aliases = set()

    def apply(self, features, axis=-1, in_place=False):
        return features * 2


class DropFirst(PostProcessor):
    """one row fewer per utterance (of those that have one)"""

    aliases = set()

    def apply(self, features, axis=-1, in_place=False):
        return features[1:]


@pytest.fixture
def stubbed(monkeypatch):
    """EnergyVAD's device calls replaced by the numpy model on CPU tensors; records the calls"""
    import torch

    calls = []

    def kwargs(self):
        return dict(energy_threshold=self.energy_threshold, energy_mean_scale=self.energy_mean_scale,
                    frames_context=self.frames_context, proportion_threshold=self.proportion_threshold)

    def decide_rows(self, feats, row_offsets):
        calls.append(("decide", tuple(feats.shape)))
        voiced, counts = vad_decide_rows(feats.numpy(), row_offsets, self.energy_col, **kwargs(self))
        return torch.from_numpy(voiced), counts

    def select_rows_(self, feats, row_offsets, voiced):
        calls.append(("select", tuple(feats.shape)))
        out, offs = select_rows(feats.numpy(), row_offsets, voiced.numpy())
        return torch.from_numpy(out), offs

    def apply_rows(self, feats, row_offsets):
        voiced, _ = decide_rows(self, feats, row_offsets)
        return select_rows_(self, feats, row_offsets, voiced)

    monkeypatch.setattr(EnergyVAD, "decide_rows", decide_rows)
    monkeypatch.setattr(EnergyVAD, "select_rows", select_rows_)
    monkeypatch.setattr(EnergyVAD, "apply_rows", apply_rows)
    return calls


def batch():
    import torch

    feats = np.arange(40, dtype=np.float32).reshape(10, 4)
    feats[:, 0] = [9, 0, 9, 9, 0, 0, 0, 9, 0, 9]
    return torch.from_numpy(feats), np.asarray([0, 4, 7, 10], dtype=np.int64), feats


def writer(tmp_path, posts):
    return FeatureDirWriter(None, [], posts, str(tmp_path))


def test_select_last_decides_where_it_stands_and_drops_after_the_last_stage(tmp_path, stubbed):
    feats, rows, host = batch()
    vad = EnergyVAD(5.0, 0.0, select_last=True)
    # behind Double the energies are 18 and 0 (decided there); the second Double sees all ten rows
    out, offs = writer(tmp_path, [Double(), vad, Double()])._postprocess(feats, rows)
    assert stubbed == [("decide", (10, 4)), ("select", (10, 4))]
    keep = host[:, 0] > 2.5
    assert offs.tolist() == [0, 3, 3, 5] and (out.numpy() == 4 * host[keep]).all()
    # ... and without select_last the rows are dropped where the stage stands
    del stubbed[:]
    out2, offs2 = writer(tmp_path, [Double(), EnergyVAD(5.0, 0.0), Double()])._postprocess(feats, rows)
    assert stubbed == [("decide", (10, 4)), ("select", (10, 4))]
    assert offs2.tolist() == offs.tolist() and (out2.numpy() == out.numpy()).all()
    # the last stage of the chain: selected at once
    out3, offs3 = writer(tmp_path, [vad])._postprocess(feats, rows)
    assert offs3.tolist() == [0, 3, 3, 5] and (out3.numpy() == host[keep]).all()
    # a later stage that packs the utterances anew (same counts, other offsets): the mask moves with them
    import torch

    gapped = torch.cat([torch.full((1, 4), 99.0), feats, torch.full((2, 4), 99.0)])  # rows of no utterance around
    out4, offs4 = writer(tmp_path, [vad, Double()])._postprocess(gapped, np.asarray([1, 5, 8, 11], dtype=np.int64))
    assert offs4.tolist() == [0, 3, 3, 5] and (out4.numpy() == 2 * host[keep]).all()


def test_a_stage_that_changes_row_counts_behind_a_pending_selection_is_refused(tmp_path, stubbed):
    feats, rows, _ = batch()
    with pytest.raises(ValueError, match="DropFirst.*EnergyVAD|EnergyVAD.*DropFirst"):
        writer(tmp_path, [EnergyVAD(5.0, 0.0, select_last=True), DropFirst()])._postprocess(feats, rows)
    # (a second VAD that drops rows where it stands changes them too)
    with pytest.raises(ValueError, match="row counts"):
        writer(tmp_path, [EnergyVAD(5.0, 0.0, select_last=True), EnergyVAD(5.0, 0.0)])._postprocess(feats, rows)
    # in front of the selection it is fine
    out, offs = writer(tmp_path, [DropFirst(), EnergyVAD(5.0, 0.0, select_last=True), Double()])._postprocess(feats, rows)
    assert offs.tolist() == [0, 2, 2, 3]


def test_two_pending_selections_are_refused(tmp_path, stubbed):
    feats, rows, _ = batch()
    chain = [EnergyVAD(5.0, 0.0, select_last=True), Double(), EnergyVAD(2.0, 0.0, select_last=True)]
    with pytest.raises(ValueError, match="two EnergyVAD"):
        writer(tmp_path, chain)._postprocess(feats, rows)
    assert stubbed == [("decide", (10, 4))]  # (refused before the second decides)


def test_the_probe_keeps_every_row(tmp_path, stubbed):
    """what sizes the staging ring's buffers: a selection can only shrink the result, down to 0 rows"""
    feats, rows, host = batch()
    for last in (False, True):
        out, offs = writer(tmp_path, [EnergyVAD(1e9, 0.0, select_last=last), Double()])._postprocess(feats, rows, probe=True)
        assert offs.tolist() == rows.tolist() and (out.numpy() == 2 * host).all()
        out, offs = writer(tmp_path, [EnergyVAD(1e9, 0.0, select_last=last), Double()])._postprocess(feats, rows)
        assert offs.tolist() == [0, 0, 0, 0] and tuple(out.shape) == (0, 4)
    assert ("decide", (10, 4)) in stubbed


# ---- 4. the stages library's binding ------------------------------------------------------------------------------


def test_the_header_declares_the_new_entry_points():
    with open(os.path.join(ROOT, "include", "pds_amd_stages.h")) as fh:
        header = fh.read()
    declared = set(re.findall(r"\b(pds_[a-z0-9_]+)\s*\(", header))
    new = {"pds_vad_energy_rows_f32", "pds_vad_energy_rows_f64", "pds_select_rows_w32"}
    assert new <= declared and declared == set(_native.STAGES_SIGNATURES)
    for name in ("pds_vad_energy_rows_f32", "pds_vad_energy_rows_f64"):
        restype, argtypes = _native.STAGES_SIGNATURES[name]
        assert restype is ctypes.c_int32 and len(argtypes) == 13
        assert argtypes[6:10] == [ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_double]
    restype, argtypes = _native.STAGES_SIGNATURES["pds_select_rows_w32"]
    assert restype is ctypes.c_int32 and len(argtypes) == 12
    assert "uint8_t *d_voiced, int64_t *d_count, void *stream);" in header
    assert "int32_t pds_select_rows_w32(const void *d_in, int64_t in_stride, int32_t words," in header
    assert not new & set(_native.SIGNATURES)


def test_the_library_exports_them_and_checks_arguments_before_any_hip_call():
    lib = _native.stages_lib()  # (NativeError if it was not built: there is no fallback)
    assert lib.pds_stages_version() >= 101
    err = lib.pds_stages_last_error
    vad32, vad64, sel = lib.pds_vad_energy_rows_f32, lib.pds_vad_energy_rows_f64, lib.pds_select_rows_w32
    # B == 0 or max_rows == 0: nothing to do, no pointer is looked at
    assert vad32(None, 1, None, None, 0, 5, 5.0, 0.5, 0, 0.6, None, None, None) == 0
    assert vad64(None, 1, None, None, 3, 0, 5.0, 0.5, 0, 0.6, None, None, None) == 0
    assert sel(None, 4, 4, None, None, 0, 9, None, None, None, 4, None) == 0
    assert sel(None, 4, 4, None, None, 3, 0, None, None, None, 4, None) == 0
    # null pointers
    assert vad32(None, 1, None, None, 2, 5, 5.0, 0.5, 0, 0.6, None, None, None) == -1 and b"null pointer" in err()
    assert sel(None, 4, 4, None, None, 2, 5, None, None, None, 4, None) == -1 and b"null pointer" in err()
    # sizes and parameters
    assert vad32(None, 1, None, None, -1, 5, 5.0, 0.5, 0, 0.6, None, None, None) == -1 and b"bad size" in err()
    assert vad64(None, 1, None, None, 2, -5, 5.0, 0.5, 0, 0.6, None, None, None) == -1 and b"bad size" in err()
    assert vad64(None, 0, None, None, 2, 5, 5.0, 0.5, 0, 0.6, None, None, None) == -1 and b"stride" in err()
    assert vad32(None, 1, None, None, 2, 5, 5.0, -0.5, 0, 0.6, None, None, None) == -1 and b"negative" in err()
    assert vad32(None, 1, None, None, 2, 5, 5.0, float("nan"), 0, 0.6, None, None, None) == -1
    assert vad32(None, 1, None, None, 2, 5, 5.0, 0.5, -1, 0.6, None, None, None) == -1 and b"negative" in err()
    for p in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert vad64(None, 1, None, None, 2, 5, 5.0, 0.5, 0, p, None, None, None) == -1 and b"between 0 and 1" in err()
    assert sel(None, 4, 0, None, None, 2, 5, None, None, None, 4, None) == -1 and b"bad size" in err()
    assert sel(None, 3, 4, None, None, 2, 5, None, None, None, 4, None) == -1 and b"stride" in err()
    assert sel(None, 4, 4, None, None, 2, 5, None, None, None, 3, None) == -1 and b"stride" in err()
    # more blocks than a grid has: 2^31 - 1 utterances of one tile each fit, of two tiles do not
    big = (1 << 31) - 1
    assert sel(None, 4, 4, None, None, big, 256, None, None, None, 4, None) == -1 and b"null pointer" in err()
    assert sel(None, 4, 4, None, None, big, 257, None, None, None, 4, None) == -1 and b"split the batch" in err()
    assert sel(None, 4, 4, None, None, 2, 1 << 40, None, None, None, 4, None) == -1 and b"split the batch" in err()
    with pytest.raises(ValueError, match="pds_select_rows"):
        _native.check_stages(-1, "pds_select_rows")
