"""``post.PCEN`` without a device: argument errors, aliases and JSON configs; the third library's header against its
signature table, its exports and its argument errors; ``NativeError`` without the library or a device; the refusal of
a computer that takes logs, in ``StreamBatch``, ``SiStreamBatch`` and the command-line tool; and the stage's host half
(``_PcenStage.plan``) against a host model of the fresh flags over a scripted sequence of ticks and ``finalize``
calls."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from pydrobert_speech_amd import _native
from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg
from pydrobert_speech_amd.command_line import signals_to_torch_feat_dir
from pydrobert_speech_amd.compute import FrameComputer
from pydrobert_speech_amd.multistream import (PcenState, StreamBatch, _PcenStage, _tick_layout, _Upload,
                                              streaming_pcen)
from pydrobert_speech_amd.multistream_si import SiStreamBatch
from pydrobert_speech_amd.post import PCEN, PostProcessor
from tests.conftest import ROOT
from tests.test_multistream_host import golden_configs

LINEAR = dict(golden_configs()["c1_kaldi_fbank"], use_log=False)
LOGGED = dict(golden_configs()["c1_kaldi_fbank"], use_log=True)
SI_LINEAR = {"name": "si", "bank": {"name": "fbank", "num_filts": 40}, "use_log": False}
SI_LOGGED = {"name": "si", "bank": {"name": "fbank", "num_filts": 40}}


def build(cfg):
    return alias_factory_subclass_from_arg(FrameComputer, json.loads(json.dumps(cfg)))


# ---- 1. arguments, aliases, configs ---------------------------------------------------------------------------------


def test_defaults_and_what_the_kernels_are_given():
    post = PCEN()
    assert (post.smooth_coeff, post.gain, post.bias, post.power, post.eps) == (0.025, 0.98, 2.0, 0.5, 1e-6)
    assert post.oms == float(np.float64(1.0) - np.float64(0.025)) == 0.975
    assert post.bp == float(np.float64(2.0) ** np.float64(0.5))
    edge = PCEN(smooth=1, gain=0, bias=0, power=2, eps=1e-30)
    assert (edge.smooth_coeff, edge.oms, edge.gain, edge.bias, edge.bp) == (1.0, 0.0, 0.0, 0.0, 0.0)
    assert isinstance(edge.smooth_coeff, float) and isinstance(PCEN(smooth=np.float32(0.5)).smooth_coeff, float)


@pytest.mark.parametrize("kwargs", [
    {"smooth": 0.0}, {"smooth": -0.1}, {"smooth": 1.0000001}, {"gain": -1e-9}, {"bias": -1.0}, {"power": 0.0},
    {"power": -0.5}, {"eps": 0.0}, {"eps": -1e-6},
    {"smooth": float("nan")}, {"gain": float("inf")}, {"bias": float("nan")}, {"power": float("inf")},
    {"eps": float("nan")}, {"eps": float("inf")}, {"smooth": -float("inf")},
    {"smooth": "0.5"}, {"gain": None}, {"bias": True}, {"power": [0.5]},
])
def test_bad_arguments_are_value_errors(kwargs):
    with pytest.raises(ValueError, match="PCEN"):
        PCEN(**kwargs)


def test_aliases_and_json_configs():
    assert PCEN.aliases == {"pcen", "per_channel_energy_norm"}
    # neither alias belongs to another post-processor: the registry finds PCEN, and only PCEN carries them
    def carriers(klass, alias):
        return [k for k in [klass, *klass.__subclasses__()] if alias in k.__dict__.get("aliases", ())] + [
            c for sub in klass.__subclasses__() for c in carriers(sub, alias) if c is not sub]
    for alias in PCEN.aliases:
        assert set(carriers(PostProcessor, alias)) == {PCEN}
        assert type(alias_factory_subclass_from_arg(PostProcessor, alias)) is PCEN
    post = alias_factory_subclass_from_arg(PostProcessor, json.loads('{"name": "pcen", "smooth": 0.05, "bias": 10}'))
    assert type(post) is PCEN and (post.smooth_coeff, post.bias, post.gain) == (0.05, 10.0, 0.98)
    post = alias_factory_subclass_from_arg(PostProcessor, {"alias": "per_channel_energy_norm", "power": 0.25})
    assert type(post) is PCEN and post.power == 0.25
    with pytest.raises(ValueError):
        alias_factory_subclass_from_arg(PostProcessor, {"name": "pcen", "smooth": 2})
    with pytest.raises(TypeError):
        alias_factory_subclass_from_arg(PostProcessor, {"name": "pcen", "time_constant": 0.4})
    assert streaming_pcen(None) is None and streaming_pcen("pcen").smooth_coeff == 0.025
    assert streaming_pcen({"name": "pcen", "smooth": 0.5}).oms == 0.5
    with pytest.raises(ValueError, match="post.PCEN"):
        streaming_pcen({"name": "deltas", "num_deltas": 2})
    with pytest.raises(ValueError, match="no post-processor"):
        streaming_pcen(3)


# ---- 2. the third library's binding ---------------------------------------------------------------------------------


def test_stages2_header_and_signature_table_name_the_same_set():
    with open(os.path.join(ROOT, "include", "pds_amd_stages2.h")) as fh:
        header = fh.read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)  # (the comments name functions of the rule header)
    declared = dict(re.findall(r"\b(pds_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code))
    assert set(declared) == set(_native.STAGES2_SIGNATURES), set(declared) ^ set(_native.STAGES2_SIGNATURES)
    assert {"pds_stages2_version", "pds_stages2_last_error"} <= set(declared)
    for name, args in declared.items():
        restype, argtypes = _native.STAGES2_SIGNATURES[name]
        count = 0 if args.strip() == "void" else len(args.split(","))
        assert count == len(argtypes), name
        if name != "pds_stages2_last_error":
            assert restype is ctypes.c_int32, name
    assert len(_native.STAGES2_SIGNATURES["pds_pcen_smooth_rows_f32"][1]) == 11
    assert len(_native.STAGES2_SIGNATURES["pds_pcen_compress_rows_f64"][1]) == 14
    assert len(_native.STAGES2_SIGNATURES["pds_multistream_pcen_f32"][1]) == 16
    # it shares no header with the other libraries
    for other in ("pds_amd.h", "pds_amd_stages.h", "pds_internal.h", "stages_internal.h"):
        assert f'"{other}"' not in header and f"/{other}" not in code
    with open(os.path.join(ROOT, "pydrobert-speech_amd", "csrc", "pcen.hip")) as fh:
        includes = re.findall(r'#include\s+"([^"]+)"', fh.read())
    assert includes == ["../../include/pds_amd_stages2.h", "pcen_rule.h"]


def test_the_definition_is_in_the_header_and_the_docstring_word_for_word():
    with open(os.path.join(ROOT, "include", "pds_amd_stages2.h")) as fh:
        header = " ".join(re.sub(r"^\s*\*\s?", "", line) for line in fh.read().splitlines()).split()
    header = " ".join(header)
    doc = " ".join(PCEN.__doc__.split())
    start, end = "Per utterance of T >= 1 rows", "T = 0 gives nothing."
    text = doc[doc.index(start): doc.index(end) + len(end)]
    assert len(text) > 900 and text in header


def test_stages2_library_exports_every_declared_symbol():
    lib = _native.stages2_lib()  # (NativeError if it was not built: there is no fallback)
    for name in _native.STAGES2_SIGNATURES:
        assert getattr(lib, name) is not None
    assert lib.pds_stages2_version() >= 100
    assert isinstance(lib.pds_stages2_last_error(), bytes)
    # argument errors are reported before any HIP call, through the library's own error string
    assert lib.pds_pcen_smooth_rows_f32(None, 4, None, None, 2, 4, 0.025, 0.975, None, 4, None) == -1
    assert b"null pointer" in lib.pds_stages2_last_error()
    assert lib.pds_pcen_smooth_rows_f64(None, 3, None, None, 2, 4, 0.025, 0.975, None, 4, None) == -1
    assert b"stride" in lib.pds_stages2_last_error()
    assert lib.pds_pcen_smooth_rows_f64(None, 4, None, None, 2, 4, 0.0, 1.0, None, 4, None) == -1
    assert b"smooth" in lib.pds_stages2_last_error()
    assert lib.pds_pcen_smooth_rows_f64(None, 4, None, None, 2, 0, 0.5, 0.5, None, 4, None) == -1
    assert lib.pds_pcen_smooth_rows_f64(None, 4, None, None, 0, 4, 0.5, 0.5, None, 4, None) == 0
    big = (1 << 31) - 1
    assert lib.pds_pcen_smooth_rows_f32(None, big, None, None, big, big, 0.5, 0.5, None, big, None) == -1
    assert b"too many lanes" in lib.pds_stages2_last_error()
    assert lib.pds_pcen_compress_rows_f32(None, 4, None, 4, 0, 4, 0.98, 2.0, 0.5, 1e-6, 1.4, None, 4, None) == 0
    assert lib.pds_pcen_compress_rows_f32(None, 4, None, 4, 5, 4, 0.98, 2.0, 0.5, 1e-6, 1.4, None, 4, None) == -1
    assert b"null pointer" in lib.pds_stages2_last_error()
    assert lib.pds_pcen_compress_rows_f64(None, 4, None, 3, 5, 4, 0.98, 2.0, 0.5, 1e-6, 1.4, None, 4, None) == -1
    assert b"stride" in lib.pds_stages2_last_error()
    assert lib.pds_pcen_compress_rows_f64(None, 4, None, 4, 1 << 62, 4, 0.98, 2.0, 0.5, 1e-6, 1.4, None, 4, None) == -1
    assert b"too many" in lib.pds_stages2_last_error()
    ms = (0.025, 0.975, 0.98, 2.0, 0.5, 1e-6, 1.4)
    assert lib.pds_multistream_pcen_f32(None, None, 4, 3, *ms, None, None, None, 0, None) == 0
    assert lib.pds_multistream_pcen_f32(None, None, 4, 3, *ms, None, None, None, 2, None) == -1
    assert b"null pointer" in lib.pds_stages2_last_error()
    assert lib.pds_multistream_pcen_f64(None, None, 4, 0, *ms, None, None, None, 2, None) == -1
    with pytest.raises(ValueError, match="multistream_pcen"):
        _native.check_stages2(-1, "pds_multistream_pcen")
    with pytest.raises(_native.NativeError, match="code -2"):
        _native.check_stages2(-2, "pds_multistream_pcen")


def test_no_cpu_path_without_a_device(monkeypatch):
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    post = PCEN()
    x = np.ones((10, 3), dtype=np.float32)
    for call in (lambda: post.apply(x, axis=0), lambda: post.smooth(x, axis=0),
                 lambda: post.apply_rows(torch.ones(4, 3), [0, 4]), lambda: post.smooth_rows(torch.ones(4, 3), [0, 4])):
        with pytest.raises(_native.NativeError, match="no HIP device"):
            call()
    with pytest.raises(_native.NativeError, match="no HIP device"):
        StreamBatch(build(LINEAR), capacity=4, pcen=post)


# ---- 3. a computer that takes logs is refused -----------------------------------------------------------------------


def test_stream_batches_refuse_a_computer_that_takes_logs(monkeypatch):
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # (the refusal comes before any device is asked for)
    for cls, logged, linear in ((StreamBatch, LOGGED, LINEAR), (SiStreamBatch, SI_LOGGED, SI_LINEAR)):
        for pcen in (PCEN(), "pcen", {"name": "pcen", "smooth": 0.1}):
            with pytest.raises(ValueError, match="PCEN takes linear energies"):
                cls(build(logged), capacity=4, pcen=pcen)
        with pytest.raises(_native.NativeError, match="no HIP device"):  # (accepted: the device comes next)
            cls(build(linear), capacity=4, pcen=PCEN())
        with pytest.raises(_native.NativeError, match="no HIP device"):  # (and without the stage logs are as fine as ever)
            cls(build(logged), capacity=4)
    with pytest.raises(ValueError, match="PCEN takes linear energies"):
        streaming_pcen("pcen", build(LOGGED))
    assert streaming_pcen("pcen", build(LINEAR)).smooth_coeff == 0.025


def test_the_command_line_tool_refuses_a_computer_that_takes_logs(tmp_path):
    map_path = tmp_path / "map.txt"
    map_path.write_text(f"utt0 {tmp_path / 'missing.npy'}\n")
    for cfg in (LOGGED, SI_LOGGED):
        for spec in ('[{"name": "pcen", "smooth": 0.025}]', '[{"name": "deltas", "num_deltas": 2}, "pcen"]'):
            with pytest.raises(ValueError, match="PCEN takes linear energies"):
                signals_to_torch_feat_dir([str(map_path), json.dumps(cfg), str(tmp_path / "out"), "--postprocess", spec])


# ---- 4. the stage's host half ---------------------------------------------------------------------------------------


class _FakeTorch:
    float32, float64 = "f4", "f8"

    class cuda:
        @staticmethod
        def current_device():
            return 0

    @staticmethod
    def device(*args):
        return args

    @staticmethod
    def zeros(shape, dtype=None, device=None):
        return ("zeros", tuple(shape), dtype)

    @staticmethod
    def empty(shape, dtype=None, device=None):
        return ("empty", tuple(shape), dtype)


class _FakeLib:
    pds_multistream_assemble_f32 = pds_multistream_assemble_f64 = None

    @staticmethod
    def pds_multistream_tile():
        return 1024


class _FakeStages2Lib:
    pds_multistream_pcen_f32, pds_multistream_pcen_f64 = "pcen_f32", "pcen_f64"


def fake_batch(monkeypatch, stages2=_FakeStages2Lib, **kwargs):
    from pydrobert_speech_amd import multistream

    class Native:
        require_device = staticmethod(lambda: _FakeTorch)
        lib = staticmethod(lambda: _FakeLib)
        stages2_lib = staticmethod(lambda: stages2)

    monkeypatch.setattr(multistream, "_native", Native)
    comp = build(LINEAR)
    monkeypatch.setattr(type(comp), "_native_plan", lambda self, device=None: None)
    return comp, StreamBatch(comp, capacity=8, **kwargs)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_stage_is_first_keeps_the_widths_and_owns_one_pool(monkeypatch, dtype):
    from pydrobert_speech_amd.post import Cepstra, Deltas, Stack, Standardize

    comp, sb = fake_batch(monkeypatch, dtype=dtype, pcen=PCEN())
    assert list(sb._stages) == ["pcen"] and isinstance(sb._stages["pcen"], _PcenStage)
    stage = sb._stages["pcen"]
    assert (sb._F0, sb._F, sb.num_coeffs, sb.lookahead, sb.num_vectors) == (40, 40, 40, 0, 1)
    assert stage.pools == {"smooth": ("empty", (8, 40), "f8")}  # float64 [capacity, C], whatever the row type
    assert stage._fn == ("pcen_f32" if dtype == np.float32 else "pcen_f64")
    assert isinstance(sb.estate, PcenState) and sb.estate is stage.state and sb.estate.fresh.all()
    assert sb._layout_flags == (False, False, False, False, False, True)
    sb.close()
    assert stage.pools == {}
    # a batch without the stage is as it was: no state, no flag, no symbol asked of the third library
    _, plain = fake_batch(monkeypatch, stages2=None, dtype=dtype)
    assert plain.estate is None and "pcen" not in plain._stages and len(plain._layout_flags) == 5
    with pytest.raises(ValueError, match="without pcen"):
        plain.pcen_smooth([0])
    with pytest.raises(AttributeError):
        fake_batch(monkeypatch, stages2=object, dtype=dtype, pcen=PCEN())  # (a stale library is an error, no fall-back)


def test_the_layout_gains_three_sections_behind_all_others():
    for n in (0, 1, 7, 8, 9, 300):
        for E in (0, n):
            for chunks in (False, True):
                for deltas, cmvn, stack, dither, sliding in ((False,) * 5, (True, True, True, True, False),
                                                             (True, False, False, True, True)):
                    old = _tick_layout(n, E, 4, chunks, deltas, cmvn, stack, dither, sliding)
                    assert _tick_layout(n, E, 4, chunks, deltas, cmvn, stack, dither, sliding, False) == old
                    at, words = _tick_layout(n, E, 4, chunks, deltas, cmvn, stack, dither, sliding, True)
                    at = dict(at)  # (the layouts are cached: the copy is taken apart)
                    fresh_words = (n + 7) // 8  # one byte per stream
                    assert words == old[1] + n + (n + 1) + fresh_words
                    assert at.pop("pcen_ids") == (old[1], n, (n,), (1,))
                    assert at.pop("pcen_rows") == (old[1] + n, n + 1, (n + 1,), (1,))
                    assert at.pop("pcen_fresh") == (old[1] + 2 * n + 1, fresh_words, (fresh_words,), (1,))
                    assert at == old[0]


def test_plan_fills_the_sections_as_a_host_model_of_the_fresh_flags_says(monkeypatch):
    """a scripted sequence of ticks and ``finalize`` calls: a stream is fresh until a tick brings it a row and again
    after its ``finalize``; a tick that brings it no row leaves it as it was; ``plan`` changes no state"""
    _, sb = fake_batch(monkeypatch, pcen=PCEN())
    stage = sb._stages["pcen"]
    live = {}  # the model: stream -> has had a row since its start or last finalize
    script = [
        # (final, ids, rows per stream)
        (False, [3, 0, 7], [0, 2, 1]),
        (False, [3, 0, 7], [0, 1, 0]),
        (False, [7, 3], [4, 1]),
        (True, [0], [1]),  # a finalize that brings a last row
        (False, [0, 5, 3], [1, 0, 2]),  # 0 starts anew
        (True, [5, 7], [0, 2]),  # 5 never had a row
        (False, [5, 7, 1, 2, 4, 6, 0, 3], [1, 1, 0, 3, 0, 0, 0, 1]),  # every stream, one of the bytes' words full
        (True, [5, 7, 1, 2, 4, 6, 0, 3], [0] * 8),
        (False, [2], [0]),
        (False, [2], [5]),
    ]
    rng = np.random.default_rng(0)
    for final, ids, k in script:
        ids, k = np.asarray(ids, dtype=np.int64), np.asarray(k, dtype=np.int64)
        n = len(ids)
        rows = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
        up = _Upload(3, _tick_layout(n, int((k > 0).sum()), 4, not final, *sb._layout_flags))
        up.pinned = rng.integers(-(1 << 62), 1 << 62, up.words + 5, dtype=np.int64)  # (garbage: every word is written)
        guard = up.pinned.copy()
        before = stage.state.live.copy()
        out_rows = stage.plan(up, ids, rows, final)
        assert out_rows is rows and (stage.state.live == before).all()  # the rows pass; plan commits nothing
        assert up.host("pcen_ids").tolist() == ids.tolist()
        assert up.host("pcen_rows").tolist() == rows.tolist()
        fresh = up.host("pcen_fresh").view(np.uint8)
        want = [0 if live.get(int(i), False) else 1 for i in ids]
        assert fresh[:n].tolist() == want and not fresh[n:].any()
        # nothing outside the stage's sections was written
        lo = up.sample_words + up.at["pcen_ids"][0]
        assert (up.pinned[:lo] == guard[:lo]).all() and (up.pinned[up.words:] == guard[up.words:]).all()
        stage.state.commit(ids, stage._step)  # (what `launch` does after its kernel)
        for i, rows_i in zip(ids.tolist(), k.tolist()):
            live[i] = False if final else (live.get(i, False) or rows_i > 0)
        assert stage.state.live.tolist() == [live.get(i, False) for i in range(8)]
        assert (stage.state.fresh == ~stage.state.live).all()
    assert stage.state.live.tolist() == [False, False, True, False, False, False, False, False]
    stage.state.reset(np.asarray([2]))
    assert stage.state.fresh.all()
    with pytest.raises(ValueError):
        PcenState(0)
