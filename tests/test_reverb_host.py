"""pre.Reverb without a device: the sixth stages library's header against the signature table, argument errors before
any HIP call, the counting calls against the Python layout, the aliases, the refusals of the constructor, the plan API,
the ``TypeError`` of a ``StreamBatch``, the definition word for word in its three places, and the command-line stage."""
import ctypes
import os
import re

import numpy as np
import pytest

import pydrobert_speech_amd as ps
from pydrobert_speech_amd import _native
from pydrobert_speech_amd import pre as pre_module
from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg
from pydrobert_speech_amd.pre import PreProcessor, Reverb, ReverbPlan
from tests import reverb_model as rm
from tests.conftest import ROOT


def _rirs():
    return [rm.response(300, 10), rm.response(1025, 600, dtype=np.float32), rm.response(40, 39, dtype=np.int16)]


def _definition(text):
    text = " ".join(text.split())
    start, end = "Bank: - `K` room impulse responses", "It never spoils another utterance."
    return text[text.index(start): text.index(end) + len(end)]


def test_the_definition_is_in_the_docstring_the_header_and_the_design_word_for_word():
    doc = _definition(Reverb.__doc__)
    assert len(doc) > 2500
    with open(os.path.join(ROOT, "include", "pds_amd_stages6.h")) as fh:
        header = "\n".join(re.sub(r"^\s*\*\s?", "", line) for line in fh.read().splitlines())
    assert _definition(header) == doc
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        design = fh.read()
    assert "4.13" in design and _definition(design[design.index("### 4.13"):]) == doc


def test_stages6_header_and_signature_table_name_the_same_set():
    with open(os.path.join(ROOT, "include", "pds_amd_stages6.h")) as fh:
        header = fh.read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = dict(re.findall(r"\b(pds_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code))
    assert set(declared) == set(_native.STAGES6_SIGNATURES), set(declared) ^ set(_native.STAGES6_SIGNATURES)
    assert {"pds_stages6_version", "pds_stages6_last_error", "pds_reverb_spectra_f32", "pds_reverb_spectra_f64",
            "pds_reverb_spectra_i16", "pds_reverb_convolve", "pds_reverb_scale",
            "pds_reverb_workspace_bytes"} <= set(declared)
    for name, args in declared.items():
        restype, argtypes = _native.STAGES6_SIGNATURES[name]
        count = 0 if args.strip() == "void" else len(args.split(","))
        assert count == len(argtypes), name
    assert _native.STAGES6_SIGNATURES["pds_reverb_workspace_bytes"][0] is ctypes.c_int64
    for other in ("pds_amd.h", "pds_amd_stages.h", "pds_amd_stages2.h", "pds_amd_stages3.h", "pds_amd_stages4.h",
                  "pds_amd_stages5.h", "pds_internal.h", "stages_internal.h"):
        assert f'"{other}"' not in header and f"/{other}" not in code


def test_reverb_hip_includes_its_header_the_rule_and_the_transform_templates_only():
    csrc = os.path.join(ROOT, "pydrobert-speech_amd", "csrc")
    with open(os.path.join(csrc, "reverb.hip")) as fh:
        includes = re.findall(r'#include\s+"([^"]+)"', fh.read())
    assert includes == ["../../include/pds_amd_stages6.h", "fft_inlane.h", "reverb_rule.h"]
    users = []
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")) and name != "reverb_rule.h":
            with open(os.path.join(csrc, name)) as fh:
                if "reverb_rule.h" in re.findall(r'#include\s+"([^"]+)"', fh.read()):
                    users.append(name)
    assert users == ["reverb.hip"]
    with open(os.path.join(csrc, "reverb_rule.h")) as fh:
        assert re.findall(r'#include\s+"([^"]+)"', fh.read()) == []
    with open(os.path.join(csrc, "Makefile")) as fh:
        make = fh.read()
    assert "STAGES6_LIB  = libpds_amd_stages6.so" in make and "STAGES6_OBJS = reverb.o" in make
    assert re.search(r"^all:.*\$\(STAGES6_LIB\)", make, flags=re.M)
    assert re.search(r"^clean:\n\trm.*\$\(STAGES6_LIB\)", make, flags=re.M)
    assert "STAGES5_OBJS = mix.o\n" in make  # the sixth library keeps the noise-mixing kernels and no other
    assert not re.search(r"^SRCS = .*reverb", make, flags=re.M)  # nothing of it went into the first library
    with open(os.path.join(csrc, "reverb.hip")) as fh:
        assert not re.search(r"atomic[A-Z]|atomic_|__hip_atomic", fh.read())


def test_stages6_library_exports_every_declared_symbol_and_reports_argument_errors():
    lib = _native.stages6_lib()  # (NativeError if it was not built: there is no fallback)
    for name in _native.STAGES6_SIGNATURES:
        assert getattr(lib, name) is not None
    assert lib.pds_stages6_version() >= 100
    assert isinstance(lib.pds_stages6_last_error(), bytes)
    assert lib.pds_reverb_block_samples() == 512 == pre_module._REVERB_BLOCK
    assert lib.pds_reverb_max_taps() == 1 << 20 == pre_module._REVERB_MAX_TAPS
    assert [lib.pds_reverb_partitions(L) for L in (1, 512, 513, 1 << 20)] == [1, 1, 2, 2048]
    for L in (-1, 0, (1 << 20) + 1):  # L = 0 and L > 2^20 are refused, with a message
        assert lib.pds_reverb_partitions(L) == -1 and b"1 to 2^20 taps" in lib.pds_stages6_last_error()
    assert [lib.pds_reverb_spectra_units(n) for n in (-1, 0, 1, 512, 513, 1024, 1025)] == [0, 0, 4, 4, 4, 4, 6]
    assert lib.pds_reverb_convolve_units(0, 5, 1) == 0 and lib.pds_reverb_convolve_units(1, 1023, 1) == 2
    assert lib.pds_reverb_convolve_units(2, 1023, 1) == 2 and lib.pds_reverb_convolve_units(1026, 1023, 1) == 4
    assert lib.pds_reverb_convolve_units(1025, 0, 0) == 2 and lib.pds_reverb_convolve_units(2049, 0, 0) == 4
    most = 8 * ((1 << 31) - 1)
    assert lib.pds_reverb_workspace_bytes(3) == 3 * 8192 and lib.pds_reverb_workspace_bytes(most + 1) == -1
    assert lib.pds_reverb_workspace_bytes(-1) == -1
    tw = np.empty(2048, dtype=np.float32)
    assert lib.pds_reverb_twiddles(tw.ctypes.data) == 0
    want = np.exp(-2j * np.pi * np.outer(np.arange(32), np.arange(32)) / 1024).astype(np.complex64).reshape(-1)
    assert np.abs(tw.view(np.complex64) - want).max() <= 2.0 ** -23
    err = lib.pds_stages6_last_error
    assert lib.pds_reverb_twiddles(None) == -1 and b"null pointer" in err()
    # argument errors are reported before any HIP call, through the library's own error string: these run without a
    # device
    for fn in (lib.pds_reverb_spectra_f32, lib.pds_reverb_spectra_f64, lib.pds_reverb_spectra_i16):
        none = (None,) * 5
        assert fn(*none, 1, 2, None, None, None) == -1 and b"null pointer" in err()
        assert fn(*none, 0, 0, None, None, None) == 0 and fn(*none, 3, 0, None, None, None) == 0
        assert fn(*none, -1, 2, None, None, None) == -1 and b"bad size" in err()
        assert fn(*none, 1, -2, None, None, None) == -1 and b"bad size" in err()
        assert fn(*none, 1, most + 1, None, None, None) == -1 and b"2^31 - 1 blocks" in err()
        assert fn(*none, 1, most, None, None, None) == -1 and b"null pointer" in err()
    conv = lib.pds_reverb_convolve

    def call(xtype, B, total, K):
        return conv(None, xtype, None, None, None, None, None, B, total, None, None, None, None, None, None, None, K,
                    None, None, None)

    assert call(0, 0, 0, 0) == 0 and call(0, 4, 0, 1) == 0
    assert call(0, 1, 2, 1) == -1 and b"null pointer" in err()
    one = ctypes.c_void_p(8)  # (any address: the call returns before it looks at memory)
    assert conv(one, 0, one, one, one, one, one, 1, 2, None, None, one, one, one, one, one, 1, one, one, None) == -1
    assert b"null pointer" in err()  # the spectra bank is needed; the workspace alone may be null
    assert call(0, -1, 2, 1) == -1 and b"bad size" in err()
    assert call(0, 1, -2, 1) == -1 and b"bad size" in err()
    assert call(0, 1, 2, -1) == -1 and b"bad size" in err()
    for xtype in (-1, 3):
        assert call(xtype, 1, 2, 1) == -1 and b"xtype" in err()
    assert call(2, 1, most + 1, 1) == -1 and b"2^31 - 1 blocks" in err()
    scale = lib.pds_reverb_scale
    assert scale(None, None, None, None, 0, 10, None) == 0 and scale(None, None, None, None, 5, 0, None) == 0
    assert scale(None, None, None, None, 1, 10, None) == -1 and b"null pointer" in err()
    assert scale(None, None, None, None, -1, 10, None) == -1 and b"bad size" in err()
    assert scale(None, None, None, None, 1, -1, None) == -1 and b"bad size" in err()
    assert scale(None, None, None, None, 65536, 10, None) == -1 and b"65535 utterances" in err()
    assert scale(None, None, None, None, 65535, 32768 * 4096 + 1, None) == -1 and b"2^31 - 1 blocks" in err()
    with pytest.raises(ValueError, match="pds_reverb_convolve"):
        _native.check_stages6(-1, "pds_reverb_convolve")
    with pytest.raises(_native.NativeError, match="code -2"):
        _native.check_stages6(-2, "pds_reverb_convolve")


def test_no_cpu_path_without_a_device(monkeypatch):
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_native.NativeError, match="no CPU fallback"):
        Reverb(_rirs()).apply(np.zeros(100, np.float32))


def test_the_aliases_and_the_constructor():
    for alias in ("reverb", "reverberate", "rir"):
        made = alias_factory_subclass_from_arg(PreProcessor, {"name": alias, "rirs": _rirs(), "prob": 0.8})
        assert isinstance(made, Reverb) and made.prob == 0.8 and made.shift_output and made.normalize_output
    rev = Reverb(_rirs(), shift_output=False, normalize_output=False, seed=3)
    assert rev.seed == 3 and rev.num_rirs == 3 and not rev.normalize_output
    assert rev.rir_lengths.tolist() == [300, 1025, 40] and rev.rir_peaks.tolist() == [0, 0, 0]
    assert Reverb(_rirs()).rir_peaks.tolist() == [10, 600, 39]
    assert Reverb(_rirs()).rir_partitions.tolist() == [1, 3, 1]
    assert "Reverb(rirs=<3>" in repr(rev) and "0x" not in repr(rev)
    assert Reverb([[0.0, -2.0, 2.0]]).rir_peaks.tolist() == [1]  # the first maximum wins a tie
    H = Reverb(_rirs()).spectra()
    assert H.dtype == np.complex64 and H.shape == (5, 1024)
    assert H.tobytes() == np.concatenate([rm.partition_spectra(h) for h in _rirs()]).tobytes()
    with pytest.raises(ValueError, match="empty"):
        Reverb([])
    with pytest.raises(ValueError, match="one channel"):
        Reverb([np.zeros((2, 100))])
    with pytest.raises(ValueError, match="empty"):
        Reverb([np.zeros(0)])
    with pytest.raises(ValueError, match="2\\^20"):
        Reverb([np.zeros((1 << 20) + 1, dtype=np.int16)])
    Reverb([np.ones(1 << 20, dtype=np.int16)])  # (the longest response is taken)
    with pytest.raises(ValueError, match="float32, float64 or int16"):
        Reverb([np.zeros(4, dtype=np.int32)])
    with pytest.raises(ValueError, match="sequence"):
        Reverb(np.zeros(4))
    for prob in (-0.1, 1.5, True, "x", float("nan")):
        with pytest.raises(ValueError, match="prob"):
            Reverb(_rirs(), prob=prob)


def test_a_response_is_read_from_a_file(tmp_path):
    h = rm.response(50, 5, dtype=np.float32)
    np.save(tmp_path / "r.npy", h)
    rev = Reverb([str(tmp_path / "r.npy"), h])
    assert rev.rir_lengths.tolist() == [50, 50] and rev.rir_peaks.tolist() == [5, 5]
    np.save(tmp_path / "two.npy", np.zeros((2, 50), dtype=np.float32))
    with pytest.raises(ValueError, match="one channel"):
        Reverb([str(tmp_path / "two.npy")])


def test_the_plan_api_without_a_device():
    rev = Reverb(_rirs(), prob=0.5, seed=11)
    plan = rev.plan(6, seeds=[1, 2, 3, 4, 5, 1])
    assert isinstance(plan, ReverbPlan) and plan.rir.dtype == np.int64 and plan.applied.dtype == bool
    want_rir, want_applied = rm.plan(ps.pre.dither_keys([1, 2, 3, 4, 5, 1]), 3, 0.5)
    assert plan.rir.tolist() == want_rir.tolist() and plan.applied.tolist() == want_applied.tolist()
    assert plan.rir[0] == plan.rir[5]
    # with seeds the object's sequence is not touched; without, it advances once per utterance
    a, b = Reverb(_rirs(), seed=11), Reverb(_rirs(), seed=11)
    a.plan(3, seeds=[7, 8, 9])
    first = a.plan(2)
    both = b.plan(4)
    assert first.rir.tolist() == both.rir[:2].tolist()
    assert a.plan(2).rir.tolist() == both.rir[2:].tolist()
    assert Reverb(_rirs(), seed=4).plan(1).rir.tolist() == Reverb(_rirs(), seed=4).plan(1, seeds=[4]).rir.tolist()
    assert not Reverb(_rirs(), prob=0.0).plan(50).applied.any() and Reverb(_rirs(), prob=1.0).plan(50).applied.all()
    given = rev.plan(3, seeds=[1, 2, 3], rirs=[2, 2, 0])
    assert given.rir.tolist() == [2, 2, 0] and given.applied.tolist() == plan.applied[:3].tolist()
    assert len(rev.plan(0).rir) == 0
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="B must be"):
            rev.plan(bad)
    with pytest.raises(ValueError, match="one seed"):
        rev.plan(2, seeds=[1])
    with pytest.raises(ValueError, match="outside"):
        rev.plan(1, rirs=[3])
    with pytest.raises(ValueError, match="plan is not one of"):
        rev._check_plan(plan, 5)
    with pytest.raises(ValueError, match="outside"):
        rev._check_plan(ReverbPlan(np.asarray([5]), np.asarray([True])), 1)
    # the layout counts as the library counts
    lib = _native.stages6_lib()
    lens = np.asarray([0, 1, 513, 5000, 2049, 1024], dtype=np.int64)
    plan = ReverbPlan(np.asarray([1, 1, 0, 1, 2, 1]), np.asarray([True, True, True, False, True, True]))
    spec_base, spec_total, unit_base, unit_total = Reverb(_rirs()).layout(lens, plan)
    spec = [lib.pds_reverb_spectra_units(int(n)) if a else 0 for n, a in zip(lens, plan.applied)]
    units = [lib.pds_reverb_convolve_units(int(n), int(Reverb(_rirs()).rir_peaks[j]), int(a))
             for n, j, a in zip(lens, plan.rir, plan.applied)]
    assert spec_base.tolist() == (np.cumsum(spec) - spec).tolist() and spec_total == sum(spec)
    assert unit_base.tolist() == (np.cumsum(units) - units).tolist() and unit_total == sum(units)
    assert Reverb(_rirs()).workspace_bytes(lens, plan) == lib.pds_reverb_workspace_bytes(spec_total)
    # a response of one tap takes no transform: no spectra, copy units
    single = Reverb([np.asarray([0.0, 0.5, 0.0])])
    base, total, _, conv = single.layout([5000], ReverbPlan(np.asarray([0]), np.asarray([True])))
    assert total == 0 and conv == lib.pds_reverb_convolve_units(5000, 1, 0) == 6


def test_a_stream_batch_refuses_a_reverb():
    from pydrobert_speech_amd import multistream

    rev = Reverb(_rirs())
    with pytest.raises(TypeError, match="no streaming form"):
        multistream.streaming_dither(rev)
    with pytest.raises(TypeError, match="no streaming form"):
        multistream.streaming_preemphasis(rev)
    comp = alias_factory_subclass_from_arg(ps.compute.FrameComputer, {"name": "stft", "bank": "fbank"})
    for kwargs in ({"dither": rev}, {"preemphasis": rev}):
        with pytest.raises(TypeError, match="no streaming form"):
            multistream.StreamBatch(comp, 2, **kwargs)


def test_the_command_line_tool_takes_the_stage(tmp_path):
    from pydrobert_speech_amd import command_line as cl

    rev = Reverb(_rirs())
    writer = cl.FeatureDirWriter(None, [rev], [], str(tmp_path / "out"), seed=4)
    assert writer.pre == [rev] and writer.seeded
    assert "reverb" in cl.__doc__ and "Reverb.apply_packed" in cl.__doc__
    got = cl._as_list([{"name": "reverb", "rirs": _rirs(), "prob": 0.8}, "dither"], PreProcessor)
    assert isinstance(got[0], Reverb) and got[0].prob == 0.8
    import inspect

    assert "reverberation (reverb)" in inspect.getsource(cl)
