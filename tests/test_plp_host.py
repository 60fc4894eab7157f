"""``post.PLP`` without a device: known answers of the numpy model that do not depend on Kaldi; the constructor's and
the width's refusals; aliases and JSON configs; what a computer fills in; the fourth library's header against its
signature table, its exports and its argument errors; the definition word for word in the docstring, the header and
DESIGN.md; ``NativeError`` without the library or a device; the refusals of ``StreamBatch``, ``SiStreamBatch`` and the
command-line tool; and the stage's place in the tick pipeline."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from pydrobert_speech_amd import _native
from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg
from pydrobert_speech_amd.command_line import FeatureDirWriter, signals_to_torch_feat_dir
from pydrobert_speech_amd.compute import FrameComputer
from pydrobert_speech_amd.multistream import StreamBatch, _PlpStage, streaming_plp
from pydrobert_speech_amd.multistream_si import SiStreamBatch
from pydrobert_speech_amd.post import PCEN, PLP, Cepstra, PostProcessor
from tests.conftest import ROOT
from tests.plp_model import (energies, plp_from_autocorrelation, plp_from_spectrum, plp_model, plp_tables, same_bits,
                             within_tolerance)
from tests.test_multistream_host import golden_configs

LINEAR = dict(golden_configs()["c1_kaldi_fbank"], use_log=False)
LOGGED = dict(golden_configs()["c1_kaldi_fbank"], use_log=True)
SI_LINEAR = {"name": "si", "bank": {"name": "fbank", "num_filts": 40}, "use_log": False}
SI_LOGGED = {"name": "si", "bank": {"name": "fbank", "num_filts": 40}}


def build(cfg):
    return alias_factory_subclass_from_arg(FrameComputer, json.loads(json.dumps(cfg)))


def centers(F):
    return [60.0 + 7900.0 * (f + 0.5) / F for f in range(F)]


# ---- 1. known answers of the model ----------------------------------------------------------------------------------


def test_an_ar1_spectrum_gives_its_coefficient_and_the_cepstrum_of_a_pole():
    alpha, p = 0.5, 12
    r = alpha ** np.arange(p + 1, dtype=np.float64)[None, :]
    a, q, E = plp_from_autocorrelation(r, p)
    assert a[0, 0] == -alpha and not a[0, 1:].any()  # exactly
    assert E[0] == 1.0 - alpha * alpha
    assert q[0].tolist() == [alpha ** n / n for n in range(1, p + 1)]
    assert q[0, :4].tolist() == [0.5, 0.125, 1.0 / 24.0, 1.0 / 64.0]


def test_the_clamp_engages_for_a_constant_autocorrelation():
    p = 12
    a, q, E = plp_from_autocorrelation(np.ones((1, p + 1)), p)
    assert E[0] == 1e-5  # k = 1 in the first step: 1 - k^2 = 0 is clamped; every later k is 0
    assert a[0, 0] == -1.0 and not a[0, 1:].any()
    # ... and it lets a NaN pass
    r = 0.3 ** np.arange(p + 1, dtype=np.float64)[None, :]
    r[0, 0] = np.nan
    a, q, E = plp_from_autocorrelation(r, p)
    assert np.isnan(E).all() and np.isnan(q).all()


@pytest.mark.parametrize("F", [1, 2, 5, 23, 40, 254])
def test_a_flat_weighted_spectrum_gives_zero_cepstra(F):
    p = min(F + 1, 12)
    post = PLP(num_ceps=p + 1, lpc_order=p, centers_hz=centers(F))
    w, _, _ = plp_tables(post, F)
    out = plp_model(post, (1.0 / w)[None, :])
    assert out.shape == (1, p + 1) and (np.abs(out) < 1e-12).all()
    # a row of zeros is finite, because of the floor; a row holding a NaN is NaN in every computed column
    assert np.isfinite(plp_model(post, np.zeros((1, F)))).all()
    x = np.arange(1.0, F + 1.0)[None, :]
    x[0, F // 2] = np.nan
    assert np.isnan(plp_model(post, x)).all()
    with_energy = PLP(num_ceps=p + 1, lpc_order=p, centers_hz=centers(F), energy=True)
    y = plp_model(with_energy, np.concatenate([[[7.5]], x], axis=1))
    assert y[0, 0] == np.log(7.5) and np.isnan(y[0, 1:]).all()


def test_the_objects_tables_are_the_models_bit_for_bit():
    for F in (1, 2, 23, 40, 65, 254):
        for energy in (False, True):
            p = min(F + 1, 32)
            for kw in ({}, {"equal_loudness": False, "lifter": 0, "scale": 0.1}, {"lifter": None}):
                post = PLP(num_ceps=p + 1, lpc_order=p, centers_hz=centers(F), energy=energy, **kw)
                mine, theirs = post.tables(F + energy), plp_tables(post, F + energy)
                assert [t.shape for t in mine] == [(F,), (p + 1, F + 2), (p + 1,)]
                assert all(same_bits(a, b) for a, b in zip(mine, theirs)), (F, energy, kw)
                assert post.aux_width(F + energy) == F + 3
    post = PLP(equal_loudness=False, lifter=0, scale=0.1)
    w, B, L = post.tables(23)
    assert (w == 1.0).all() and (L == 0.1).all()
    assert (B[:, 0] == 1.0 / 48.0).all() and (B[0, 1:-1] == 2.0 / 48.0).all() and B[0, -1] == 1.0 / 48.0
    assert abs(B[0].sum() - 1.0) < 1e-15  # (r[0] of a flat spectrum of ones is 1)


def test_a_two_ulp_change_of_the_spectrum_moves_no_output_by_a_thousandth_of_the_tolerance():
    """the conditioning of steps 5 to 7 on the tests' inputs: what the device's ``pow`` may differ by from numpy's is
    far inside the standing tolerance, so that tolerance tests the kernel"""
    rng = np.random.default_rng(5)
    worst = 0.0
    for F in (1, 2, 5, 23, 40):
        p = min(F + 1, 12)
        post = PLP(num_ceps=p + 1, lpc_order=p, centers_hz=centers(F))
        w, B, L = plp_tables(post, F)
        x = energies(rng, (200, F), np.float64, sigma=4.0)
        from tests.plp_model import plp_spectrum

        d = plp_spectrum(post, x, w)
        q0, E0 = plp_from_spectrum(d, B)
        up = np.nextafter(np.nextafter(d, np.inf), np.inf)
        q1, E1 = plp_from_spectrum(np.where(rng.random(d.shape) < 0.5, up, d), B)
        y0 = np.concatenate([L[0] * np.log(E0)[:, None], L[None, 1:] * q0[:, :p]], axis=1)
        y1 = np.concatenate([L[0] * np.log(E1)[:, None], L[None, 1:] * q1[:, :p]], axis=1)
        worst = max(worst, float((np.abs(y1 - y0) / (1e-9 + 1e-9 * np.abs(y0))).max()))
    print("worst move of an output, in float64 tolerances:", worst)
    assert worst < 1e-3


# ---- 2. arguments, aliases, configs ---------------------------------------------------------------------------------


def test_defaults():
    post = PLP()
    assert (post.num_ceps, post.lpc_order, post.compress_factor, post.lifter, post.scale) == (13, 12, 1.0 / 3.0, 22.0, 1.0)
    assert (post.equal_loudness, post.centers_hz, post.floor, post.energy) == (True, None, 2.0 ** -126, False)
    assert PLP(lifter=None).lifter == 0.0 and PLP(energy=True).energy is True and PLP(energy=False).energy is False
    assert PLP(centers_hz=np.arange(3.0)).centers_hz == (0.0, 1.0, 2.0)
    assert isinstance(PLP(compress_factor=np.float32(0.5)).compress_factor, float)


@pytest.mark.parametrize("kwargs", [
    {"lpc_order": 0}, {"lpc_order": 33}, {"lpc_order": 12.0}, {"lpc_order": True}, {"lpc_order": None},
    {"num_ceps": 0}, {"num_ceps": 14}, {"num_ceps": 3, "lpc_order": 1}, {"num_ceps": 2.0}, {"num_ceps": False},
    {"compress_factor": 0.0}, {"compress_factor": -1.0}, {"compress_factor": float("inf")},
    {"compress_factor": float("nan")}, {"compress_factor": "0.33"}, {"compress_factor": None},
    {"floor": 0.0}, {"floor": -1e-30}, {"floor": float("nan")}, {"floor": None},
    {"lifter": -1.0}, {"lifter": float("inf")}, {"lifter": float("nan")}, {"lifter": "22"}, {"lifter": True},
    {"scale": -0.1}, {"scale": float("inf")}, {"scale": float("nan")}, {"scale": None}, {"scale": "1"},
    {"equal_loudness": 1}, {"equal_loudness": None}, {"energy": 1}, {"energy": "yes"},
    {"centers_hz": []}, {"centers_hz": [[1.0, 2.0]]}, {"centers_hz": [100.0, float("nan")]}, {"centers_hz": [-1.0]},
    {"centers_hz": "abc"}, {"centers_hz": 100.0},
])
def test_bad_arguments_are_value_errors(kwargs):
    with pytest.raises(ValueError, match="PLP"):
        PLP(**kwargs)


def test_the_widths_refusals_come_before_any_device_work(monkeypatch):
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # (a device would be a NativeError)
    flat = dict(equal_loudness=False)
    for post, width in (
        (PLP(**flat), 257),  # W > 256
        (PLP(energy=True, **flat), 257),
        (PLP(**flat), 10),  # p = 12 > F + 1 = 11
        (PLP(energy=True, **flat), 11),
        (PLP(num_ceps=2, lpc_order=3, **flat), 1),
        (PLP(num_ceps=1, lpc_order=1, energy=True, **flat), 1),  # F = 0
        (PLP(), 23),  # equal loudness without centres
        (PLP(centers_hz=centers(22)), 23),  # ... with another count of them
        (PLP(centers_hz=centers(23), energy=True), 23),
    ):
        with pytest.raises(ValueError, match="PLP"):
            post.apply(np.ones((4, width), dtype=np.float32))
        with pytest.raises(ValueError, match="PLP"):
            post.apply(np.ones((width, 4), dtype=np.float32), axis=0)
        with pytest.raises(ValueError, match="PLP"):
            post.apply_rows(torch.ones(4, width))
        with pytest.raises(ValueError, match="PLP"):
            post.tables(width)
    # the bounds themselves are served
    for post, width in ((PLP(**flat), 256), (PLP(energy=True, **flat), 256), (PLP(**flat), 11),
                        (PLP(num_ceps=3, lpc_order=2, **flat), 1), (PLP(num_ceps=33, lpc_order=32, **flat), 31)):
        with pytest.raises(_native.NativeError, match="no HIP device"):
            post.apply(np.ones((4, width), dtype=np.float32))
    with pytest.raises(ValueError, match="at least one dimension"):
        PLP(**flat).apply(np.float32(1.0))


def test_aliases_and_json_configs():
    assert PLP.aliases == {"plp", "plp_cepstra", "rasta_plp_off"}

    def carriers(klass, alias):
        return [k for k in [klass, *klass.__subclasses__()] if alias in k.__dict__.get("aliases", ())] + [
            c for sub in klass.__subclasses__() for c in carriers(sub, alias) if c is not sub]
    for alias in PLP.aliases:
        assert set(carriers(PostProcessor, alias)) == {PLP}
        assert type(alias_factory_subclass_from_arg(PostProcessor, alias)) is PLP
    cfg = {"name": "plp", "num_ceps": 9, "lpc_order": 10, "compress_factor": 0.5, "lifter": 0, "scale": 0.1,
           "equal_loudness": False, "floor": 1e-20, "energy": True}
    post = alias_factory_subclass_from_arg(PostProcessor, json.loads(json.dumps(cfg)))
    assert type(post) is PLP
    assert (post.num_ceps, post.lpc_order, post.compress_factor, post.lifter, post.scale) == (9, 10, 0.5, 0.0, 0.1)
    assert (post.equal_loudness, post.floor, post.energy, post.centers_hz) == (False, 1e-20, True, None)
    # the object's arguments go through JSON and come back as the same object
    again = alias_factory_subclass_from_arg(PostProcessor, json.loads(json.dumps(dict(post._arguments(), name="plp"))))
    assert again._arguments() == post._arguments()
    post = alias_factory_subclass_from_arg(PostProcessor, {"alias": "plp_cepstra", "centers_hz": [100.0, 200.0]})
    assert post.centers_hz == (100.0, 200.0) and post._arguments()["energy"] is None
    with pytest.raises(ValueError, match="PLP"):
        alias_factory_subclass_from_arg(PostProcessor, {"name": "plp", "lpc_order": 40})
    with pytest.raises(TypeError):
        alias_factory_subclass_from_arg(PostProcessor, {"name": "plp", "norm": "ortho"})
    assert streaming_plp(None) is None and streaming_plp("plp").num_ceps == 13
    assert streaming_plp({"name": "plp", "num_ceps": 5}).num_ceps == 5
    with pytest.raises(ValueError, match="post.PLP"):
        streaming_plp({"name": "mfcc"})
    with pytest.raises(ValueError, match="no post-processor"):
        streaming_plp(3)


def test_a_computer_fills_in_what_the_object_leaves_open():
    comp = build(LINEAR)
    F = comp.bank.num_filts
    post = PLP.for_computer(comp)
    assert post.centers_hz == tuple(float(c) for c in comp.bank.centers_hz) and len(post.centers_hz) == F
    assert post.energy == comp.includes_energy
    with_energy = build(dict(LINEAR, include_energy=True))
    assert PLP.for_computer(with_energy).energy is True and PLP.for_computer(with_energy, energy=False).energy is False
    assert PLP.for_computer(comp, energy=True, num_ceps=5).energy is True
    mine = PLP(centers_hz=centers(F), energy=False)
    assert mine.bound_to(comp) is mine  # nothing open: the object itself
    assert PLP.for_computer(comp, centers_hz=centers(F)).centers_hz == tuple(centers(F))
    flat = PLP(equal_loudness=False)
    bound = flat.bound_to(with_energy)
    assert bound is not flat and bound.energy and bound.centers_hz is None and flat.energy is False  # (not changed)
    for cfg in (LOGGED, SI_LOGGED):
        with pytest.raises(ValueError, match="PLP takes linear energies"):
            PLP.for_computer(build(cfg))
    assert len(PLP.for_computer(build(SI_LINEAR)).centers_hz) == 40


# ---- 3. the fourth library's binding --------------------------------------------------------------------------------


def test_stages4_header_and_signature_table_name_the_same_set():
    with open(os.path.join(ROOT, "include", "pds_amd_stages4.h")) as fh:
        header = fh.read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = dict(re.findall(r"\b(pds_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code))
    assert set(declared) == set(_native.STAGES4_SIGNATURES), set(declared) ^ set(_native.STAGES4_SIGNATURES)
    assert {"pds_stages4_version", "pds_stages4_last_error", "pds_plp_rows_f32", "pds_plp_rows_f64"} <= set(declared)
    for name, args in declared.items():
        restype, argtypes = _native.STAGES4_SIGNATURES[name]
        count = 0 if args.strip() == "void" else len(args.split(","))
        assert count == len(argtypes), name
    assert len(_native.STAGES4_SIGNATURES["pds_plp_rows_f32"][1]) == 16
    assert _native.STAGES4_SIGNATURES["pds_plp_rows_f64"][0] is ctypes.c_int32
    assert _native.STAGES4_SIGNATURES["pds_plp_lds_bytes"][0] is ctypes.c_int64
    # it shares no header with the other libraries
    for other in ("pds_amd.h", "pds_amd_stages.h", "pds_amd_stages2.h", "pds_amd_stages3.h", "pds_internal.h",
                  "stages_internal.h"):
        assert f'"{other}"' not in header and f"/{other}" not in code


def test_plp_hip_includes_its_header_and_the_rule_and_nothing_else_of_the_project():
    csrc = os.path.join(ROOT, "pydrobert-speech_amd", "csrc")
    with open(os.path.join(csrc, "plp.hip")) as fh:
        includes = re.findall(r'#include\s+"([^"]+)"', fh.read())
    assert includes == ["../../include/pds_amd_stages4.h", "plp_rule.h"]
    # ... and the rule is included by nothing but plp.hip (and the CPU test)
    users = []
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")) and name != "plp_rule.h":
            with open(os.path.join(csrc, name)) as fh:
                if "plp_rule.h" in re.findall(r'#include\s+"([^"]+)"', fh.read()):
                    users.append(name)
    assert users == ["plp.hip"]
    with open(os.path.join(csrc, "plp_rule.h")) as fh:
        assert re.findall(r'#include\s+"([^"]+)"', fh.read()) == []
    with open(os.path.join(csrc, "Makefile")) as fh:
        make = fh.read()
    assert "STAGES4_LIB  = libpds_amd_stages4.so" in make and "STAGES4_OBJS = plp.o" in make
    assert re.search(r"^all:.*\$\(STAGES4_LIB\)", make, flags=re.M)
    command = subprocess.run(["make", "-n", "-B", "plp.o"], cwd=csrc, check=True, capture_output=True, text=True).stdout
    assert "plp.hip" in command and "-ffp-contract=off" in command
    assert "STAGES3_OBJS = specaug.o\n" in make  # the third library keeps the SpecAugment kernels and no other


def _definition(text):
    text = " ".join(text.split())
    start, end = "Notation for a row `x` of width `W`:", "A row of zeros is finite, because of the floor."
    return text[text.index(start): text.index(end) + len(end)]


def test_the_definition_is_in_the_docstring_the_header_and_the_design_word_for_word():
    doc = _definition(PLP.__doc__)
    assert len(doc) > 2500
    with open(os.path.join(ROOT, "include", "pds_amd_stages4.h")) as fh:
        header = "\n".join(re.sub(r"^\s*\*\s?", "", line) for line in fh.read().splitlines())
    assert _definition(header) == doc
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        design = fh.read()
    assert "4.11" in design and _definition(design[design.index("4.11"):]) == doc


def test_stages4_library_exports_every_declared_symbol_and_reports_argument_errors():
    lib = _native.stages4_lib()  # (NativeError if it was not built: there is no fallback)
    for name in _native.STAGES4_SIGNATURES:
        assert getattr(lib, name) is not None
    assert lib.pds_stages4_version() >= 100
    assert isinstance(lib.pds_stages4_last_error(), bytes)
    assert lib.pds_plp_block_rows() == 64
    assert [lib.pds_plp_lds_bytes(p) for p in (0, 1, 12, 32, 33)] == [-1, 3 * 512, 25 * 512, 65 * 512, -1]
    # argument errors are reported before any HIP call, through the library's own error string: these run without a
    # device
    ok = dict(stride=23, R=5, F=23, copy=0, p=12, K=13, cf=1.0 / 3.0, floor=2.0 ** -126, out_stride=13)

    def call(fn=lib.pds_plp_rows_f32, **kw):
        a = dict(ok, **kw)
        return fn(None, a["stride"], a["R"], a["F"], a["copy"], None, None, None, a["p"], a["K"], a["cf"], a["floor"],
                  None, a["out_stride"], None, None)
    for fn in (lib.pds_plp_rows_f32, lib.pds_plp_rows_f64):
        assert call(fn) == -1 and b"null pointer" in lib.pds_stages4_last_error()
        assert call(fn, R=0) == 0  # (no rows: the pointers are not looked at)
        assert call(fn, R=-1) == -1 and b"bad size" in lib.pds_stages4_last_error()
        for bad in (dict(F=0), dict(F=257), dict(F=256, copy=1), dict(copy=2), dict(copy=-1), dict(p=0), dict(p=33),
                    dict(F=10, stride=10), dict(K=0), dict(K=14), dict(F=1, stride=1, p=3)):
            assert call(fn, **bad) == -1 and b"1 <= F" in lib.pds_stages4_last_error(), bad
        for bad in (0.0, -0.5, float("inf"), float("nan")):
            assert call(fn, cf=bad) == -1 and b"compress_factor" in lib.pds_stages4_last_error()
        for bad in (0.0, -1.0, float("nan")):
            assert call(fn, floor=bad) == -1 and b"floor" in lib.pds_stages4_last_error()
        assert call(fn, stride=22) == -1 and b"stride" in lib.pds_stages4_last_error()
        assert call(fn, copy=1, stride=23) == -1 and b"stride" in lib.pds_stages4_last_error()
        assert call(fn, out_stride=12) == -1 and b"stride" in lib.pds_stages4_last_error()
        assert call(fn, R=64 * ((1 << 31) - 1) + 1) == -1 and b"too many rows" in lib.pds_stages4_last_error()
        assert call(fn, R=64 * ((1 << 31) - 1)) == -1 and b"null pointer" in lib.pds_stages4_last_error()
    with pytest.raises(ValueError, match="pds_plp_rows"):
        _native.check_stages4(-1, "pds_plp_rows")
    with pytest.raises(_native.NativeError, match="code -2"):
        _native.check_stages4(-2, "pds_plp_rows")


def test_no_cpu_path_without_a_device(monkeypatch):
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    post = PLP(centers_hz=centers(23))
    x = np.ones((10, 23), dtype=np.float32)
    for call in (lambda: post.apply(x), lambda: post.apply(x.T, axis=0), lambda: post.apply_rows(torch.ones(4, 23)),
                 lambda: post.apply_rows(torch.ones(4, 23), [0, 4])):
        with pytest.raises(_native.NativeError, match="no HIP device"):
            call()
    with pytest.raises(_native.NativeError, match="no HIP device"):
        StreamBatch(build(LINEAR), capacity=4, plp=PLP())


# ---- 4. the refusals of the stream batches and the tool -------------------------------------------------------------


def test_stream_batches_refuse_logs_rival_stages_and_widths(monkeypatch):
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # (the refusals come before any device is asked for)
    for cls, logged, linear in ((StreamBatch, LOGGED, LINEAR), (SiStreamBatch, SI_LOGGED, SI_LINEAR)):
        for plp in (PLP(), "plp", {"name": "plp", "num_ceps": 5}):
            with pytest.raises(ValueError, match="PLP takes linear energies"):
                cls(build(logged), capacity=4, plp=plp)
            with pytest.raises(ValueError, match="without cepstra and pcen"):
                cls(build(linear), capacity=4, plp=plp, cepstra=Cepstra(13))
            with pytest.raises(ValueError, match="without cepstra and pcen"):
                cls(build(linear), capacity=4, plp=plp, pcen=PCEN())
        # a width the object refuses: more LPC coefficients than the bank supports, centres of another bank
        narrow = dict(linear, bank=dict(name="fbank", num_filts=8)) if cls is SiStreamBatch else None
        if narrow is not None:
            with pytest.raises(ValueError, match="lpc_order"):
                cls(build(narrow), capacity=4, plp=PLP())
        with pytest.raises(ValueError, match="centre frequencies"):
            cls(build(linear), capacity=4, plp=PLP(centers_hz=[100.0, 200.0]))
        with pytest.raises(_native.NativeError, match="no HIP device"):  # (accepted: the device comes next)
            cls(build(linear), capacity=4, plp=PLP())
    with pytest.raises(ValueError, match="PLP takes linear energies"):
        streaming_plp("plp", build(LOGGED))
    bound = streaming_plp("plp", build(LINEAR))
    assert len(bound.centers_hz) == build(LINEAR).bank.num_filts


def test_the_command_line_tool_binds_the_stage_and_refuses_a_computer_that_takes_logs(tmp_path):
    map_path = tmp_path / "map.txt"
    map_path.write_text(f"utt0 {tmp_path / 'missing.npy'}\n")
    for cfg in (LOGGED, SI_LOGGED):
        for spec in ('[{"name": "plp"}]', '[{"name": "deltas", "num_deltas": 2}, "plp"]'):
            with pytest.raises(ValueError, match="PLP takes linear energies"):
                signals_to_torch_feat_dir([str(map_path), json.dumps(cfg), str(tmp_path / "out"), "--postprocess", spec])
    comp = build(dict(LINEAR, include_energy=True))
    given = PLP(num_ceps=5)
    writer = FeatureDirWriter(comp, [], [given, Cepstra(3)], str(tmp_path / "out2"))
    bound = writer.post[0]
    assert type(bound) is PLP and bound is not given and bound.num_ceps == 5 and bound.energy is True
    assert bound.centers_hz == tuple(float(c) for c in comp.bank.centers_hz) and given.centers_hz is None
    assert type(writer.post[1]) is Cepstra
    said = FeatureDirWriter(comp, [], [PLP(energy=False, equal_loudness=False)], str(tmp_path / "out3")).post[0]
    assert said.energy is False and said.centers_hz is None


# ---- 5. the stage's place in the tick pipeline ----------------------------------------------------------------------


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
    pds_multistream_cmvn_f32 = pds_multistream_cmvn_f64 = "cmvn"

    @staticmethod
    def pds_multistream_tile():
        return 1024


def fake_batch(monkeypatch, cfg=LINEAR, **kwargs):
    from pydrobert_speech_amd import multistream

    asked = []

    class Native:
        require_device = staticmethod(lambda: _FakeTorch)
        lib = staticmethod(lambda: _FakeLib)
        stages4_lib = staticmethod(lambda: asked.append("stages4"))

    monkeypatch.setattr(multistream, "_native", Native)
    comp = build(cfg)
    monkeypatch.setattr(type(comp), "_native_plan", lambda self, device=None: None)
    return comp, StreamBatch(comp, capacity=8, **kwargs), asked


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_stage_stands_in_cepstras_place_and_owns_nothing(monkeypatch, dtype):
    comp, sb, asked = fake_batch(monkeypatch, dtype=dtype, plp=PLP(num_ceps=7), cmvn="cmvn")
    assert list(sb._stages) == ["plp", "cmvn"] and isinstance(sb._stages["plp"], _PlpStage)
    stage = sb._stages["plp"]
    F = comp.num_coeffs
    assert (sb._F0, sb._F, sb.num_coeffs, sb.lookahead, sb.num_vectors) == (F, 7, 7, 0, 1)
    assert (stage.width_in, stage.width, stage.pools, stage.sections, stage.state) == (F, 7, {}, (), None)
    assert sb._stages["cmvn"].width == 7 and asked == ["stages4"]
    assert stage.spec.centers_hz == tuple(float(c) for c in comp.bank.centers_hz)  # bound to the batch's computer
    rows = np.asarray([0, 2, 5], dtype=np.int64)
    assert stage.plan(None, np.asarray([1, 2]), rows, False) is rows
    assert sb._layout_flags == (False, True, False, False, False)  # no section of its own
    sb.close()
    # a batch without the stage does not ask for the library
    _, plain, asked = fake_batch(monkeypatch, dtype=dtype)
    assert "plp" not in plain._stages and asked == []
    # with the energy column the object takes it from the computer
    _, sb, _ = fake_batch(monkeypatch, cfg=dict(LINEAR, include_energy=True), dtype=dtype, plp="plp")
    assert sb._stages["plp"].spec.energy is True and sb.num_coeffs == 13
