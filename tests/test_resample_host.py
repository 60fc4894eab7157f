"""The host side of rate conversion (CPU only): ``Resample``'s table against the model's, whether the definition
resamples (model only), the output and due counts, aliases, argument errors, and the stages library's new entry points
against the header and their own argument checks."""
import ctypes
import os

import numpy as np
import pytest

from pydrobert_speech_amd import _native
from pydrobert_speech_amd import pre as pre_module
from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg
from pydrobert_speech_amd.command_line import FeatureDirWriter
from pydrobert_speech_amd.pre import Preemphasize, PreProcessor, Resample
from tests import resample_model as model
from tests.conftest import ROOT

RATE_PAIRS = [(1, 2), (2, 1), (3, 2), (2, 3), (7, 5), (44100, 16000), (16000, 11025), (11025, 16000)]
SMALL_PAIRS = [(1, 2), (2, 1), (3, 2), (2, 3), (7, 5)]

# The largest |w - w_model| / max|w_model| measured over RATE_PAIRS and num_zeros 1 and 6: 0.  Both tables call the C
# library's sin and cos, value by value, on arguments built by the same correctly rounded operations in the same order,
# so there is nothing to differ by.  Allowed: four times what was measured.
WEIGHTS_MEASURED = 0.0
WEIGHTS_ALLOWED = 4 * WEIGHTS_MEASURED

# ---- 1. the table ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("num_zeros", [1, 6])
@pytest.mark.parametrize("rates", RATE_PAIRS, ids=lambda r: f"{r[0]}to{r[1]}")
def test_table_is_the_models(rates, num_zeros):
    rs = Resample(*rates, num_zeros=num_zeros)
    in_unit, out_unit, first, ntaps, w = model.table(*rates, num_zeros=num_zeros)
    assert (rs.in_unit, rs.out_unit, rs.max_taps) == (in_unit, out_unit, int(ntaps.max()))
    assert rs.first.dtype == np.int32 and rs.ntaps.dtype == np.int32 and rs.weights.dtype == np.float64
    assert rs.first.tolist() == first.tolist() and rs.ntaps.tolist() == ntaps.tolist()
    assert rs.last.tolist() == (first + ntaps - 1).tolist()
    assert rs.weights.shape == w.shape == (out_unit, rs.max_taps)
    worst = float(np.abs(rs.weights - w).max() / np.abs(w).max())
    print(f"{rates} num_zeros={num_zeros}: largest weight difference {worst / 2.0 ** -53:.3g} * 2^-53 * max|w|")
    assert worst <= WEIGHTS_ALLOWED
    for table in (rs.first, rs.ntaps, rs.last, rs.weights):  # read-only
        with pytest.raises(ValueError):
            table[...] = 0
    # zeros behind each phase's taps
    assert not rs.weights[np.arange(rs.max_taps)[None, :] >= rs.ntaps[:, None]].any()


def test_table_sizes_of_the_common_rates():
    got = {}
    for rates in ((8000, 16000), (16000, 8000), (48000, 16000), (44100, 16000), (16000, 11025), (11025, 16000)):
        rs = Resample(*rates)
        got[rates] = (rs.in_unit, rs.out_unit, int(rs.ntaps.min()), int(rs.ntaps.max()))
    assert got == {(8000, 16000): (1, 2, 12, 13), (16000, 8000): (2, 1, 25, 25), (48000, 16000): (3, 1, 37, 37),
                   (44100, 16000): (441, 160, 33, 34), (16000, 11025): (640, 441, 17, 18),
                   (11025, 16000): (441, 640, 12, 13)}
    assert Resample.MAX_TABLE >= 16384


def test_a_table_over_the_limit_is_refused():
    rs = Resample(1, 80659)  # 13 taps per phase: 1048567 entries, just within
    assert rs.out_unit * rs.max_taps <= Resample.MAX_TABLE < 80663 * 13
    with pytest.raises(ValueError, match=str(Resample.MAX_TABLE)):
        Resample(1, 80663)
    with pytest.raises(ValueError, match=str(Resample.MAX_TABLE)):
        Resample(1, (1 << 31) - 1)


# ---- 2. does the definition resample? (model only) -------------------------------------------------------------------


def test_the_model_equals_the_scalar_double_loop():
    rng = np.random.default_rng(5)
    for rates in ((3, 2), (2, 3), (7, 5)):
        for dtype in (np.float32, np.float64, np.int16):
            x = np.rint(3000 * rng.standard_normal(61)).astype(dtype)
            assert model.same_bits(model.resample(x, *rates), model.resample_scalar(x, *rates))


@pytest.mark.parametrize("tone,from_rate,to_rate", [(440, 16000, 8000), (440, 8000, 16000), (1000, 44100, 16000),
                                                    (1000, 16000, 11025)])
def test_a_sine_comes_out_as_the_sine_at_the_new_rate(tone, from_rate, to_rate):
    n = from_rate // 2
    x = np.sin(2 * np.pi * tone * np.arange(n) / from_rate)
    y = model.resample(x, from_rate, to_rate)
    assert len(y) == -(-n * to_rate // from_rate)
    at = np.arange(len(y)) / to_rate
    edge = 40 / min(from_rate, to_rate)  # 40 input periods of the lower rate at each end
    inner = (at >= edge) & (at <= n / from_rate - edge)
    assert inner.sum() > 3000
    worst = float(np.abs(y - np.sin(2 * np.pi * tone * at))[inner].max())
    print(f"{tone} Hz, {from_rate} -> {to_rate}: largest difference {worst:.3g}")
    assert worst < 1e-3  # a cap on the definition's pass-band error


# ---- 3. counts -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("rates", RATE_PAIRS, ids=lambda r: f"{r[0]}to{r[1]}")
def test_num_output_samples_is_the_ceiling(rates):
    rs = Resample(*rates)
    ns = np.concatenate([np.arange(0, 3 * rs.in_unit + 3), [10 ** 9, 2 ** 40 + 1]])
    want = [-(-int(n) * rates[1] // rates[0]) for n in ns]
    assert rs.num_output_samples(ns).tolist() == want
    assert [rs.num_output_samples(int(n)) for n in ns[:50]] == want[:50]
    assert isinstance(rs.num_output_samples(7), int)


@pytest.mark.parametrize("rates", SMALL_PAIRS + [(16000, 8000), (8000, 16000), (44100, 16000)],
                         ids=lambda r: f"{r[0]}to{r[1]}")
def test_due_count(rates):
    rs = Resample(*rates)
    top = min(3 * rs.in_unit, 1400)
    ns = np.arange(0, top + 1)
    got = rs.num_due_samples(ns)
    assert got[0] == 0 and (np.diff(got) >= 0).all()  # more samples never take an output back
    assert (got <= rs.num_output_samples(ns)).all()
    step = 1 if rs.out_unit < 10 else 97
    for n in ns[::step].tolist():
        # outputs due after n, plus those finalize adds, are the m of an utterance of n samples
        due = model.due(n, rs.in_unit, rs.out_unit, rs.first, rs.ntaps)
        assert got[n] == due == rs.num_due_samples(n), n
        at_finalize = model.num_output_samples(n, *rates) - due
        assert at_finalize >= 0 and due + at_finalize == rs.num_output_samples(n)
    # far into a stream (once whole units are due) the count moves by out_unit per in_unit
    base = top + 2 * rs.max_taps
    assert rs.num_due_samples(base) == model.due(base, rs.in_unit, rs.out_unit, rs.first, rs.ntaps) >= rs.out_unit
    far = (1 << 40) // rs.in_unit * rs.in_unit
    assert rs.num_due_samples(far + base) == rs.num_due_samples(base) + far // rs.in_unit * rs.out_unit


# ---- 4. the pre-processor's arguments ---------------------------------------------------------------------------------


def test_aliases_and_repr():
    assert "Resample" in pre_module.__all__ and "Resample" in pre_module.__doc__
    for alias in ("resample", "resampling"):
        inst = alias_factory_subclass_from_arg(PreProcessor, {"name": alias, "from_rate": 8000, "to_rate": 16000})
        assert type(inst) is Resample
        assert (inst.from_rate, inst.to_rate, inst.num_zeros, inst.rolloff) == (8000, 16000, 6, 0.99)
    inst = alias_factory_subclass_from_arg(
        PreProcessor, {"alias": "resample", "from_rate": 44100, "to_rate": 16000, "num_zeros": 4, "rolloff": 0.9})
    assert repr(inst) == "Resample(from_rate=44100, to_rate=16000, num_zeros=4, rolloff=0.9)"
    assert repr(Resample(np.int64(3), np.int32(2))) == "Resample(from_rate=3, to_rate=2, num_zeros=6, rolloff=0.99)"
    assert type(alias_factory_subclass_from_arg(PreProcessor, "preemphasis")) is Preemphasize
    assert Resample(5, 5).is_identity and not Resample(5, 4).is_identity


@pytest.mark.parametrize("args", [
    (0, 16000), (16000, 0), (-8000, 16000), (8000, -1), (8000.0, 16000), (8000, 16000.5), ("8000", 16000), (True, 2),
    (None, 16000), (1 << 31, 3), (8000, 16000, 0), (8000, 16000, -2), (8000, 16000, 2.5), (8000, 16000, True),
    (8000, 16000, 6, 0), (8000, 16000, 6, 0.0), (8000, 16000, 6, -0.5), (8000, 16000, 6, 1.01), (8000, 16000, 6, "0.9"),
    (8000, 16000, 6, None), (8000, 16000, 6, float("nan"))])
def test_bad_arguments(args):
    with pytest.raises(ValueError):
        Resample(*args)


def test_apply_refuses_before_it_needs_a_device():
    rs = Resample(3, 2)
    with pytest.raises(ValueError, match="in_place"):
        rs.apply(np.zeros(8, np.float32), in_place=True)
    with pytest.raises(ValueError, match="1-D"):
        rs.apply(np.zeros((2, 8), np.float32))
    with pytest.raises(ValueError, match="1-D"):
        rs.apply(np.float32(1.0))
    same = Resample(2, 2)
    x = np.arange(5, dtype=np.float32)
    assert same.apply(x, in_place=True) is x  # equal rates: nothing to do


def test_the_command_line_tool_accepts_it(tmp_path):
    FeatureDirWriter(None, [Resample(8000, 16000), Preemphasize()], [], str(tmp_path))

    class Other(PreProcessor):
        def apply(self, signal, axis=None, in_place=False):
            return signal

    with pytest.raises(NotImplementedError, match="Other"):
        FeatureDirWriter(None, [Resample(8000, 16000), Other()], [], str(tmp_path))


# ---- 5. the stages library's binding ----------------------------------------------------------------------------------

PACKED = ("pds_resample_packed_f32", "pds_resample_packed_f64", "pds_resample_packed_i16_f32")
STREAMED = ("pds_multistream_resample_f32", "pds_multistream_resample_f64", "pds_multistream_resample_i16_f32")


def test_header_and_signature_table_name_the_new_symbols():
    with open(os.path.join(ROOT, "include", "pds_amd_stages.h")) as fh:
        header = fh.read()
    for name in PACKED:
        restype, argtypes = _native.STAGES_SIGNATURES[name]
        assert restype is ctypes.c_int32 and len(argtypes) == 14 and f"int32_t {name}(" in header
    for name in STREAMED:
        restype, argtypes = _native.STAGES_SIGNATURES[name]
        assert restype is ctypes.c_int32 and len(argtypes) == 13 and f"int32_t {name}(" in header
    assert not set(PACKED + STREAMED) & set(_native.SIGNATURES)  # (the first library's table gained nothing)
    # the definition stands in the header and in the class docstring, word for word
    doc = [line.strip() for line in Resample.__doc__.splitlines()]
    text = [line.strip().lstrip("*").strip() for line in header.splitlines()]
    start, stop = doc.index("The definition.  from_rate and to_rate are positive integers, num_zeros >= 1, 0 < rolloff <= 1."), \
        doc.index("samples reach exactly the outputs whose windows hold them.")
    at = text.index(doc[start])
    assert stop - start > 20 and text[at : at + stop - start + 1] == doc[start : stop + 1]


def test_entry_points_check_their_arguments_before_any_hip_call():
    lib = _native.stages_lib()  # (NativeError if it was not built: there is no fallback)
    err = lib.pds_stages_last_error
    for name in PACKED:
        fn = getattr(lib, name)
        # (d_in, d_in_off, d_in_len, d_out_off, B, max_len, in_unit, out_unit, max_taps, d_first, d_ntaps, d_weights,
        #  d_out, stream)
        assert fn(None, None, None, None, 0, 100, 1, 2, 13, None, None, None, None, None) == 0  # an empty batch
        assert fn(None, None, None, None, 3, 0, 1, 2, 13, None, None, None, None, None) == 0  # no output
        assert fn(None, None, None, None, 3, 100, 1, 2, 13, None, None, None, None, None) == -1
        assert b"null pointer" in err()
        assert fn(None, None, None, None, -1, 100, 1, 2, 13, None, None, None, None, None) == -1
        assert b"bad size" in err()
        assert fn(None, None, None, None, 3, -100, 1, 2, 13, None, None, None, None, None) == -1
        assert b"bad size" in err()
        for units in ((0, 2, 13), (1, 0, 13), (1, 2, 0), (-1, 2, 13)):
            assert fn(None, None, None, None, 3, 100, *units, None, None, None, None, None) == -1
            assert b"positive" in err()
        assert fn(None, None, None, None, 3, 100, 1, 80663, 13, None, None, None, None, None) == -1
        assert b"1048576" in err()
        assert fn(None, None, None, None, 1 << 30, 1 << 40, 1, 2, 13, None, None, None, None, None) == -1
        assert b"split the batch" in err()
    for name in STREAMED:
        fn = getattr(lib, name)
        # (d_samples, d_hist, capacity, in_unit, out_unit, max_taps, d_first, d_ntaps, d_weights, d_meta, n, d_out, stream)
        assert fn(None, None, 4, 1, 2, 13, None, None, None, None, 0, None, None) == 0
        assert fn(None, None, 4, 1, 2, 13, None, None, None, None, 2, None, None) == -1
        assert b"null pointer" in err()
        assert fn(None, None, 4, 1, 2, 13, None, None, None, None, -2, None, None) == -1
        assert fn(None, None, -4, 1, 2, 13, None, None, None, None, 2, None, None) == -1
        assert b"bad size" in err()
        assert fn(None, None, 4, 1, 0, 13, None, None, None, None, 2, None, None) == -1
        assert b"positive" in err()
        assert fn(None, None, 4, 1, 80663, 13, None, None, None, None, 2, None, None) == -1
        assert b"1048576" in err()
    with pytest.raises(ValueError, match="pds_resample_packed"):
        _native.check_stages(-1, "pds_resample_packed")
