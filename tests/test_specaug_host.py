"""``post.SpecAugment`` without a device: the model's Philox against Random123's known answers and the draws' spread;
aliases, JSON configs, every argument error, ``__repr__``; the fourth library's header against its signature table,
its exports and its argument errors; ``NativeError`` without the library or a device; and, over a fake native layer
that reads the host memory it is handed, the seed sequence, the refusals of ``apply_rows`` and the splitting of a batch
that needs more blocks than one launch holds (the limit itself, 2^31 - 1 blocks, is out of reach of a test's memory:
the split is tested here with a smaller limit and nowhere on the GPU)."""
import contextlib
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest

from pydrobert_speech_amd import _native, post as post_module
from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg
from pydrobert_speech_amd.post import PostProcessor, SpecAugment
from tests import specaug_model as sm
from tests.conftest import ROOT

# ---- 1. the generator -----------------------------------------------------------------------------------------------

KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_the_models_philox_gives_random123s_known_answers():
    for counter, key, want in KNOWN:
        assert tuple(int(v) for v in sm.philox(counter, key)) == want
    got = sm.philox([k[0] for k in KNOWN], [k[1] for k in KNOWN])  # ... and vectorised
    assert got.shape == (3, 4) and [tuple(int(v) for v in row) for row in got] == [k[2] for k in KNOWN]
    # P(i, d) has counter (i, 0, d, 0) and key (k mod 2^32, k >> 32)
    key = np.asarray([0x299F31D0A4093822], dtype=np.uint64)
    assert (sm.draw(5, 3, key)[0] == sm.philox((5, 0, 3, 0), (0xA4093822, 0x299F31D0))).all()


def test_u_stays_in_its_range():
    for r in (0, 1, 0x7FFFFFFF, 0xFFFFFFFF):
        for n in (0, 1, 7, (1 << 31) - 1):
            assert 0 <= int(sm.uniform(r, n)) <= n
    assert int(sm.uniform(0xFFFFFFFF, (1 << 31) - 1)) == (1 << 31) - 1 and int(sm.uniform(0xFFFFFFFF, 0)) == 0


def test_the_draws_are_not_degenerate():
    """seeds 0 .. 4095, every domain and the two words the plan uses: the counts of U(r, 7) lie within 100 of 512 (the
    binomial sigma is 21: under 5 sigma)"""
    keys = sm.dither_keys(range(4096))
    assert len(set(keys.tolist())) == 4096
    worst = 0
    for d in (1, 2, 3):
        r = sm.draw(0, d, keys)
        for word in (0, 1):
            counts = np.bincount(sm.uniform(r[:, word], 7), minlength=8)
            assert len(counts) == 8 and counts.sum() == 4096
            worst = max(worst, int(np.abs(counts - 512).max()))
            assert np.abs(counts - 512).max() <= 100, (d, word, counts)
    print("the count farthest from 512:", worst, "away")


# ---- 2. arguments, aliases, configs ---------------------------------------------------------------------------------


def test_defaults_and_limits():
    post = SpecAugment()
    assert (post.freq_masks, post.freq_width, post.time_masks, post.time_width) == (2, 10, 2, 50)
    assert (post.time_ratio, post.warp, post.fill, post.seed) == (1.0, 0, 0.0, None)
    assert post.plan_words == 10 and isinstance(post.time_ratio, float) and isinstance(post.fill, float)
    edge = SpecAugment(16, (1 << 31) - 2, 16, (1 << 31) - 2, 1e-300, 1 << 29, "mean", 0)
    assert edge.plan_words == 66 and edge.fill == "mean" and edge.seed == 0
    zero = SpecAugment(0, 0, 0, 0, 1, 0, np.float32(-1.5), np.int64(3))
    assert zero.plan_words == 2 and zero.fill == -1.5 and zero.time_ratio == 1.0
    for fill in (float("nan"), float("inf"), -float("inf"), 3):
        assert isinstance(SpecAugment(fill=fill).fill, float)
    assert np.isnan(SpecAugment(fill=float("nan")).fill)


@pytest.mark.parametrize("kwargs", [
    {"freq_masks": -1}, {"freq_masks": 17}, {"freq_masks": 2.0}, {"freq_masks": True}, {"freq_masks": "2"},
    {"time_masks": -1}, {"time_masks": 17}, {"time_masks": 1.5}, {"time_masks": None},
    {"freq_width": -1}, {"freq_width": (1 << 31) - 1}, {"freq_width": 10.0}, {"freq_width": False},
    {"time_width": -1}, {"time_width": (1 << 31) - 1}, {"time_width": "50"}, {"time_width": [50]},
    {"time_ratio": 0.0}, {"time_ratio": -0.5}, {"time_ratio": 1.0000001}, {"time_ratio": float("nan")},
    {"time_ratio": float("inf")}, {"time_ratio": "1.0"}, {"time_ratio": True}, {"time_ratio": None},
    {"warp": -1}, {"warp": (1 << 29) + 1}, {"warp": 5.0}, {"warp": True},
    {"fill": "zero"}, {"fill": None}, {"fill": True}, {"fill": [0.0]}, {"fill": "Mean"},
    {"seed": -1}, {"seed": 1.5}, {"seed": "7"}, {"seed": True},
])
def test_bad_arguments_are_value_errors(kwargs):
    with pytest.raises(ValueError, match="SpecAugment"):
        SpecAugment(**kwargs)


def test_aliases_and_json_configs():
    assert SpecAugment.aliases == {"specaugment", "spec_augment", "specaug"}

    def carriers(klass, alias):
        found = [klass] if alias in klass.__dict__.get("aliases", ()) else []
        return found + [c for sub in klass.__subclasses__() for c in carriers(sub, alias)]

    for alias in SpecAugment.aliases:
        assert set(carriers(PostProcessor, alias)) == {SpecAugment}
        assert type(alias_factory_subclass_from_arg(PostProcessor, alias)) is SpecAugment
    post = alias_factory_subclass_from_arg(
        PostProcessor, json.loads('{"name": "specaugment", "warp": 2, "fill": "mean", "seed": 3}'))
    assert type(post) is SpecAugment and (post.warp, post.fill, post.seed, post.freq_masks) == (2, "mean", 3, 2)
    post = alias_factory_subclass_from_arg(PostProcessor, {"alias": "specaug", "time_ratio": 0.2, "fill": -1})
    assert type(post) is SpecAugment and (post.time_ratio, post.fill) == (0.2, -1.0)
    with pytest.raises(ValueError):
        alias_factory_subclass_from_arg(PostProcessor, {"name": "spec_augment", "freq_masks": 17})
    with pytest.raises(TypeError):
        alias_factory_subclass_from_arg(PostProcessor, {"name": "specaugment", "adaptive": True})


def test_repr_shows_the_constructor_arguments_only():
    post = SpecAugment(1, 7, 3, 20, 0.5, 4, "mean", seed=11)
    text = repr(post)
    assert text == ("SpecAugment(freq_masks=1, freq_width=7, time_masks=3, time_width=20, time_ratio=0.5, warp=4, "
                    "fill='mean', seed=11)")
    post._keys(3, None)  # the state moves, the text does not
    assert repr(post) == text
    same = eval(text)
    assert repr(same) == text and same._seed == SpecAugment(seed=11)._seed
    assert repr(SpecAugment()) == repr(SpecAugment()) and "seed=None" in repr(SpecAugment())


def test_the_wrapper_and_the_stream_batches(monkeypatch):
    import torch

    from pydrobert_speech_amd.compute import FrameComputer
    from pydrobert_speech_amd.multistream import StreamBatch
    from pydrobert_speech_amd.multistream_si import SiStreamBatch
    from pydrobert_speech_amd.torch import PyTorchPostProcessorWrapper

    module = PyTorchPostProcessorWrapper.from_postprocessor(SpecAugment(seed=1))  # accepted as it is
    assert isinstance(module, torch.nn.Module) and isinstance(module.postprocessor, SpecAugment)
    # no stage of batched streaming: the classes have no argument for it, and under another stage's it is refused
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # (the refusal comes before any device is asked for)
    stft = alias_factory_subclass_from_arg(FrameComputer, {"name": "stft", "bank": "fbank", "use_log": False})
    si = alias_factory_subclass_from_arg(FrameComputer, {"name": "si", "bank": {"name": "fbank", "num_filts": 40},
                                                         "use_log": False})
    for cls, comp in ((StreamBatch, stft), (SiStreamBatch, si)):
        with pytest.raises(TypeError):
            cls(comp, capacity=4, specaugment=SpecAugment())
        for name in ("pcen", "cepstra", "sliding_cmvn"):
            for arg in (SpecAugment(), "specaugment", {"name": "specaug", "warp": 2}):
                with pytest.raises(ValueError, match=name):
                    cls(comp, capacity=4, **{name: arg})


# ---- 3. the fourth library's binding --------------------------------------------------------------------------------


def test_stages3_header_and_signature_table_name_the_same_set():
    with open(os.path.join(ROOT, "include", "pds_amd_stages3.h")) as fh:
        header = fh.read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = dict(re.findall(r"\b(pds_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code))
    assert set(declared) == set(_native.STAGES3_SIGNATURES), set(declared) ^ set(_native.STAGES3_SIGNATURES)
    assert {"pds_stages3_version", "pds_stages3_last_error"} <= set(declared)
    for name, args in declared.items():
        restype, argtypes = _native.STAGES3_SIGNATURES[name]
        count = 0 if args.strip() == "void" else len(args.split(","))
        assert count == len(argtypes), name
        if name != "pds_stages3_last_error":
            assert restype is ctypes.c_int32, name
    assert len(_native.STAGES3_SIGNATURES["pds_specaug_plan"][1]) == 12
    assert len(_native.STAGES3_SIGNATURES["pds_specaug_mean_rows_f32"][1]) == 8
    assert len(_native.STAGES3_SIGNATURES["pds_specaug_apply_rows_f64"][1]) == 15
    # it shares no header with the other libraries
    for other in ("pds_amd.h", "pds_amd_stages.h", "pds_amd_stages2.h", "pds_internal.h", "stages_internal.h",
                  "dither_noise.h", "pcen_rule.h"):
        assert f'"{other}"' not in header and f"/{other}" not in code
    csrc = os.path.join(ROOT, "pydrobert-speech_amd", "csrc")
    with open(os.path.join(csrc, "specaug.hip")) as fh:
        assert re.findall(r'#include\s+"([^"]+)"', fh.read()) == ["../../include/pds_amd_stages3.h", "specaug_rule.h"]
    with open(os.path.join(csrc, "specaug_rule.h")) as fh:
        assert re.findall(r'#include\s+"([^"]+)"', fh.read()) == []  # (what host and device share stands alone)


def test_the_definition_is_in_the_header_and_the_docstring_word_for_word():
    with open(os.path.join(ROOT, "include", "pds_amd_stages3.h"), encoding="utf-8") as fh:
        header = " ".join(re.sub(r"^\s*\*\s?", "", line) for line in fh.read().splitlines()).split()
    header = " ".join(header)
    doc = " ".join(SpecAugment.__doc__.split())
    start, end = "Per utterance of T ≥ 1 rows and C ≥ 1 columns with a 64-bit key k:", "T = 0 gives nothing."
    text = doc[doc.index(start): doc.index(end) + len(end)]
    assert len(text) > 2400 and text in header
    for phrase in ("`U(r, n) = (uint64(r) · uint64(n + 1)) >> 32` for 0 ≤ n < 2³¹", "`w1 = w0 − W + U(r1, 2W)`",
                   "`b = min(time_width, (int64) floor(time_ratio · (double) T))`, the product rounded once",
                   "`s = ((+0.0 + p_0) + p_1) + … + p_63`", "`i + 1 ≤ T − 1` whenever `a > 0`"):
        assert phrase in text, phrase


def test_stages3_library_exports_every_declared_symbol():
    lib = _native.stages3_lib()  # (NativeError if it was not built: there is no fallback)
    for name in _native.STAGES3_SIGNATURES:
        assert getattr(lib, name) is not None
    assert lib.pds_stages3_version() >= 100
    assert isinstance(lib.pds_stages3_last_error(), bytes)
    assert lib.pds_specaug_tile_rows() == post_module._SPECAUG_TILE
    # argument errors are reported before any HIP call, through the library's own error string
    plan = dict(B=2, C=4, F=2, fw=10, N=2, tw=50, ratio=1.0, warp=0)

    def call_plan(**kw):
        a = dict(plan, **kw)
        return lib.pds_specaug_plan(None, None, a["B"], a["C"], a["F"], a["fw"], a["N"], a["tw"], a["ratio"], a["warp"],
                                    None, None)

    assert call_plan() == -1 and b"null pointer" in lib.pds_stages3_last_error()
    assert call_plan(B=0) == 0
    for bad, word in (({"B": -1}, b"size"), ({"C": 0}, b"size"), ({"F": 17}, b"masks"), ({"N": -1}, b"masks"),
                      ({"fw": -1}, b"width"), ({"tw": (1 << 31) - 1}, b"width"), ({"ratio": 0.0}, b"time_ratio"),
                      ({"ratio": 1.5}, b"time_ratio"), ({"ratio": float("nan")}, b"time_ratio"),
                      ({"warp": -1}, b"warp"), ({"warp": (1 << 29) + 1}, b"warp")):
        assert call_plan(**bad) == -1 and word in lib.pds_stages3_last_error(), bad
        assert call_plan(B=0, **{k: v for k, v in bad.items() if k != "B"}) in (0, -1)
    assert lib.pds_specaug_mean_rows_f32(None, 4, None, None, 0, 4, None, None) == 0
    assert lib.pds_specaug_mean_rows_f32(None, 4, None, None, 2, 4, None, None) == -1
    assert b"null pointer" in lib.pds_stages3_last_error()
    assert lib.pds_specaug_mean_rows_f64(None, 3, None, None, 2, 4, None, None) == -1
    assert b"stride" in lib.pds_stages3_last_error()
    assert lib.pds_specaug_mean_rows_f64(None, 4, None, None, 2, 0, None, None) == -1

    def call_apply(fn=lib.pds_specaug_apply_rows_f32, in_stride=4, B=2, C=4, F=2, N=2, out_stride=4, max_rows=9):
        return fn(None, in_stride, None, None, B, C, None, F, N, None, 0.0, None, out_stride, max_rows, None)

    assert call_apply() == -1 and b"null pointer" in lib.pds_stages3_last_error()
    assert call_apply(B=0) == 0 and call_apply(max_rows=0) == 0
    assert call_apply(lib.pds_specaug_apply_rows_f64, in_stride=3) == -1 and b"stride" in lib.pds_stages3_last_error()
    assert call_apply(out_stride=3) == -1 and b"stride" in lib.pds_stages3_last_error()
    assert call_apply(F=17) == -1 and b"masks" in lib.pds_stages3_last_error()
    assert call_apply(N=-1) == -1 and call_apply(C=0) == -1 and call_apply(B=-1) == -1 and call_apply(max_rows=-1) == -1
    tile = lib.pds_specaug_tile_rows()
    assert call_apply(B=1 << 16, max_rows=tile * (1 << 15)) == -1 and b"too many blocks" in lib.pds_stages3_last_error()
    assert call_apply(B=1 << 16, max_rows=tile * ((1 << 15) - 1)) == -1 and b"null pointer" in lib.pds_stages3_last_error()
    with pytest.raises(ValueError, match="specaug_apply_rows"):
        _native.check_stages3(-1, "pds_specaug_apply_rows")
    with pytest.raises(_native.NativeError, match="code -2"):
        _native.check_stages3(-2, "pds_specaug_apply_rows")


def test_no_cpu_path_without_a_device(monkeypatch):
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    post = SpecAugment(seed=0)
    x = np.ones((10, 3), dtype=np.float32)
    for call in (lambda: post.apply(x), lambda: post.apply_rows(torch.ones(4, 3), [0, 4]),
                 lambda: post.mean_rows(torch.ones(4, 3), [0, 4]), lambda: post.plan_rows([4], 3)):
        with pytest.raises(_native.NativeError, match="no HIP device"):
            call()


# ---- 4. the packed calls over a fake native layer ---------------------------------------------------------------------


def _words(address, count):
    """`count` int64 words of host memory at `address`, copied"""
    return np.ctypeslib.as_array((ctypes.c_int64 * count).from_address(address)).copy()


class _FakeLib:
    """records the calls; its tensors are host memory, so the tables it is handed can be read"""

    def __init__(self):
        self.calls = []

    def pds_specaug_plan(self, d_nrows, d_keys, B, C, F, fw, N, tw, ratio, warp, d_plan, stream):
        self.calls.append(("plan", _words(d_nrows, B), _words(d_keys, B).view(np.uint64), B, C, (F, fw, N, tw, ratio, warp)))
        return 0

    def _mean(self, d_in, stride, d_row_off, d_nrows, B, C, d_mean, stream):
        self.calls.append(("mean", d_in, stride, _words(d_row_off, B), _words(d_nrows, B), B, C, d_mean))
        return 0

    def _apply(self, d_in, in_stride, d_row_off, d_nrows, B, C, d_plan, F, N, d_mean, fill, d_out, out_stride, max_rows,
               stream):
        self.calls.append(("apply", d_in, in_stride, _words(d_row_off, B), _words(d_nrows, B), B, C, d_plan, F, N, d_mean,
                           fill, d_out, out_stride, max_rows))
        return 0

    pds_specaug_mean_rows_f32 = pds_specaug_mean_rows_f64 = _mean
    pds_specaug_apply_rows_f32 = pds_specaug_apply_rows_f64 = _apply


@pytest.fixture
def fake(monkeypatch):
    import torch

    class FakeCuda:
        device = staticmethod(lambda device: contextlib.nullcontext())
        current_stream = staticmethod(lambda device=None: types.SimpleNamespace(cuda_stream=0))
        current_device = staticmethod(lambda: 0)

    class FakeTorch:
        cuda = FakeCuda

        def __getattr__(self, name):
            return getattr(torch, name)

    lib = _FakeLib()

    class Native:
        NativeError = _native.NativeError
        require_device = staticmethod(lambda: FakeTorch())
        stages3_lib = staticmethod(lambda: lib)

        @staticmethod
        def check_stages3(rc, what):
            assert rc == 0, what

    monkeypatch.setattr(post_module, "_native", Native)
    monkeypatch.setattr(post_module, "_is_gpu_tensor", lambda x: isinstance(x, torch.Tensor))
    return lib


def test_the_seed_sequence(fake):
    import torch

    post = SpecAugment(seed=5, warp=2)
    state = sm._seed_state(5)
    feats = torch.zeros((9, 4))
    post.apply_rows(feats, [0, 3, 3, 9])  # seeds=None: one step per utterance, in order, empty ones included
    want = []
    for _ in range(3):
        state = sm._next_key(state)
        want.append(state)
    kind, nrows, keys, B, C, args = fake.calls[0]
    assert kind == "plan" and keys.tolist() == want and nrows.tolist() == [3, 0, 6] and (B, C) == (3, 4)
    assert args == (2, 10, 2, 50, 1.0, 2) and post._seed == want[-1]
    assert keys[0] == sm.dither_keys([5])[0]  # the first apply of SpecAugment(seed=5)
    post.apply_rows(feats, [0, 3, 3, 9], seeds=[7, 8, 9])  # explicit seeds leave the sequence alone
    assert fake.calls[2][2].tolist() == sm.dither_keys([7, 8, 9]).tolist() and post._seed == want[-1]
    post.plan_rows([4, 5], 3, seeds=[1, 2], device="cpu")
    assert post._seed == want[-1] and fake.calls[-1][2].tolist() == sm.dither_keys([1, 2]).tolist()
    post.plan_rows([4, 5], 3, device="cpu")
    assert fake.calls[-1][2].tolist() == [sm._next_key(want[-1]), sm._next_key(sm._next_key(want[-1]))]
    assert post._seed == sm._next_key(sm._next_key(want[-1]))
    before, calls = post._seed, len(fake.calls)
    plan = torch.zeros((3, post.plan_words), dtype=torch.int64)
    post.apply_rows(feats, [0, 3, 3, 9], plan=plan)  # a given plan: no draw, no step
    assert post._seed == before and [c[0] for c in fake.calls[calls:]] == ["apply"]
    assert fake.calls[-1][7] == plan.data_ptr()
    with pytest.raises(ValueError, match="one seed per utterance"):
        post.apply_rows(feats, [0, 3, 3, 9], seeds=[1, 2])
    with pytest.raises(ValueError, match="one seed per utterance"):
        post.plan_rows([4, 5], 3, seeds=[1], device="cpu")


def test_the_launches_of_one_call(fake):
    import torch

    feats = torch.zeros((12, 8), dtype=torch.float64)[:, 2:7]  # a column slice: rows 8 apart
    rows = [1, 4, 4, 11]
    out = SpecAugment(fill="mean", seed=1).apply_rows(feats, rows)
    assert [c[0] for c in fake.calls] == ["plan", "mean", "apply"]
    _, d_in, stride, row_off, nrows, B, C, d_mean = fake.calls[1]
    assert (d_in, stride, B, C) == (feats.data_ptr(), 8, 3, 5) and row_off.tolist() == [1, 4, 4]
    call = fake.calls[2]
    assert call[1:3] == (feats.data_ptr(), 8) and call[3].tolist() == [1, 4, 4] and call[4].tolist() == [3, 0, 7]
    assert call[5:7] == (3, 5) and call[8:10] == (2, 2) and call[10] == d_mean and call[11] == 0.0
    assert call[12:] == (out.data_ptr(), 5, 7)  # the longest utterance's rows
    fake.calls.clear()
    SpecAugment(fill=-2.5, seed=1, freq_masks=0).apply_rows(feats, rows, out=feats)  # in place without a warp
    assert [c[0] for c in fake.calls] == ["plan", "apply"]
    call = fake.calls[1]
    assert call[10] is None and call[11] == -2.5 and call[12] == feats.data_ptr() and call[13] == 8 and call[8] == 0
    fake.calls.clear()
    for empty in ([0], [3, 3], [0, 0, 0]):
        SpecAugment(seed=1).apply_rows(feats, empty)
    assert fake.calls == []


def test_apply_rows_refusals(fake):
    import torch

    feats = torch.zeros((9, 4))
    warped, plain = SpecAugment(warp=1, seed=0), SpecAugment(seed=0)
    with pytest.raises(ValueError, match="out is feats under warp"):
        warped.apply_rows(feats, [0, 9], out=feats)
    with pytest.raises(ValueError, match="shares feats' memory"):
        warped.apply_rows(feats, [0, 9], out=feats[:])
    plain.apply_rows(feats, [0, 9], out=feats)  # allowed where warp == 0
    plan = torch.zeros((1, 10), dtype=torch.int64)
    for post in (warped, plain):
        with pytest.raises(ValueError, match="plan and seeds"):
            post.apply_rows(feats, [0, 9], seeds=[3], plan=plan)
    for bad in (torch.zeros((2, 10), dtype=torch.int64), torch.zeros((1, 8), dtype=torch.int64),
                torch.zeros((1, 10), dtype=torch.int32), np.zeros((1, 10), dtype=np.int64),
                torch.zeros((1, 20), dtype=torch.int64)[:, ::2]):
        with pytest.raises(ValueError, match="plan must be"):
            plain.apply_rows(feats, [0, 9], plan=bad)
    with pytest.raises(ValueError, match="row_offsets"):
        plain.apply_rows(feats, [0, 10])
    with pytest.raises(ValueError, match="row_offsets"):
        plain.apply_rows(feats, [4, 2])
    with pytest.raises(ValueError, match="2-D float32 or float64"):
        plain.apply_rows(feats.to(torch.float16), [0, 9])
    with pytest.raises(ValueError, match="out must be"):
        plain.apply_rows(feats, [0, 9], out=torch.zeros((9, 5)))
    with pytest.raises(ValueError, match="out must be"):
        plain.apply_rows(feats, [0, 9], out=torch.zeros((9, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match="in_place under warp"):
        warped.apply(np.zeros((9, 4), dtype=np.float32), in_place=True)
    with pytest.raises(ValueError, match="row count"):
        plain.plan_rows([1 << 31], 4, device="cpu")
    with pytest.raises(ValueError, match="row count"):
        plain.plan_rows([-1], 4, device="cpu")
    for C in (0, -3, 1 << 31, 4.0, True):
        with pytest.raises(ValueError, match="C must be"):
            plain.plan_rows([5], C, device="cpu")


def test_spans_cover_the_batch_within_the_limit():
    tile = post_module._SPECAUG_TILE
    spans = post_module._specaug_spans
    assert spans([]) == [] and spans([0, 0]) == [(0, 2, 0)] and spans([5, 0, 70]) == [(0, 3, 70)]
    rng = np.random.default_rng(0)
    for limit in (1, 2, 7, 50):
        for _ in range(30):
            nrows = rng.integers(0, limit * tile + 1, rng.integers(1, 40)).tolist()
            got = spans(nrows, limit)
            assert [s[0] for s in got] == [0] + [s[1] for s in got[:-1]] and got[-1][1] == len(nrows)  # in order, whole
            for k, (lo, hi, longest) in enumerate(got):
                assert hi > lo and longest == max(nrows[lo:hi])
                assert (hi - lo) * -(-longest // tile) <= limit
                if hi < len(nrows):  # greedy: the next utterance would not have fitted
                    assert (hi + 1 - lo) * -(-max(nrows[lo:hi + 1]) // tile) > limit
    # at the real limit: 2^31 - 1 utterances of one tile fit one launch, one more does not
    assert post_module._SPECAUG_MAX_BLOCKS == (1 << 31) - 1
    assert spans([(1 << 31) - 1]) == [(0, 1, (1 << 31) - 1)]


def test_an_oversized_batch_is_split(fake, monkeypatch):
    import torch

    tile = post_module._SPECAUG_TILE
    monkeypatch.setattr(post_module, "_SPECAUG_MAX_BLOCKS", 7)
    nrows = [1, 2, 3, 0, tile + 1, 2, 3 * tile, 1, 1, 7 * tile, 1, 2, 3, 1, 2, 3, 1, 2]
    rows = np.concatenate([[0], np.cumsum(nrows)])
    feats = torch.zeros((int(rows[-1]), 4))
    post = SpecAugment(fill="mean", seed=2, freq_masks=1, time_masks=3)
    out = post.apply_rows(feats, rows)
    kinds = [c[0] for c in fake.calls]
    assert kinds[:2] == ["plan", "mean"] and set(kinds[2:]) == {"apply"} and len(kinds) > 3  # one plan, one mean
    plan_ptr, mean_ptr = None, fake.calls[1][7]
    lo = 0
    for call in fake.calls[2:]:
        _, d_in, in_stride, row_off, counts, B, C, d_plan, F, N, d_mean, fill, d_out, out_stride, max_rows = call
        assert (d_in, in_stride, C, F, N, d_out, out_stride) == (feats.data_ptr(), 4, 4, 1, 3, out.data_ptr(), 4)
        assert counts.tolist() == nrows[lo:lo + B] and row_off.tolist() == rows[lo:lo + B].tolist()
        assert max_rows == max(nrows[lo:lo + B]) and B * -(-max_rows // tile) <= 7
        plan_ptr = d_plan if plan_ptr is None else plan_ptr
        assert d_plan == plan_ptr + 8 * post.plan_words * lo and d_mean == mean_ptr + 8 * lo
        lo += B
    assert lo == len(nrows)
