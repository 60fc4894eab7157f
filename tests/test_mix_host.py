"""``pre.AddNoise`` on the host (no GPU): every refusal, each before the device is touched; alias and JSON
construction and ``__repr__``; the plan (deterministic, the same alone and at any index of a batch, in range over
10,000 seeds, ``lo == hi``, ``prob`` 0 and 1) against the numpy model of the definition (tests/mix_model.py); the
model's own signal-to-noise ratio; the definition word for word in the class, the header and DESIGN.md; the sixth
library's binding."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from pydrobert_speech_amd import _native
from pydrobert_speech_amd import pre as pre_module
from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg
from pydrobert_speech_amd.pre import AddNoise, NoisePlan, PreProcessor, dither_keys
from tests import mix_model as mm
from tests.conftest import ROOT


def _clips(lengths=(5, 16385, 2), dtype=np.float32, seed=0):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.int16:
        return [rng.integers(-3000, 3000, n).astype(np.int16) for n in lengths]
    return [rng.standard_normal(n).astype(dtype) for n in lengths]


# ---- 1. construction -----------------------------------------------------------------------------------------------


def test_aliases_json_and_repr(tmp_path):
    clips = _clips()
    for alias in ("add_noise", "additive_noise", "mix_noise"):
        got = alias_factory_subclass_from_arg(PreProcessor, {"name": alias, "clips": clips, "snr_db": [0, 15]})
        assert type(got) is AddNoise and got.snr_db == (0.0, 15.0) and got.prob == 1.0 and got.num_clips == 3
    np.save(tmp_path / "n1.npy", clips[0])
    np.savez(tmp_path / "n2.npz", clips[1])
    import torch

    torch.save(torch.from_numpy(clips[2]), tmp_path / "n3.pt")
    cfg = {"name": "add_noise", "clips": [str(tmp_path / "n1.npy"), str(tmp_path / "n2.npz"), str(tmp_path / "n3.pt")],
           "snr_db": 10, "prob": 0.5, "seed": 3}
    read = alias_factory_subclass_from_arg(PreProcessor, cfg)
    assert read.snr_db == (10.0, 10.0) and read.prob == 0.5 and read.seed == 3
    assert read.bank.dtype == np.float32 and np.array_equal(read.bank, np.concatenate(clips))
    assert read.clip_lengths.tolist() == [5, 16385, 2] and read.clip_offsets.tolist() == [0, 5, 16390]
    assert repr(read) == "AddNoise(clips=<3 of float32>, snr_db=(10.0, 10.0), prob=0.5, seed=3)"
    assert "0x" not in repr(read) and str(tmp_path) not in repr(read)
    mixed = AddNoise([clips[0], torch.from_numpy(clips[1])])  # arrays and tensors side by side
    assert mixed.num_clips == 2 and mixed.snr_db == (5.0, 20.0) and mixed.seed is None
    assert AddNoise(_clips(dtype=np.int16)).bank.dtype == np.int16  # PCM stays at two bytes a sample
    assert AddNoise(_clips(dtype=np.float64)).bank.dtype == np.float64


@pytest.mark.parametrize("snr_db", [(3.0, 2.0), (0.0, float("inf")), float("nan"), (1.0,), (1.0, 2.0, 3.0), "loud",
                                    None, (float("nan"), 1.0), True, (False, 3)])
def test_a_bad_snr_is_refused(snr_db):
    with pytest.raises(ValueError, match="snr_db"):
        AddNoise(_clips(), snr_db=snr_db)


@pytest.mark.parametrize("prob", [-0.1, 1.5, float("nan"), "often", None, True])
def test_a_bad_prob_is_refused(prob):
    with pytest.raises(ValueError, match="prob"):
        AddNoise(_clips(), prob=prob)


def test_bad_banks_are_refused(tmp_path):
    with pytest.raises(ValueError, match="empty"):
        AddNoise([])
    with pytest.raises(ValueError, match="clip 1 is empty"):
        AddNoise([np.ones(3, np.float32), np.ones(0, np.float32)])
    with pytest.raises(ValueError, match="mixed dtypes"):
        AddNoise([np.ones(3, np.float32), np.ones(3, np.float64)])
    with pytest.raises(ValueError, match="mixed dtypes"):
        AddNoise([np.ones(3, np.int16), np.ones(3, np.float32)])
    with pytest.raises(ValueError, match="float32, float64 or int16"):
        AddNoise([np.ones(3, np.int32)])
    with pytest.raises(ValueError, match="1-D"):
        AddNoise([np.ones((2, 3), np.float32)])
    with pytest.raises(ValueError, match="sequence"):
        AddNoise(np.ones(3, np.float32))
    with pytest.raises(ValueError, match="sequence"):
        AddNoise("noise.wav")
    np.save(tmp_path / "empty.npy", np.zeros(0, np.float32))
    with pytest.raises(ValueError, match="clip 0 is empty"):
        AddNoise([str(tmp_path / "empty.npy")])


# ---- 2. refusals of the calls, before the device is touched --------------------------------------------------------


@pytest.fixture
def no_device(monkeypatch):
    """CPU tensors pass for GPU tensors, and any step towards the device is an error"""
    import torch

    def touched(*args, **kwargs):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(pre_module, "_is_gpu_tensor", lambda x: isinstance(x, torch.Tensor))
    monkeypatch.setattr(_native, "require_device", touched)
    monkeypatch.setattr(_native, "stages5_lib", touched)
    return torch


def test_signals_that_are_refused(no_device):
    torch = no_device
    an = AddNoise(_clips(), seed=1)
    before = an._seed
    for call in (an.apply_packed, an.energy_packed):
        with pytest.raises(ValueError, match="1-D GPU tensor"):
            call(np.zeros(8, np.float32), [0], [8])
        with pytest.raises(ValueError, match="1-D GPU tensor"):
            call(torch.zeros((2, 4)), [0], [8])
        for dtype in (torch.float16, torch.int32, torch.int64, torch.uint8):
            with pytest.raises(ValueError, match="float32, float64 or int16"):
                call(torch.zeros(8, dtype=dtype), [0], [8])
        with pytest.raises(ValueError, match="one offset per length"):
            call(torch.zeros(8), [0, 4], [8])
        for offs, lens in (([0], [9]), ([-1], [4]), ([4], [-1]), ([0, 6], [4, 3])):
            with pytest.raises(ValueError, match="outside signal"):
                call(torch.zeros(8), offs, lens)
    with pytest.raises(ValueError, match="one seed per utterance"):
        an.apply_packed(torch.zeros(8), [0, 4], [4, 4], seeds=[1])
    assert an._seed == before  # (no refusal has advanced the sequence)


def test_a_gpu_less_tensor_is_refused_without_the_patch():
    import torch

    with pytest.raises(ValueError, match="1-D GPU tensor"):
        AddNoise(_clips()).apply_packed(torch.zeros(8), [0], [8])


def test_plans_that_are_refused(no_device):
    torch = no_device
    an = AddNoise(_clips((5, 16385, 2)), seed=1)
    x = torch.zeros(8)
    good = an.plan(2, seeds=[1, 2])
    with pytest.raises(ValueError, match="not one of 2 utterances"):
        an.apply_packed(x, [0, 4], [4, 4], plan=an.plan(3, seeds=[1, 2, 3]))
    with pytest.raises(ValueError, match="not one of 2 utterances"):
        an.apply_packed(x, [0, 4], [4, 4], plan=good._replace(ratio=good.ratio[:1]))
    for bad in (-1, 3):
        with pytest.raises(ValueError, match="clip outside"):
            an.apply_packed(x, [0, 4], [4, 4], plan=good._replace(clip=np.array([0, bad])))
    for clip, start in ((0, 5), (2, 2), (1, 16385), (0, -1)):
        with pytest.raises(ValueError, match="start outside its clip"):
            an.apply_packed(x, [0, 4], [4, 4], plan=good._replace(clip=np.array([0, clip]), start=np.array([0, start])))
    with pytest.raises(ValueError, match="integers"):
        an.apply_packed(x, [0, 4], [4, 4], plan=good._replace(start=np.array([0.0, 1.0])))
    with pytest.raises(ValueError, match="plan must hold"):
        an.apply_packed(x, [0, 4], [4, 4], plan=(good.clip, good.start))
    # the plan() call's own arguments
    with pytest.raises(ValueError, match="one seed per utterance"):
        an.plan(2, seeds=[1])
    with pytest.raises(ValueError, match="non-negative integer"):
        an.plan(-1)
    with pytest.raises(ValueError, match="one clip index per utterance"):
        an.plan(2, seeds=[1, 2], clips=[0])
    with pytest.raises(ValueError, match=r"outside \[0, 3\)"):
        an.plan(2, seeds=[1, 2], clips=[0, 3])
    with pytest.raises(ValueError, match="one finite value per utterance"):
        an.plan(2, seeds=[1, 2], snr_db=[1.0, float("nan")])


class _FakeSignal:
    """a signal of any length that takes no memory: what the size checks look at and nothing else"""

    is_cuda = True

    def __init__(self, n):
        import torch

        self._n, self.dtype = n, torch.float32

    def dim(self):
        return 1

    def numel(self):
        return self._n


def test_a_batch_of_too_many_blocks_is_refused(monkeypatch):
    def touched(*args, **kwargs):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_native, "require_device", touched)
    an = AddNoise(_clips(), seed=1)
    tile = 4096
    # the apply kernel: 65535 utterances of 32769 blocks each are more than 2^31 - 1 blocks in one launch
    n = 32768 * tile + 1
    B = 65535
    offs = np.arange(B, dtype=np.int64) * n
    with pytest.raises(ValueError, match="more than 2\\^31 - 1 blocks in one launch of the apply kernel"):
        an.apply_packed(_FakeSignal(B * n), offs, np.full(B, n), plan=NoisePlan(*(np.zeros(B, dtype=t) for t in (
            np.int64, np.int64, np.float64, np.float64, bool))))
    # ... and what passes that check goes on to the device (which the patch turns into an error of another kind)
    n = 32768 * tile - 3
    with pytest.raises(AssertionError, match="the device was touched"):
        an.apply_packed(_FakeSignal(B * n), np.arange(B, dtype=np.int64) * n, np.full(B, n), plan=NoisePlan(*(
            np.zeros(B, dtype=t) for t in (np.int64, np.int64, np.float64, np.float64, bool))))
    # the energy kernel: four chunks of 16384 samples a block
    n = 16384 * 4 * (1 << 31)
    with pytest.raises(ValueError, match="more than 2\\^31 - 1 blocks in one launch of the energy kernel"):
        an.energy_packed(_FakeSignal(n), [0], [n])
    with pytest.raises(AssertionError, match="the device was touched"):
        an.energy_packed(_FakeSignal(n), [0], [n - 16384 * 4])


# ---- 3. the plan ---------------------------------------------------------------------------------------------------


def _as_dict(plan):
    return {name: getattr(plan, name) for name in ("clip", "start", "snr_db", "ratio", "applied")}


def _same_plan(a, b):
    a, b = (_as_dict(p) if isinstance(p, NoisePlan) else p for p in (a, b))
    for name in ("clip", "start", "applied"):
        assert np.array_equal(a[name], b[name]), name
    for name in ("snr_db", "ratio"):  # bit for bit
        assert a[name].dtype == np.float64 and a[name].tobytes() == np.asarray(b[name], dtype=np.float64).tobytes(), name


def test_the_plan_is_the_models_and_deterministic():
    lengths = (5, 16385, 2, 77)
    an = AddNoise(_clips(lengths), snr_db=(-3.5, 17.25), prob=0.6, seed=11)
    seeds = list(range(100, 164))
    got = an.plan(64, seeds=seeds)
    assert isinstance(got, NoisePlan) and got.clip.dtype == np.int64 and got.start.dtype == np.int64
    assert got.applied.dtype == bool and got.ratio.dtype == np.float64
    _same_plan(got, mm.plan(dither_keys(seeds), lengths, (-3.5, 17.25), 0.6))
    _same_plan(got, an.plan(64, seeds=seeds))  # the same seeds, the same plan
    assert 0 < got.applied.sum() < 64 and len(set(got.clip.tolist())) == 4
    # an utterance's plan is the same alone and at any index of a batch
    alone = an.plan(1, seeds=[seeds[37]])
    other = an.plan(5, seeds=[7, 8, seeds[37], 9, 10])
    for name in NoisePlan._fields:
        assert getattr(alone, name)[0] == getattr(got, name)[37] == getattr(other, name)[2], name
    # explicit seeds leave the object's own sequence alone; seeds=None advances it once per utterance
    state = pre_module._seed_state(11)
    assert an._seed == state
    keys = []
    for _ in range(5):
        state = pre_module._next_key(state)
        keys.append(state)
    own = an.plan(5)
    assert an._seed == keys[-1]
    _same_plan(own, mm.plan(keys, lengths, (-3.5, 17.25), 0.6))
    assert keys[0] == int(dither_keys([11])[0])  # the first utterance of AddNoise(seed=11): the package's one seed rule
    an.plan(0)
    assert an._seed == keys[-1]
    empty = an.plan(0, seeds=[])
    assert all(len(v) == 0 for v in empty)


def test_overrides_take_the_place_of_the_draws():
    lengths = (5, 16385, 2)
    an = AddNoise(_clips(lengths), snr_db=(0.0, 10.0), seed=2)
    seeds = list(range(40))
    clips = np.arange(40) % 3
    snrs = np.linspace(-5.0, 25.0, 40)
    got = an.plan(40, seeds=seeds, clips=clips, snr_db=snrs)
    _same_plan(got, mm.plan(dither_keys(seeds), lengths, (0.0, 10.0), 1.0, clips=clips, snrs=snrs))
    assert np.array_equal(got.clip, clips) and got.snr_db.tobytes() == snrs.tobytes()
    assert (got.start < np.asarray(lengths)[clips]).all() and (got.start >= 0).all()  # drawn against the chosen clip
    drawn = an.plan(40, seeds=seeds)
    assert not np.array_equal(drawn.clip, clips)


@pytest.fixture(scope="module")
def many_keys():
    return dither_keys(range(10000))


@pytest.mark.parametrize("K", [1, 3, 7])
def test_draws_stay_in_range_over_ten_thousand_seeds(many_keys, K):
    lengths = [(1, 2, 16385)[k % 3] for k in range(K)]
    an = AddNoise([np.ones(n, np.float32) for n in lengths], snr_db=(-2.0, 31.0), prob=0.25)
    x0, x1, x2, x3 = pre_module._philox_draws(many_keys, pre_module._MIX_COUNTER)
    clip = pre_module._mix_pick(x0, np.uint64(K))
    plan = an.plan(10000, seeds=range(10000))
    assert np.array_equal(plan.clip, clip)
    assert plan.clip.min() == 0 and plan.clip.max() == K - 1
    assert (plan.start >= 0).all() and (plan.start < np.asarray(lengths)[plan.clip]).all()
    for j, n in enumerate(lengths):
        starts = plan.start[plan.clip == j]
        assert starts.max() == n - 1 if n < 100 else starts.max() > 0.99 * n  # (every position of a short clip is met)
    assert (plan.snr_db >= -2.0).all() and (plan.snr_db <= 31.0).all() and plan.snr_db.std() > 5
    assert 0.2 < plan.applied.mean() < 0.3
    assert plan.ratio.tolist() == [math.pow(10.0, v / 10.0) for v in plan.snr_db.tolist()]  # one scalar call each
    # the largest words give the largest indices
    top = np.array([0xFFFFFFFF], dtype=np.uint64)
    assert pre_module._mix_pick(top, np.uint64(K))[0] == K - 1
    for n in (1, 2, 16385, 1 << 32):
        assert pre_module._mix_pick(top, np.uint64(n))[0] == n - 1
    # a first spot check of the vectorised draws against the model's integers
    for b in (0, 1, 9999):
        assert [int(x[b]) for x in (x0, x1, x2, x3)] == mm.philox4x32_10(mm.COUNTER, many_keys[b])


def test_equal_bounds_and_the_two_ends_of_prob():
    for lo in (-5.0, 0.0, 7.3, 12.000000000000002):
        plan = AddNoise(_clips(), snr_db=lo).plan(500, seeds=range(500))
        assert (plan.snr_db == lo).all() and plan.snr_db.tobytes() == np.full(500, lo).tobytes()
        assert (plan.ratio == 10.0 ** (lo / 10.0)).all()
    assert not AddNoise(_clips(), prob=0.0).plan(2000, seeds=range(2000)).applied.any()
    assert AddNoise(_clips(), prob=1.0).plan(2000, seeds=range(2000)).applied.all()


def test_philox_known_answers_of_the_model():
    # Random123's kat_vectors for philox4x32-10
    assert mm.philox4x32_10((0, 0, 0, 0), 0) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert mm.philox4x32_10((0xFFFFFFFF,) * 4, (1 << 64) - 1) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert mm.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), 0x299F31D0A4093822) == [
        0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    # the counter is in the header, and it is none the dither or SpecAugment can form (their fourth word is zero)
    with open(os.path.join(ROOT, "pydrobert-speech_amd", "csrc", "mix_rule.h")) as fh:
        rule = fh.read()
    assert "MIX_COUNTER_3 = 0x4D495831u" in rule and mm.COUNTER == pre_module._MIX_COUNTER == (0, 0, 0, 0x4D495831)


# ---- 4. the model --------------------------------------------------------------------------------------------------


def test_the_models_two_energies_agree():
    rng = np.random.default_rng(3)
    for n in (1, 63, 64, 65, 16385):
        X = rng.standard_normal((3, n)).astype(np.float32)
        rows = mm.energy_rows(X)
        assert rows.tobytes() == np.asarray([mm.energy(x) for x in X]).tobytes()
        assert np.allclose(rows, (X.astype(np.float64) ** 2).sum(1), rtol=1e-12)
    assert mm.energy(np.zeros(0, np.float32)) == 0.0 and mm.power(np.zeros(0, np.float32)) == 0.0


def test_the_model_reaches_the_requested_snr():
    """float64 data, an utterance exactly as long as its clip: every clip sample is used once, so Pn is the power
    actually added, and the ratio measured from y - x is the requested one but for the roundings of g and of the sums
    (a few parts in 1e16 of each, far inside 1e-9 dB)"""
    rng = np.random.default_rng(4)
    for n, snr in ((1000, 0.0), (16385, 12.5), (40000, -3.0), (777, 20.0)):
        x = rng.standard_normal(n) * 37.0
        clip = rng.standard_normal(n) * 0.2
        keys = dither_keys([5])
        plan = mm.plan(keys, [n], (snr, snr), 1.0)
        out, g = mm.apply_packed(x, [0], [n], [clip], plan)
        assert g[0] > 0 and out.dtype == np.float64
        noise = out - x
        measured = 10.0 * np.log10(np.sum(x * x) / np.sum(noise * noise))
        print(f"n = {n}, requested {snr} dB, measured {measured!r} dB")
        assert abs(measured - snr) < 1e-9
        start = int(plan["start"][0])
        assert np.allclose(noise, g[0] * np.roll(clip, -start), rtol=0, atol=1e-12 * np.abs(x).max())


def test_the_models_zero_gain_is_a_copy():
    x = np.array([1.0, -0.0, np.nan, 3.0], dtype=np.float32)
    x.view(np.uint32)[2] = 0x7FC01234  # a NaN with a payload
    got = mm.mix(x, np.ones(3, np.float32), 1, np.float64(0.0))
    assert got.tobytes() == x.tobytes()
    assert mm.gain(np.float64("nan"), 1.0, 1.0, True) == 0.0 and mm.gain(1.0, np.float64("nan"), 1.0, True) == 0.0
    assert mm.gain(0.0, 1.0, 1.0, True) == 0.0 and mm.gain(1.0, 0.0, 1.0, True) == 0.0
    assert mm.gain(1.0, 1.0, 1.0, False) == 0.0 and mm.gain(4.0, 1.0, 1.0, True) == 2.0
    pcm = np.array([5, -7, 0], dtype=np.int16)
    assert mm.mix(pcm, np.ones(3, np.int16), 0, np.float64(0.0)).tobytes() == np.array([5, -7, 0], np.float32).tobytes()


# ---- 5. the definition and the sixth library's binding --------------------------------------------------------------


def _definition(text):
    text = " ".join(text.split())
    start, end = "Segment energy `E(x, n)` of `n` samples, float64:", "is only promised not to disturb other utterances."
    return text[text.index(start): text.index(end) + len(end)]


def test_the_definition_is_in_the_docstring_the_header_and_the_design_word_for_word():
    doc = _definition(AddNoise.__doc__)
    assert len(doc) > 2000
    with open(os.path.join(ROOT, "include", "pds_amd_stages5.h")) as fh:
        header = "\n".join(re.sub(r"^\s*\*\s?", "", line) for line in fh.read().splitlines())
    assert _definition(header) == doc
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        design = fh.read()
    assert "4.12" in design and _definition(design[design.index("### 4.12"):]) == doc


def test_stages5_header_and_signature_table_name_the_same_set():
    with open(os.path.join(ROOT, "include", "pds_amd_stages5.h")) as fh:
        header = fh.read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = dict(re.findall(r"\b(pds_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code))
    assert set(declared) == set(_native.STAGES5_SIGNATURES), set(declared) ^ set(_native.STAGES5_SIGNATURES)
    applies = {f"pds_mix_apply_{x}_{z}" for x in ("f32", "f64", "i16") for z in ("f32", "f64", "i16")}
    assert {"pds_stages5_version", "pds_stages5_last_error", "pds_mix_gain", "pds_mix_chunk_energy_f32",
            "pds_mix_chunk_energy_f64", "pds_mix_chunk_energy_i16"} | applies <= set(declared)
    for name, args in declared.items():
        restype, argtypes = _native.STAGES5_SIGNATURES[name]
        count = 0 if args.strip() == "void" else len(args.split(","))
        assert count == len(argtypes), name
    assert len(_native.STAGES5_SIGNATURES["pds_mix_apply_f32_f32"][1]) == 12
    assert _native.STAGES5_SIGNATURES["pds_mix_gain"][0] is ctypes.c_int32
    assert _native.STAGES5_SIGNATURES["pds_mix_chunk_count"][0] is ctypes.c_int64
    # it shares no header with the other libraries
    for other in ("pds_amd.h", "pds_amd_stages.h", "pds_amd_stages2.h", "pds_amd_stages3.h", "pds_amd_stages4.h",
                  "pds_internal.h", "stages_internal.h"):
        assert f'"{other}"' not in header and f"/{other}" not in code


def test_mix_hip_includes_its_header_and_the_rule_and_nothing_else_of_the_project():
    csrc = os.path.join(ROOT, "pydrobert-speech_amd", "csrc")
    with open(os.path.join(csrc, "mix.hip")) as fh:
        includes = re.findall(r'#include\s+"([^"]+)"', fh.read())
    assert includes == ["../../include/pds_amd_stages5.h", "mix_rule.h"]
    users = []
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")) and name != "mix_rule.h":
            with open(os.path.join(csrc, name)) as fh:
                if "mix_rule.h" in re.findall(r'#include\s+"([^"]+)"', fh.read()):
                    users.append(name)
    assert users == ["mix.hip"]
    with open(os.path.join(csrc, "mix_rule.h")) as fh:
        assert re.findall(r'#include\s+"([^"]+)"', fh.read()) == []
    with open(os.path.join(csrc, "Makefile")) as fh:
        make = fh.read()
    assert "STAGES5_LIB  = libpds_amd_stages5.so" in make and "STAGES5_OBJS = mix.o" in make
    assert re.search(r"^all:.*\$\(STAGES5_LIB\)", make, flags=re.M)
    command = subprocess.run(["make", "-n", "-B", "mix.o"], cwd=csrc, check=True, capture_output=True, text=True).stdout
    assert "mix.hip" in command and "-ffp-contract=off" in command
    assert "STAGES4_OBJS = plp.o\n" in make  # the fifth library keeps the PLP kernels and no other
    with open(os.path.join(csrc, "pre.hip")) as fh:
        assert "mix" not in fh.read()  # nothing of it went into the first library


def test_stages5_library_exports_every_declared_symbol_and_reports_argument_errors():
    lib = _native.stages5_lib()  # (NativeError if it was not built: there is no fallback)
    for name in _native.STAGES5_SIGNATURES:
        assert getattr(lib, name) is not None
    assert lib.pds_stages5_version() >= 100
    assert isinstance(lib.pds_stages5_last_error(), bytes)
    assert lib.pds_mix_chunk_samples() == 16384 == pre_module._MIX_CHUNK
    assert lib.pds_mix_tile_samples() == 4096 == pre_module._MIX_TILE
    lengths = [-3, 0, 1, 16383, 16384, 16385, 32769, 1 << 40]
    assert [lib.pds_mix_chunk_count(n) for n in lengths] == pre_module._mix_chunks(lengths).tolist()
    assert [lib.pds_mix_chunk_count(n) for n in lengths] == [0, 0, 1, 1, 1, 2, 3, 1 << 26]
    err = lib.pds_stages5_last_error
    # argument errors are reported before any HIP call, through the library's own error string: these run without a
    # device
    for fn in (lib.pds_mix_chunk_energy_f32, lib.pds_mix_chunk_energy_f64, lib.pds_mix_chunk_energy_i16):
        assert fn(None, None, None, None, 1, 1, None, None) == -1 and b"null pointer" in err()
        assert fn(None, None, None, None, 0, 0, None, None) == 0 and fn(None, None, None, None, 3, 0, None, None) == 0
        assert fn(None, None, None, None, -1, 1, None, None) == -1 and b"bad size" in err()
        assert fn(None, None, None, None, 1, -1, None, None) == -1 and b"bad size" in err()
        most = 4 * ((1 << 31) - 1)
        assert fn(None, None, None, None, 1, most + 1, None, None) == -1 and b"2^31 - 1 blocks" in err()
        assert fn(None, None, None, None, 1, most, None, None) == -1 and b"null pointer" in err()
    gain = lib.pds_mix_gain
    assert gain(None, None, None, 0, 2, None, None, None, None, 0, None, None) == 0
    assert gain(None, None, None, 1, 0, None, None, None, None, 0, None, None) == -1 and b"null pointer" in err()
    assert gain(None, None, None, -1, 0, None, None, None, None, 0, None, None) == -1 and b"bad size" in err()
    for mode in (-1, 3):
        assert gain(None, None, None, 1, mode, None, None, None, None, 0, None, None) == -1 and b"mode" in err()
    for x in ("f32", "f64", "i16"):
        for z in ("f32", "f64", "i16"):
            fn = getattr(lib, f"pds_mix_apply_{x}_{z}")
            none = (None,) * 8
            assert fn(*none, 1, 10, None, None) == -1 and b"null pointer" in err()
            assert fn(*none, 0, 10, None, None) == 0 and fn(*none, 5, 0, None, None) == 0
            assert fn(*none, -1, 10, None, None) == -1 and b"bad size" in err()
            assert fn(*none, 1, -1, None, None) == -1 and b"bad size" in err()
            assert fn(*none, 65536, 10, None, None) == -1 and b"65535 utterances" in err()
            assert fn(*none, 65535, 32768 * 4096 + 1, None, None) == -1 and b"2^31 - 1 blocks" in err()
            assert fn(*none, 65535, 32768 * 4096 - 3, None, None) == -1 and b"null pointer" in err()
    with pytest.raises(ValueError, match="pds_mix_apply"):
        _native.check_stages5(-1, "pds_mix_apply")
    with pytest.raises(_native.NativeError, match="code -2"):
        _native.check_stages5(-2, "pds_mix_apply")


def test_no_cpu_path_without_a_device(monkeypatch):
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    an = AddNoise(_clips())
    with pytest.raises(_native.NativeError, match="no CPU fallback"):
        an.apply(np.zeros(100, np.float32))
    with pytest.raises(_native.NativeError, match="no CPU fallback"):
        an.clip_power()


def test_the_command_line_tool_takes_the_stage(tmp_path):
    from pydrobert_speech_amd import command_line as cl

    an = AddNoise(_clips())
    writer = cl.FeatureDirWriter(None, [an], [], str(tmp_path / "out"), seed=4)
    assert writer.pre == [an] and writer.seeded
    assert not cl.FeatureDirWriter(None, [an], [], str(tmp_path / "out"), seed=4, seeded=False).seeded
    assert "add_noise" in cl.__doc__ and "AddNoise.apply_packed" in cl.__doc__
    got = cl._as_list([{"name": "add_noise", "clips": _clips(), "snr_db": [0, 15]}, "dither"], PreProcessor)
    assert [type(p).__name__ for p in got] == ["AddNoise", "Dither"]
