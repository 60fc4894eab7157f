"""STFT parity on structured signals -- tones, DC, Nyquist, chirps, steps, clipped audio, levels from 1e-3 to 1e7,
the log floor straddled, non-finite samples -- through every kernel form, under the float32 error model of
tests/structured.py (read its docstring first).

Every other GPU parity test feeds white noise at amplitude 3000, which cannot see a wrong DC or Nyquist bin, a
low-accuracy twiddle or anything 40 dB below the frame's peak.  Here each (configuration, flow) packs all families
and levels into one ragged batch: one utterance of 12 S + L samples per family, and the same utterances again at
odd sample offsets so that frames do not start on the kernels' row boundaries.  One or two launches per case.

What is allowed: an element passes the suite's strict rule (1e-5 + 1e-4 |ref|; 1e-9 for float64 arithmetic) or the
model's bound with kappa = MARGIN * KAPPA_REF = 4 x what numpy's float32 rFFT needs on the same signals
(structured.KAPPA_REF, measured on the CPU, asserted by test_structured_model.py), about one float32 eps of the
frame's peak amplitude per bin.  The direct-DFT kernel is held to 4 x KAPPA_REF_DFT (a float32 DFT-matrix product's
need: its sums are up to 1024 terms long), float64 arithmetic to 2 x 4 x KAPPA_REF at eps = 2^-53 (the oracle's own
rounding is as large as the kernel's).  No form has a margin of its own.

With PDS_STRUCTURED_REPORT=<file> in the environment every comparison appends one line there (configuration, flow,
family, the largest kappa the kernel needed, elements that passed only through the bound):
profiles/r5a_structured_parity.txt is such a file.
"""
import json
import os

import numpy as np
import pytest

from oracle import stft_oracle as orc
from pydrobert_speech_amd import config
from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg
from pydrobert_speech_amd.compute import FrameComputer
from tests import structured as st

pytestmark = pytest.mark.gpu

EXTRAS = [n for n in st.suite_names() if n not in st.FIXTURE_CONFIGS and n != "lds_fft_8192"]
K32 = st.MARGIN * st.KAPPA_REF
K32_DFT = st.MARGIN * st.KAPPA_REF_DFT
K64 = st.MARGIN_F64 * st.KAPPA_REF
F32 = dict(eps=st.EPS32, rtol=1e-4, atol=1e-5)
F64 = dict(eps=st.EPS64, rtol=1e-9, atol=1e-9)
# the two configurations of test_gpu_post.py's one-launch statics + deltas tests that have every sample format
DELTAS_CONFIGS = {
    "fbank80_energy": {"name": "stft", "bank": {"name": "fbank", "num_filts": 80}, "frame_length_ms": 25,
                       "include_energy": True, "use_power": True},
    "mel64_1024_energy": {"name": "stft", "bank": {"name": "tri", "scaling_function": "mel", "num_filts": 64,
                                                   "sampling_rate": 48000},
                          "frame_length_ms": 20, "include_energy": True, "use_power": True},
}
_GAINS = {}


def build(cfg):
    return alias_factory_subclass_from_arg(FrameComputer, json.loads(json.dumps(cfg)))


def report(name, flow, label, result):
    path = os.environ.get("PDS_STRUCTURED_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(f"{name} {flow} {label} kappa {result.kappa:.3f} bound_only {result.bound_only}/{result.elements}\n")


def utterances(name, p, dtype):
    """[(label, samples as the kernel gets them)]: cases() in the flow's sample format"""
    if name not in _GAINS:
        _GAINS[name] = st.straddle_gain(p)
    out = []
    for label, x in st.cases(p, gain=_GAINS[name]):
        out.append((label, st.quantise_i16(x) if dtype == "i2" else x.astype(dtype)))
    return out


def pack(sigs, twice=True):
    """The utterances back to back, then (twice) once more, each copy at an odd sample offset"""
    import torch

    offs, pos = [], 0
    for _ in sigs:
        offs.append(pos)
        pos += len(_)
    if twice:
        for x in sigs:
            pos += 1 + pos % 2 + 2 * (len(offs) % 3)  # -> odd
            assert pos % 2 == 1
            offs.append(pos)
            pos += len(x)
        sigs = sigs + sigs
    buf = np.zeros(pos + 1, sigs[0].dtype)
    for o, x in zip(offs, sigs):
        buf[o : o + len(x)] = x
    return torch.from_numpy(buf).cuda(), np.asarray(offs), np.asarray([len(x) for x in sigs])


def oracle_signal(x, preemph):
    """(signal the oracle transforms, raw samples or None): float64, pre-emphasised like the reference's pass"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        return (orc.preemphasize(x, preemph), x) if preemph else (x, None)


def check_rows(name, flow, p, labelled, got, rows, kappa, tol, preemph=0.0, nonfinite=None):
    """Every utterance of the launch under the model; one report line per label (the worse of its copies)"""
    failures, worst = [], {}
    n = len(labelled)
    for b in range(len(rows) - 1):
        label, x = labelled[b % n]
        sig, raw = oracle_signal(x, preemph)
        mode = nonfinite(label) if nonfinite else "nan"
        r = st.compare(got[rows[b] : rows[b + 1]], sig, p, kappa, raw=raw, nonfinite=mode, **tol)
        if not r.ok:
            failures.append(f"{name} / {flow} / {label} (utterance {b}): {r.message}")
        if label not in worst or r.kappa > worst[label].kappa:
            worst[label] = r
    for label, r in worst.items():
        report(name, flow, label, r)
    assert not failures, "\n".join([f"{len(failures)} utterances outside the model (kappa {kappa:.3g}):"] + failures[:12])


def run_flow(name, flow, comp, p, dtype, kappa, tol, preemph=0.0, generic=False, out_dtype=None):
    import torch

    labelled = utterances(name, p, dtype)
    x, offs, lens = pack([s for _, s in labelled])
    out = None
    if out_dtype is not None:
        total = sum(comp.num_frames(int(n)) for n in lens)
        out = torch.full((total, comp.num_coeffs), float("nan"), dtype=out_dtype, device="cuda")
    feats, rows = comp.compute_packed(x, offs, lens, generic=generic, preemphasis=preemph, out=out)
    assert int(rows[-1]) == feats.shape[0] == 2 * len(labelled) * p.num_frames(st.utterance_length(p))
    check_rows(name, flow, p, labelled, feats.cpu().numpy(), rows, kappa, tol, preemph)
    return feats


# ------------------------------------------------------------------------------------------- the flows ----


@pytest.mark.parametrize("name", st.FIXTURE_CONFIGS + EXTRAS)
def test_fused_float32_kernel(name):
    p, cfg = st.suite_config(name)
    comp = build(cfg)
    assert comp.kernel_kind == comp.dft_size
    run_flow(name, "f32", comp, p, "f4", K32, F32)


@pytest.mark.parametrize("name", st.FIXTURE_CONFIGS + [n for n in EXTRAS if st.named_dft_size(n) <= 1024])
def test_direct_dft_kernel(name):
    p, cfg = st.suite_config(name)
    assert p.dft_size <= 1024 and (name in st.FIXTURE_CONFIGS or p.dft_size == st.named_dft_size(name))
    run_flow(name, "generic", build(cfg), p, "f4", K32_DFT, F32, generic=True)


@pytest.mark.parametrize("dtype", ["f4", "f8"])
def test_lds_fft_8192(dtype):
    p, cfg = st.suite_config("lds_fft_8192")
    comp = build(cfg)
    assert comp.dft_size == 8192 and comp.kernel_kind == 0
    if dtype == "f4":
        run_flow("lds_fft_8192", "f32", comp, p, "f4", K32, F32)
    else:
        run_flow("lds_fft_8192", "f64", comp, p, "f8", K64, F64)


@pytest.mark.parametrize("name", st.FIXTURE_CONFIGS)
def test_float64_samples_float32_arithmetic(name, monkeypatch):
    """has_f64in plans: samples rounded at the frame load; float32 and float64 feature stores of one kernel"""
    import torch

    p, cfg = st.suite_config(name)
    comp = build(cfg)
    assert comp._native_plan().has_f64in
    monkeypatch.setattr(config, "FLOAT64_ARITHMETIC", "float32")
    wide = run_flow(name, "f64in/f64out", comp, p, "f8", K32, F32)
    narrow = run_flow(name, "f64in/f32out", comp, p, "f8", K32, F32, out_dtype=torch.float32)
    assert wide.dtype == torch.float64 and narrow.dtype == torch.float32
    assert torch.equal(wide.float(), narrow)


@pytest.mark.parametrize("name", st.FIXTURE_CONFIGS)
def test_float64_arithmetic(name):
    import torch

    p, cfg = st.suite_config(name)
    feats = run_flow(name, "f64", build(cfg), p, "f8", K64, F64)
    assert feats.dtype == torch.float64


@pytest.mark.parametrize("preemph", [0.0, 0.97], ids=["plain", "preemph"])
@pytest.mark.parametrize("name", st.FIXTURE_CONFIGS)
def test_int16_samples(name, preemph):
    p, cfg = st.suite_config(name)
    comp = build(cfg)
    assert comp._native_plan().has_i16in
    run_flow(name, "i16+preemph" if preemph else "i16", comp, p, "i2", K32, F32, preemph=preemph)


@pytest.mark.parametrize("name", st.FIXTURE_CONFIGS)
def test_float32_with_preemphasis(name):
    p, cfg = st.suite_config(name)
    run_flow(name, "f32+preemph", build(cfg), p, "f4", K32, F32, preemph=0.97)


WALKS = ["ell", "seg", "rseg", "mseg"]


def forced(name, walk, monkeypatch):
    """The computer of `name` built with PDS_STFT_WALK = `walk` (read when the plan is created) and its plan.  The
    switch forces a walk the plan built tables for and leaves the plan's own choice where it built none (the segment
    walks are for dense banks, the matrix-pipe one for N >= 1024): the plan says which, so a switch that went
    unread, or a plan that kept another walk it could have left, fails here and not nowhere."""
    monkeypatch.setenv("PDS_STFT_WALK", walk)
    comp = build(st.suite_config(name)[1])
    plan = comp._native_plan()
    assert plan.walk in plan.walks_built and "ell" in plan.walks_built, (name, walk, plan.walk, plan.walks_built)
    if walk in plan.walks_built:
        assert plan.walk == walk, (name, "forced", walk, "the plan prefers", plan.walk, plan.walks_built)
    return comp, plan


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("name", st.FIXTURE_CONFIGS)
def test_each_filter_walk(name, walk, monkeypatch):
    comp, plan = forced(name, walk, monkeypatch)
    p, _ = st.suite_config(name)
    # (the report names the walk the plan took, where it is not the one asked for)
    run_flow(name, f"walk={walk}" if plan.walk == walk else f"walk={walk}->{plan.walk}", comp, p, "f4", K32, F32)


def test_every_filter_walk_runs_on_some_fixture_configuration(monkeypatch):
    """test_each_filter_walk means what its name says: each of the four walks is the plan's walk for at least one
    of the five configurations when forced (and "ell" for all of them)"""
    taken = {walk: [n for n in st.FIXTURE_CONFIGS if forced(n, walk, monkeypatch)[1].walk == walk] for walk in WALKS}
    assert taken["ell"] == st.FIXTURE_CONFIGS, taken
    assert all(taken[walk] for walk in WALKS), taken


@pytest.mark.parametrize("bank", sorted(DELTAS_CONFIGS))
def test_one_launch_statics_and_deltas(bank):
    """launch_with_deltas(fused=True): the statics under the model, the deltas against orc.deltas of the launch's own
    statics (float32 accumulation against float64, as test_full_size_statics_plus_deltas_chain bounds it)"""
    import torch

    from pydrobert_speech_amd.post import Deltas
    comp = build(DELTAS_CONFIGS[bank])
    assert comp._native_plan().has_fused_deltas
    p = st.params_from_computer(comp)
    C = comp.num_coeffs
    labelled = utterances(bank, p, "f4")
    x, offs, lens = pack([s for _, s in labelled])
    layout = comp.prepare_layout(offs, lens, device=x.device)
    out = torch.full((layout.total_rows, 3 * C), float("nan"), device="cuda")
    comp.launch_with_deltas(x, layout, Deltas(2), out=out, fused=True)
    got, rows = out.cpu().numpy(), layout.row_offsets
    assert np.isfinite(got).all()
    check_rows(bank, "deltas/statics", p, labelled, got[:, :C], rows, K32, F32)
    for b in range(len(rows) - 1):
        mine = got[rows[b] : rows[b + 1]]
        want = orc.deltas(mine[:, :C], axis=0, num_deltas=2, target_axis=-1)
        assert np.allclose(mine, want, rtol=1e-5, atol=1e-5), (bank, labelled[b % len(labelled)][0], b)


# ------------------------------------------------------------------------------------ non-finite samples ----

# one configuration per transform size (128, 512, 1024, 4096) and an unpadded one (N = L = 320); three have an energy column
NONFINITE_CONFIGS = ["n128_fbank_8k", "c3_fbank80_energy", "c5_gammatone64_48k", "n4096_gabor_44k", "nopad320_fbank"]
VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}


def poisoned(p, dtype):
    """Noise at 3000 with one NaN, +Inf or -Inf: at the first sample (centred framing mirrors it into the left
    padding), the last (likewise on the right), mid-signal, and one sample either side of where a four-frame chunk's
    last frame ends and of where the next chunk's first frame starts"""
    n, L, S = st.utterance_length(p), p.frame_length, p.frame_shift
    rng = np.random.default_rng(31)
    spots = {"first": 0, "last": n - 1, "mid": n // 2 + 1,
             "chunk_start-1": 4 * S - p.pad_left - 1, "chunk_start": 4 * S - p.pad_left,
             "chunk_end-1": 3 * S - p.pad_left + L - 1, "chunk_end": 3 * S - p.pad_left + L}
    out = []
    for kind, v in VALUES.items():
        for spot, i in spots.items():
            x = (3000 * rng.standard_normal(n)).astype(dtype)
            x[i] = v
            out.append((f"{kind}@{spot}", x))
    return out


def nonfinite_case(name, flow, monkeypatch, zero_taps):
    p, cfg = st.suite_config(name)
    comp = build(cfg)
    dtype = "f8" if flow.startswith("f64in") else "f4"
    preemph = 0.97 if flow.endswith("preemph") else 0.0
    if dtype == "f8":
        monkeypatch.setattr(config, "FLOAT64_ARITHMETIC", "float32")
    labelled = [(label, x) for label, x in poisoned(p, dtype)
                if st.hidden_under_zero_taps(oracle_signal(x, preemph)[0], p) == zero_taps]
    assert len(labelled) >= 6 and len(labelled) % 3 == 0  # (the same spots for NaN, +Inf and -Inf)
    x, offs, lens = pack([s for _, s in labelled], twice=False)
    feats, rows = comp.compute_packed(x, offs, lens, preemphasis=preemph)
    got = feats.cpu().numpy()
    # (the oracle's own statement of what is poisoned, so that the test cannot pass on an oracle that poisons nothing)
    for _, s in labelled:
        with np.errstate(all="ignore"):
            bad = ~np.isfinite(orc.compute_full(oracle_signal(s, preemph)[0], p)).all(axis=1)
        assert 0 < bad.sum() < len(bad)
    check_rows(name, ("nonfinite0/" if zero_taps else "nonfinite/") + flow, p, labelled, got, rows, K32, F32, preemph,
               nonfinite=lambda label: "nan" if label.startswith("nan") else "rows")


@pytest.mark.parametrize("flow", ["f32", "f64in", "f32+preemph", "f64in+preemph"])
@pytest.mark.parametrize("name", NONFINITE_CONFIGS)
def test_nonfinite_samples(name, flow, monkeypatch):
    """Ordinary data for the kernels.  Which frames a sample poisons comes from the oracle's output: a NaN gives the
    oracle's NaN pattern element for element; an Inf makes exactly the oracle's non-finite rows non-finite, with the
    oracle's +inf in their energy column; every other row is finite and within the model.  (Pre-emphasis poisons
    samples n and n + 1.)  The spots of poisoned() that some frame meets only under an exactly-zero window tap are
    the test below."""
    nonfinite_case(name, flow, monkeypatch, zero_taps=False)


@pytest.mark.parametrize("flow", ["f32", "f64in", "f32+preemph", "f64in+preemph"])
@pytest.mark.parametrize("name", NONFINITE_CONFIGS)
def test_nonfinite_samples_under_zero_window_taps(name, flow, monkeypatch):
    """The same check where some frame meets the poisoned sample only under a window tap that is exactly 0 (the first
    or last tap of a Hann window).  The reference and the oracle poison that frame too: 0 * NaN = NaN, 0 * Inf = NaN.

    The fused kernels apply the window with v_mul_legacy_f32 (0 * x = 0 for every x), which the lanes past a frame's
    end need; with the tap stored as 0 they dropped such a sample and returned finite spectral coefficients for that
    one frame (18 of these 20 cases failed: "NaN positions differ, first at frame 4 coefficient 0", "finite spectral
    coefficients in a non-finite row").  The plan now stores a zero tap inside the frame as 2^-100
    (stft_fast.hip::fast_tables_create), which no finite sample can tell from 0 in float32 and every NaN / Inf
    survives."""
    nonfinite_case(name, flow, monkeypatch, zero_taps=True)
