"""Every object file of the fused STFT kernel against the oracle, in every sample flow it holds instantiations for.

tests/flow_matrix.py declares one configuration per PDS_GEOM line of csrc/stft_geoms.def and the flows each line must
run (test_flow_matrix_host.py holds that table against the .def on the CPU).  Each case here is one or two launches
of the structured batch of test_gpu_structured.py -- every signal family and level, each utterance 12 S + L samples,
the whole set packed twice with the second copy at odd sample offsets -- under the same model: strict
1e-5 + 1e-4 |ref|, or the bound with kappa = MARGIN * KAPPA_REF.  No tolerance of its own.

Every case proves which instantiation ran: the plan names the line it dispatches to (plan.geometry), its has_f64in /
has_i16in / has_fused_deltas flags are what the matrix declares, and the launch runs with torch.Tensor.to poisoned,
so that a float64-in or int16-in entry point that declines (FrameComputer.launch would convert and retry) fails the
case instead of hiding behind the fallback.  The one-launch deltas and the fused CMVN sums also watch the return code
of their entry point: their fallbacks (two launches) convert nothing.
"""
import numpy as np
import pytest

from oracle import stft_oracle as orc
from pydrobert_speech_amd import _native, config
from tests import flow_matrix as fm
from tests import structured as st
from tests.test_gpu_structured import F32, K32, K32_DFT, build, check_rows, pack, run_flow, utterances

pytestmark = pytest.mark.gpu


def poison_conversions(comp, monkeypatch):
    """Every launch method of `comp` runs with torch.Tensor.to failing (prepare_layout, which uploads its index arrays
    with .to, stays as it is: run_flow calls it through compute_packed)"""
    import torch

    def fail(*a, **k):
        pytest.fail("the launch converted a tensor: a fused entry point declined and the fallback ran")

    def guarded(inner):
        def call(*a, **k):
            with monkeypatch.context() as m:
                m.setattr(torch.Tensor, "to", fail)
                return inner(*a, **k)
        return call

    for method in ("launch", "launch_with_deltas", "launch_with_cmvn"):
        monkeypatch.setattr(comp, method, guarded(getattr(comp, method)))


def watch(symbol, monkeypatch):
    """The return codes of every call of the library's `symbol` from here on"""
    lib, codes = _native.lib(), []
    inner = getattr(lib, symbol)

    def call(*a):
        codes.append(inner(*a))
        return codes[-1]

    monkeypatch.setattr(lib, symbol, call)
    return codes


def sample_flow(name, flow, comp, p, monkeypatch):
    import torch

    preemph = 0.97 if flow.endswith("+preemph") else 0.0
    if flow.startswith("f32"):
        run_flow(name, flow, comp, p, "f4", K32, F32, preemph=preemph)
    elif flow.startswith("i16"):
        feats = run_flow(name, flow, comp, p, "i2", K32, F32, preemph=preemph)
        assert feats.dtype == torch.float32
    elif flow == "f64in":
        monkeypatch.setattr(config, "FLOAT64_ARITHMETIC", "float32")
        wide = run_flow(name, "f64in/f64out", comp, p, "f8", K32, F32)
        narrow = run_flow(name, "f64in/f32out", comp, p, "f8", K32, F32, out_dtype=torch.float32)
        assert wide.dtype == torch.float64 and narrow.dtype == torch.float32
        assert torch.equal(wide.float(), narrow)  # one kernel, two store widths
    else:
        # (float32 stores: float64 features with a fused pre-emphasis are these, widened by the caller)
        monkeypatch.setattr(config, "FLOAT64_ARITHMETIC", "float32")
        run_flow(name, flow, comp, p, "f8", K32, F32, preemph=preemph, out_dtype=torch.float32)


def deltas_flow(name, flow, comp, p, K, monkeypatch):
    """As test_one_launch_statics_and_deltas: statics under the model, deltas against orc.deltas of the launch's own
    statics at the bound of that test; and nothing written past (K + 1) C columns of a wider buffer"""
    import torch

    from pydrobert_speech_amd.post import Deltas

    C, spare, fill = comp.num_coeffs, 5, -12345.0
    labelled = utterances(name, p, "f4")
    x, offs, lens = pack([s for _, s in labelled])
    layout = comp.prepare_layout(offs, lens, device=x.device)
    out = torch.full((layout.total_rows + 2, (K + 1) * C + spare), fill, device="cuda")
    codes = watch("pds_stft_deltas_batch", monkeypatch)
    res = comp.launch_with_deltas(x, layout, Deltas(K), out=out, fused=True)
    assert codes == [0], ("the one-launch entry point did not serve the call", codes)
    assert res.shape == (layout.total_rows + 2, (K + 1) * C)
    full, rows = out.cpu().numpy(), layout.row_offsets
    assert (full[:, (K + 1) * C :] == fill).all() and (full[layout.total_rows :] == fill).all()
    got = full[: layout.total_rows, : (K + 1) * C]
    assert np.isfinite(got).all()
    check_rows(name, f"{flow}/statics", p, labelled, got[:, :C], rows, K32, F32)
    for b in range(len(rows) - 1):
        mine = got[rows[b] : rows[b + 1]]
        want = orc.deltas(mine[:, :C], axis=0, num_deltas=K, target_axis=-1)
        assert np.allclose(mine, want, rtol=1e-5, atol=1e-5), (name, flow, labelled[b % len(labelled)][0], b)


def ragged_lengths(L, S, rng):
    # (L // 2 + 1: the shortest utterance that yields frames at all -- one frame, or two where S is small)
    return [0, 1, S, 7 * S + 3, 400 * S, 3 * S, 0, 55 * S, 2 * S, L // 2 + 1] + [
        int(n) for n in rng.integers(0, 60 * S, size=60)]


def ragged_flow(name, flow, comp, p, monkeypatch):
    """config.RAGGED_SCHEDULING on against off: the same rows bit for bit; the utterance behind an empty one, the
    shortest one with frames and the longest against the oracle under the model"""
    import torch

    what = flow.split(":")[1]
    preemph = 0.97 if what.endswith("+preemph") else 0.0
    lens = ragged_lengths(comp.frame_length, comp.frame_shift, np.random.default_rng(6))
    host = st.quantise_i16(3000 * np.random.default_rng(16).standard_normal(int(np.sum(lens))))
    host = host if what.startswith("i16") else host.astype("f4")
    x = torch.from_numpy(host).cuda()
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    layout = comp.prepare_layout(offs, lens, device=x.device)
    assert layout.fill < 0.9
    monkeypatch.setattr(config, "RAGGED_SCHEDULING", True)
    a = torch.full((layout.total_rows, comp.num_coeffs), float("nan"), device="cuda")
    comp.launch(x, layout, out=a, preemphasis=preemph)
    monkeypatch.setattr(config, "RAGGED_SCHEDULING", False)
    b = torch.full_like(a, float("nan"))
    comp.launch(x, layout, out=b, preemphasis=preemph)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    got, rows = a.cpu().numpy(), layout.row_offsets
    assert lens[6] == 0 and 1 <= rows[10] - rows[9] <= 2 and lens[4] == max(lens)
    for u in (7, 9, 4):
        sig = host[offs[u] : offs[u] + lens[u]].astype(np.float64)
        raw = sig if preemph else None
        r = st.compare(got[rows[u] : rows[u + 1]], orc.preemphasize(sig, preemph) if preemph else sig, p, K32, raw=raw, **F32)
        assert r.ok, (name, flow, "utterance", u, r.message)


def cmvn_flow(name, flow, comp, p, monkeypatch):
    """As test_cmvn_sums_fused_with_the_stft_launch: the fused result against CMVN().apply_rows of the launch's own
    features at 1e-9 (float64 out), the same call twice equal bits; and those features against the oracle"""
    import torch

    from pydrobert_speech_amd.post import CMVN

    S, C = comp.frame_shift, comp.num_coeffs
    lens = [0, S, 5 * S, 9 * S + 3, 300 * S, 33 * S, 1, 4 * S, 120 * S + 7, 12 * S, 2 * S] + [
        int(n) for n in np.random.default_rng(11).integers(0, 40 * S, size=60)]
    host = (3000 * np.random.default_rng(12).standard_normal(int(np.sum(lens)))).astype("f4")
    x = torch.from_numpy(host).cuda()
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    layout = comp.prepare_layout(offs, lens, device=x.device)
    feats = torch.full((layout.total_rows, C), float("nan"), device="cuda")
    codes = watch("pds_stft_cmvn_batch_f32", monkeypatch)
    fused = comp.launch_with_cmvn(x, layout, CMVN(), feats_out=feats, fused=True)
    again = comp.launch_with_cmvn(x, layout, CMVN(), fused=True)
    assert codes == [0, 0], ("the fused entry point did not serve the call", codes)
    two = CMVN().apply_rows(feats, layout.row_offsets, out_dtype=torch.float64)
    assert fused.dtype == torch.float64 and fused.shape == two.shape == (layout.total_rows, C)
    assert bool(torch.isfinite(fused).all()) and torch.equal(fused, again)
    assert float((fused - two).abs().max()) <= 1e-9 * max(1.0, float(two.abs().max()))
    got, rows = feats.cpu().numpy(), layout.row_offsets
    for u in (1, 4, 8):
        sig = host[offs[u] : offs[u] + lens[u]].astype(np.float64)
        r = st.compare(got[rows[u] : rows[u + 1]], sig, p, K32, **F32)
        assert r.ok, (name, flow, "utterance", u, r.message)
    want = orc.cmvn_local(got[rows[4] : rows[5]], axis=-1)
    assert np.allclose(fused[rows[4] : rows[5]].cpu().numpy(), want, rtol=1e-8, atol=1e-8)


@pytest.mark.parametrize("preemph", [0.0, 0.97], ids=["plain", "preemph"])
@pytest.mark.parametrize("dtype", ["f8", "i2"])
def test_declined_sample_formats_take_the_converting_fallback(dtype, preemph, monkeypatch):
    """The other side of the poisoned conversions: a plan that has the float64-in / int16-in instantiations but whose
    filter table stays outside LDS (the N = 2048 gammatone bank).  The entry point must decline, so that
    FrameComputer.launch converts and retries, and the result is the oracle's.

    With a fused pre-emphasis pds_stft_batch_f64in did not decline: the launch handed the call to the direct-DFT
    kernel, which read the float64 samples as pairs of floats and returned PDS_OK (every structured utterance failed:
    "NaN positions differ", "got -2.07 want 5.93, needs kappa 2.79e+05")."""
    import torch

    name = "n2048_gammatone_44k"
    p, cfg = st.suite_config(name)
    comp = build(cfg)
    plan = comp._native_plan()
    assert plan.geometry == (64, 32, 64) and plan.has_f64in and plan.has_i16in
    monkeypatch.setattr(config, "FLOAT64_ARITHMETIC", "float32")
    codes = watch("pds_stft_batch_f64in" if dtype == "f8" else "pds_stft_batch_i16in", monkeypatch)
    flow = ("f64in" if dtype == "f8" else "i16") + ("+preemph" if preemph else "") + "/declined"
    # (converted samples with a pre-emphasis and the table outside LDS run the generic float32 kernel: the bound of
    # test_direct_dft_kernel; a float32 DFT-matrix restatement of this very case needs kappa 0.20 on the CPU)
    feats = run_flow(name, flow, comp, p, dtype, K32_DFT if preemph else K32, F32, preemph=preemph, out_dtype=torch.float32)
    assert codes and all(rc != 0 for rc in codes), ("the plan serves the call: take another bank for this test", codes)
    assert feats.dtype == torch.float32


@pytest.mark.parametrize("row,name,flow", fm.cases(), ids=[f"{name}-{flow}" for _, name, flow in fm.cases()])
def test_flow(row, name, flow, monkeypatch):
    kind = flow.split(":")[0]
    if kind == "cmvn":
        monkeypatch.setenv("PDS_STFT_WALK", fm.CMVN_WALK[row])
    p, cfg = st.suite_config(name)
    comp = build(cfg)
    plan = comp._native_plan()
    assert comp.kernel_kind == comp.dft_size == fm.dft_size(row)
    assert plan.geometry == row, (name, "reaches", plan.geometry, "and not", row)
    assert (plan.has_f64in, plan.has_i16in, plan.has_fused_deltas) == fm.plan_flags(row), (name, row)
    poison_conversions(comp, monkeypatch)
    if kind == "deltas":
        deltas_flow(name, flow, comp, p, int(flow[-1]), monkeypatch)
    elif kind == "ragged":
        ragged_flow(name, flow, comp, p, monkeypatch)
    elif kind == "cmvn":
        assert plan.walk == fm.CMVN_WALK[row] and plan.has_fused_cmvn, (name, plan.walk, plan.walks_built)
        cmvn_flow(name, flow, comp, p, monkeypatch)
    else:
        sample_flow(name, flow, comp, p, monkeypatch)
