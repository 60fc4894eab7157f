"""The fused STFT kernel's items at a signal end -- frames that reach in front of sample 0 or past sample n - 1 and are
gathered with reflected indices -- at the shortest lengths that reach each arm of that code, in every sample flow.

An item is GROUPS = 64 / N2 consecutive frames of one utterance (csrc/stft_wave_kernel.h).  It is regular when all its
frames exist and every row they load lies inside the signal; otherwise its frames are gathered: in straight-line code
where one bounce suffices (mode 1: start >= -n and start + L <= 2 n for every frame), by the rolled general reflection
otherwise (mode 2).  `modes()` below restates that classification on the host, the lengths of every case are searched
with it, and each case asserts that the arm it is there for is reached.

Three framings per case, one launch each: the computer's own pad_left; pad_left = 0 (causal frames: the only natural
way to `start + L > 2 n`, the upper boundary between the modes); and a pad_left equal to a signal's length (`start = -n`
against `start < -n`, the lower boundary).  Utterances are a few frames long, so a case takes well under a second.

Check A: every utterance against oracle.stft_oracle.compute_full with the tolerance of tests/test_gpu_stft.py -- strict
1e-5 + 1e-4 |ref|, and with a fused pre-emphasis 2e-5 + 2e-4 |ref| or the float32 floor of tools/fuzz_parity.py.

Check B (flows without pre-emphasis): y = x explicitly reflect-padded by a multiple of GROUPS * S on the left and enough
samples on the right that the frames of x are frames of regular items of y.  Frame t of x and frame t + k of y then go
through identical arithmetic on identical samples, only the loads differ: the rows must be equal bit for bit.  A case in
which no row of an edge item was compared fails.
"""
import dataclasses
import importlib.util
import os

import numpy as np
import pytest

from oracle import stft_oracle as orc
from pydrobert_speech_amd import config
from tests import flow_matrix as fm
from tests import structured as st
from tests.conftest import ROOT, assert_features_close
from tests.test_gpu_structured import build

pytestmark = pytest.mark.gpu

F32 = dict(rtol=1e-4, atol=1e-5)
PREEMPH = 0.97
# geometry (N1, N2, ROWS of csrc/stft_geoms.def) -> configuration of the structured suite that reaches it
GEOMETRIES = {
    (32, 16, 25): "c1_kaldi_fbank",          # the headline: N = 512, 16 lanes per frame, kaldi shift (pad_left 120)
    (32, 8, 25): "n256_tri_8k",              # 8 kHz: N = 256, 8 lanes, eight frames per item
    (64, 32, 38): "n2048_fbank_48k",         # N = 2048, 32 lanes, two frames per item, energy
    (64, 64, 38): "n4096_fbank_48k",         # N = 4096, 64 lanes, one frame per item
    (25, 16, 25): "nopad400_tri_mel40",      # no zero padding: N = L = 400
}
ENERGY = "c3_fbank80_energy"                 # the headline geometry once more, with the energy column


def _cases():
    out = []
    for row, name in list(GEOMETRIES.items()) + [((32, 16, 25), ENERGY)]:
        flows = ["f32", "f32+preemph"]
        if fm.dft_size(row) in fm.F64IN_SIZES:
            flows += ["i16", "i16+preemph", "f64", "f64+preemph"]
        if row in fm.FUSED_ROWS:
            flows += ["deltas", "ragged:f32", "ragged:i16+preemph"]
        out += [(row, name, flow) for flow in flows]
    return out


CASES = _cases()


@dataclasses.dataclass
class Framed(orc.StftParams):
    """StftParams with the frames' left padding given, as FrameComputer.launch(pad_left=...) takes it"""
    pad: int = 0

    @property
    def pad_left(self) -> int:
        return self.pad


def framed(p, pad):
    return Framed(**{f.name: getattr(p, f.name) for f in dataclasses.fields(orc.StftParams)}, pad=pad)


def modes(n, p, pad, G, span, pre):
    """Per item of an utterance of n samples: 0 regular, 1 one bounce, 2 general reflection, None where the kernel's
    choice between 0 and 1 depends on the rows an instantiation loads (`span` = the most any of them does)"""
    L, S, nfr = p.frame_length, p.frame_shift, p.num_frames(n)
    out = []
    for tb in range(0, nfr, G):
        starts = [min(tb + g, nfr - 1) * S - pad for g in range(G)]
        if any(s < -n or s + L > 2 * n for s in starts):
            out.append(2)
        elif tb + G > nfr or any(s < pre or s + L > n for s in starts):
            out.append(1)
        elif starts[-1] + span <= n:
            out.append(0)
        else:
            out.append(None)
    return out


def pick_lengths(p, G, span, pre):
    """[(framing pad_left, [lengths])] and what the lengths are there for: the shortest utterances that reach each arm"""
    L, S, P = p.frame_length, p.frame_shift, p.pad_left
    natural, why = [1], {}

    def first(lo, hi, ok):
        return next((n for n in range(lo, hi) if ok(n)), None)

    # the first item bounces once, a later one is regular
    n = first(L // 2 + 1, 40 * G * S + 4 * L, lambda n: (lambda m: m[0] == 1 and 0 in m and 2 not in m)(modes(n, p, P, G, span, pre)))
    assert n is not None
    natural.append(n)
    why["regular behind an edge"] = (P, n)
    # the last item has lanes past the last frame
    for rem in (1, 2, 3):
        if rem < G:
            n = (2 * G + rem) * S
            assert p.num_frames(n) % G == rem
            natural.append(n)
    # first and last frame in one item, a frame that bounces at both ends
    def both_ends(n):
        nfr = p.num_frames(n)
        m = modes(n, p, P, G, span, pre)
        return 0 < nfr <= G and m == [1] and any(t * S - P < 0 and t * S - P + L > n for t in range(nfr))
    n = first(L // 2 + 1, 2 * L, both_ends)
    if n is not None:
        natural.append(n)
        why["both ends"] = (P, n)
    natural.append(37 * S + 11)  # (and a longer one: the batch is ragged)
    # causal frames: one sample either side of start + L > 2 n
    n = first(L // 2 + 1, 3 * L, lambda n: 2 in modes(n, p, 0, G, span, pre) and set(modes(n + 1, p, 0, G, span, pre)) == {1})
    assert n is not None
    why["start + L > 2 n"] = (0, n)
    # a left padding as long as a signal: start = -n (one bounce) against start < -n
    n = first(L // 2 + 2, 3 * L, lambda n: set(modes(n, p, n, G, span, pre)) == {1} and 2 in modes(n - 1, p, n, G, span, pre))
    assert n is not None
    why["start < -n"] = (n, n - 1)
    upper = why["start + L > 2 n"][1]
    return [(P, natural), (0, [upper, upper + 1, 9 * S + 3]), (n, [n, n - 1, 9 * S + 1])], why


def signal(n, flow, rng):
    x = 3000 * rng.standard_normal(n)
    if flow.startswith("i16") or flow.endswith("i16+preemph"):
        return np.clip(np.rint(x), -32768, 32767).astype("i2")
    return x.astype("f8" if flow.startswith("f64") else "f4")


def padded(x, padl, padr):
    return x[orc.reflect_indices(np.arange(-padl, len(x) + padr), len(x))]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.fixture(scope="module")
def floor_close():
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(ROOT, "tools", "fuzz_parity.py"))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    return fuzz.close


@pytest.mark.parametrize("row,name,flow", CASES, ids=[f"{name}-{flow}" for _, name, flow in CASES])
def test_edge_items(row, name, flow, floor_close, monkeypatch):
    import torch

    from pydrobert_speech_amd.post import Deltas

    p, cfg = st.suite_config(name)
    comp = build(cfg)
    plan = comp._native_plan()
    assert plan.geometry == row and comp.kernel_kind == comp.dft_size
    N2, rows_per_frame = row[1], row[2]
    G, L, S, C = 64 // N2, comp.frame_length, comp.frame_shift, comp.num_coeffs
    span = max(rows_per_frame * N2, (rows_per_frame + 1) // 2 * 32)  # (float64 samples on 16 lanes load pairs of rows)
    pre = flow.endswith("+preemph")
    coeff = PREEMPH if pre else 0.0
    ragged, deltas = flow.startswith("ragged"), flow == "deltas"
    monkeypatch.setattr(config, "FLOAT64_ARITHMETIC", "float32")
    monkeypatch.setattr(config, "RAGGED_SCHEDULING", ragged)
    framings, why = pick_lengths(p, G, span, 1 if pre else 0)
    assert row != (32, 16, 25) or "both ends" in why
    rng = np.random.default_rng(sum(row) + len(flow))
    for pad, lens in framings:
        pf = framed(p, pad)
        xs = [signal(n, flow, rng) for n in lens]
        # check B's copies: frame t of x is frame t + k of y, inside regular items of y
        k = G * max(1, -(-(pad + 1) // (G * S)))
        ys = []
        for x in xs:
            nfr = pf.num_frames(len(x))
            if pre or not nfr:
                continue
            last = (k + nfr - 1) // G
            need = max((last + 1) * G * S + S, (last * G + G - 1) * S - pad + span) + 8
            y = padded(x, k * S, max(need - k * S - len(x), L))
            m = modes(len(y), pf, pad, G, span, 0)
            assert all(m[c] == 0 for c in range(k // G, last + 1)), (name, flow, pad, len(x), m)
            ys.append(y)
        sigs = xs + ys
        lengths = [len(s) for s in sigs]
        offs = np.concatenate([[0], np.cumsum(lengths)[:-1]])
        dev = torch.from_numpy(np.concatenate(sigs)).cuda()
        layout = comp.prepare_layout(offs, lengths, device=dev.device)
        assert [int(v) for v in layout.nframes] == [pf.num_frames(n) for n in lengths]
        if ragged:
            assert layout.fill < 0.9
        if deltas:
            got = comp.launch_with_deltas(dev, layout, Deltas(2), pad_left=pad, fused=True).cpu().numpy()
        else:
            got = comp.launch(dev, layout, pad_left=pad, preemphasis=coeff).cpu().numpy()
        r = layout.row_offsets
        assert got.shape == (r[-1], (3 if deltas else 1) * C) and np.isfinite(got).all()
        # check A
        for b, x in enumerate(xs):
            mine = got[r[b] : r[b + 1]]
            x64 = x.astype(np.float64)
            want = orc.compute_full(orc.preemphasize(x64, coeff) if pre else x64, pf)
            if pre:
                ok, msg = floor_close(mine, want, 2e-4, 2e-5, is_log=p.use_log)
                assert ok, (name, flow, pad, len(x), msg)
            else:
                assert_features_close(mine[:, :C], want, what=(name, flow, pad, len(x)), **F32)
            if deltas:
                assert np.allclose(mine, orc.deltas(mine[:, :C], axis=0, num_deltas=2, target_axis=-1), rtol=1e-5, atol=1e-5)
        # check B
        if pre:
            continue
        compared, at = 0, len(xs)
        for b, x in enumerate(xs):
            nfr = pf.num_frames(len(x))
            if not nfr:
                continue
            mine, theirs = got[r[b] : r[b + 1], :C], got[r[at] + k : r[at] + k + nfr, :C]
            at += 1
            same = (bits(mine) == bits(theirs)).all(axis=1)
            assert same.all(), (name, flow, pad, len(x), "frames", np.flatnonzero(~same)[:8].tolist())
            m = modes(len(x), pf, pad, G, span, 0)
            compared += sum(min(G, nfr - c * G) for c in range(len(m)) if m[c] in (1, 2))
        assert at == len(sigs)
        assert compared > 0, (name, flow, pad, "no row of an edge item went through check B")
