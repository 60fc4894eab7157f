"""Short-integration parity on structured signals -- tones, DC, Nyquist, impulses, chirps, steps, levels from 1e-3 to
1e7, the log floor straddled, non-finite samples -- through the overlap-save FFT form (csrc/si_fft.hip), the direct
form (csrc/si.hip) and its float64 instantiation, under the float32 error model of tests/si_structured.py (read its
docstring first).

Every other SI parity test feeds Gaussian noise and compares with test_gpu_si.close, which forgives everything below
1e-3 max|want|: a filter spectrum delayed by 1e-3 sample passes it (test_si_structured_model.py shows that on the
CPU).  Here each configuration packs all families and levels into one batch without gaps, one utterance of
14 S + min(M, 3000) samples per family, and the same utterances once more so that each also starts elsewhere: one
launch per form.

What is allowed: an element passes the strict rule (2e-5 + 2e-4 |ref|; 1e-9 for float64) or the model's bound with
kappa = MARGIN x KAPPA_REF_FFT (FFT form) or MARGIN x KAPPA_REF_DIRECT (direct form) -- four times what the float32
restatements of the oracle need on the CPU on the same signals -- and the float64 direct kernel MARGIN_F64 x
KAPPA_REF_DIRECT at eps = 2^-53.  No form has a margin of its own.

With PDS_SI_STRUCTURED_REPORT=<file> in the environment every comparison appends one line there (configuration, form,
family, the largest kappa the kernel needed, elements that passed only through the bound):
profiles/r15a_si_structured_parity.txt is such a file.
"""
import os

import numpy as np
import pytest

from oracle import si_oracle as so
from tests import si_structured as sis

pytestmark = pytest.mark.gpu

K_FFT = sis.MARGIN * sis.KAPPA_REF_FFT
K_DIRECT = sis.MARGIN * sis.KAPPA_REF_DIRECT
K_F64 = sis.MARGIN_F64 * sis.KAPPA_REF_DIRECT
_ORACLE = {}  # (configuration, label, sample type) -> oracle_linear(): computed once, read-only


def report(name, form, label, result):
    path = os.environ.get("PDS_SI_STRUCTURED_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(f"{name} {form} {label} kappa {result.kappa:.4f} bound_only {result.bound_only}/{result.elements}\n")


def run_packed(comp, sigs, direct=False):
    """The utterances back to back, no gaps (a read past an utterance's end lands in its neighbour), one launch"""
    import torch

    lens = np.array([len(x) for x in sigs], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    feats, rows = comp.compute_packed(torch.from_numpy(np.concatenate(sigs)).cuda(), offs, lens, direct=direct)
    return feats.cpu().numpy(), rows


def check_rows(name, form, p, labelled, got, rows, kappa, tol):
    """Every utterance of the launch under the model; one report line per label (the worse of its copies)"""
    failures, worst = [], {}
    n = len(labelled)
    for b in range(len(rows) - 1):
        label, x = labelled[b % n]
        key = (name, label, x.dtype.str)
        if key not in _ORACLE:
            _ORACLE[key] = sis.oracle_linear(x, so.frame_count(len(x), p), p)
        r = sis.compare(got[rows[b] : rows[b + 1]], x, p, kappa, pre=_ORACLE[key], **tol)
        if not r.ok:
            failures.append(f"{name} / {form} / {label} (utterance {b}): {r.message}")
        if label not in worst or r.kappa > worst[label].kappa:
            worst[label] = r
    for label, r in worst.items():
        report(name, form, label, r)
    assert not failures, "\n".join([f"{len(failures)} utterances outside the model (kappa {kappa:.3g}):"] + failures[:12])


@pytest.mark.parametrize("name", sis.suite_names())
def test_every_form_on_structured_signals(name):
    comp = sis.build(name)
    p, form = sis.suite_config(name)
    assert comp.fft_size == form[0], (comp.fft_size, form)  # (the host restatement of csrc/si_shape.h)
    assert (name == sis.DIRECT_ONLY) == (comp.fft_size == 0)
    cases = sis.cases(p)
    T = so.frame_count(sis.utterance_length(p), p)
    for dtype, direct, flow, kappa, tol in (("f4", False, "fft", K_FFT, sis.F32), ("f4", True, "direct", K_DIRECT, sis.F32),
                                            ("f8", True, "direct_f64", K_F64, sis.F64)):
        if flow == "fft" and not comp.fft_size:
            continue
        labelled = [(label, x.astype(dtype)) for label, x in cases]
        sigs = [x for _, x in labelled]
        got, rows = run_packed(comp, sigs + sigs, direct=direct)
        assert got.dtype == np.dtype(dtype) and rows[-1] == got.shape[0] == 2 * len(labelled) * T
        check_rows(name, flow, p, labelled, got, rows, kappa, tol)


@pytest.mark.parametrize("name", ["s1_gabor_mel", "s6_fbank_long"])
def test_streaming_ragged_chunks(name):
    """A chirp and the impulses through compute_chunk with ragged cuts, and finalize (each call a launch of the FFT
    form whose `start` moves the transforms relative to the signal): the reference's frame counts call by call, the
    frames against so.features over the whole signal under the same model"""
    comp = sis.build(name)
    p, form = sis.suite_config(name)
    assert comp.fft_size == form[0] != 0
    S, n = p.frame_shift, 40 * p.frame_shift + p.max_support + 77
    rng = np.random.default_rng(5)
    for family in ("chirp", "impulses"):
        x = sis.FAMILIES[family](n, sis.GRID_N, rng).astype("f4")
        cuts = np.unique(np.concatenate([rng.integers(1, n, 9), [1, S - 1, 3 * S, 3 * S + 1, 17 * S + S // 2]]))
        pieces = np.split(x, cuts)
        outs = [comp.compute_chunk(piece) for piece in pieces] + [comp.finalize()]
        counts = so.stream_frame_counts([len(piece) for piece in pieces], p)
        assert [len(o) for o in outs] == counts and sum(counts) > 30 and sum(c > 0 for c in counts) >= 5
        got = np.concatenate(outs)
        assert got.dtype == np.float32
        r = sis.compare(got, x, p, K_FFT, **sis.F32)
        report(name, "stream", family, r)
        assert r.ok, (name, family, r.message)


# ------------------------------------------------------------------------------------ non-finite samples ----

VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}
# a 1024-point bank whose Hann window ends in zero taps and whose stream starts with virtual zeros, a causal one with
# a Gamma window, the real magnitude bank with an energy row and raw sums, the 2048-point one
NONFINITE_CONFIGS = ["s1_gabor_mel", "s2_gammatone_power", "s3_tri_energy_nolog", "s6_fbank_long"]


def spans(p, T):
    """[lo, hi) of the signal samples each frame's taps and window reach: t S + start - (M - 1) .. t S + start + 2 S"""
    t = np.arange(T)
    return t * p.frame_shift + sis.start_of(p) - (p.max_support - 1), t * p.frame_shift + sis.start_of(p) + 2 * p.frame_shift


def poison_spots(p, form, n):
    """{label: sample index}: the first, the last and a middle sample, either side of a transform boundary
    (d V + start - (NT - V)), and -- where the window starts or ends with a tap that is exactly zero -- the one sample
    some frame meets only under that tap (and under the filters' last or first tap)"""
    S, M, start = p.frame_shift, p.max_support, sis.start_of(p)
    NT, blocks = form
    V = blocks * S
    d = (n // 2 + NT) // V
    edge = d * V + start - (NT - V)
    spots = {"first": 0, "last": n - 1, "mid": n // 2, "edge-1": edge - 1, "edge": edge}
    t0 = (n // 3) // S
    if p.window[0] == 0:
        spots["zero_tap_first"] = t0 * S + start - (M - 1)
    if p.window[-1] == 0:
        spots["zero_tap_last"] = t0 * S + start + 2 * S - 1
    assert all(0 <= j < n for j in spots.values()), spots
    return spots, t0


@pytest.mark.parametrize("direct", [False, True], ids=["fft", "direct"])
@pytest.mark.parametrize("name", NONFINITE_CONFIGS)
def test_nonfinite_samples_are_contained(name, direct):
    """Containment, not pattern parity (the FFT form turns every output of a transform whose stretch holds a NaN or an
    Inf into NaN, the oracle's np.convolve poisons an M-tap window, the direct form one of M rounded up to nine).
    Each poisoned utterance stands between two clean ones without gaps, in a batch that also holds its clean copy:
    every frame the oracle poisons is non-finite (a set neither empty nor everything; a sample under an exactly-zero
    window tap counts: 0 * NaN = NaN); every frame with no non-finite sample within R = 2048 of its span is finite
    and has the clean copy's bits; every finite row is within the model; the neighbours have the bits they have in a
    batch of their own."""
    comp = sis.build(name)
    p, form = sis.suite_config(name)
    assert comp.fft_size == form[0] != 0
    S, M = p.frame_shift, p.max_support
    n = 2 * (sis.R + M + 2 * S) + 6 * S + 3
    rng = np.random.default_rng(31)
    clean = (3000 * rng.standard_normal(n)).astype("f4")
    left, right = (3000 * rng.standard_normal(3 * S + 7)).astype("f4"), (3000 * rng.standard_normal(5 * S + 1)).astype("f4")
    spots, t0 = poison_spots(p, form, n)
    labelled = []
    for kind, v in VALUES.items():
        for spot, j in spots.items():
            x = clean.copy()
            x[j] = v
            labelled.append((f"{kind}@{spot}", j, x))
    sigs = []
    for _, _, x in labelled + [("clean", None, clean)]:
        sigs += [left, x, right]
    got, rows = run_packed(comp, sigs, direct=direct)
    alone, alone_rows = run_packed(comp, [left, right], direct=direct)
    own = {0: alone[alone_rows[0] : alone_rows[1]], 2: alone[alone_rows[1] : alone_rows[2]]}
    assert len(own[0]) > 0 and len(own[2]) > 0 and np.isfinite(alone).all()
    T = so.frame_count(n, p)
    lo, hi = spans(p, T)
    kappa, flow = (K_DIRECT, "nonfinite/direct") if direct else (K_FFT, "nonfinite/fft")
    mine = lambda b: got[rows[b] : rows[b + 1]]  # noqa: E731
    want_clean = mine(3 * len(labelled) + 1)
    assert want_clean.shape == (T, comp.num_coeffs) and np.isfinite(want_clean).all()
    r = sis.compare(want_clean, clean, p, kappa, **sis.F32)
    assert r.ok, r.message
    failures, worst = [], {}
    for i, (label, j, x) in enumerate(labelled):
        for side in (0, 2):
            if not np.array_equal(mine(3 * i + side), own[side]):
                failures.append(f"{label}: the {'left' if side == 0 else 'right'} neighbour's rows changed")
        y = mine(3 * i + 1)
        pre = sis.oracle_linear(x, T, p)
        must = ~np.isfinite(pre[0])  # (element by element: what the oracle poisons)
        assert 0 < must.any(axis=1).sum() < T, label
        if "zero_tap" in label:
            assert must[t0].all() and (lo[t0] == j or hi[t0] - 1 == j), label
        far = (j < lo - sis.R) | (j >= hi + sis.R)
        assert far.any() and not (far & must.any(axis=1)).any(), label
        finite = np.isfinite(y).all(axis=1)
        if np.isfinite(y[must]).any():
            t = int(np.argwhere(must & np.isfinite(y))[0, 0])
            failures.append(f"{label}: frame {t} is finite, its span [{lo[t]}, {hi[t]}) holds sample {j}")
        if not finite[far].all():
            t = int(np.argwhere(far & ~finite)[0, 0])
            failures.append(f"{label}: frame {t} is not finite, sample {j} is beyond {sis.R} of its span [{lo[t]}, {hi[t]})")
        elif not np.array_equal(y[far], want_clean[far]):
            failures.append(f"{label}: a frame far from sample {j} differs from the clean copy's")
        rows_ok = finite & ~must.any(axis=1)
        r = sis.compare(np.where(rows_ok[:, None], y, 0.0), x, p, kappa, pre=pre, rows=rows_ok, **sis.F32)
        if not r.ok:
            failures.append(f"{label}: {r.message}")
        spot = label.split("@")[1]
        if spot not in worst or r.kappa > worst[spot].kappa:
            worst[spot] = r
    for spot, r in worst.items():
        report(name, flow, spot, r)
    assert not failures, "\n".join([f"{name} / {flow}: {len(failures)} findings"] + failures[:12])
