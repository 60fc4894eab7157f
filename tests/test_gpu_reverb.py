"""pre.Reverb on the device against tests/reverb_model.py: the wet signal under the float32 error model (every tap count
and peak at which the block and partition arithmetic changes, a ragged batch with odd offsets and gaps, the structured
signal families at three levels, three sample dtypes and three bank dtypes), the normalisation bit for bit given the
device's wet signal, independence of batch, offset and order, locality of NaN and inf, the copied utterances, more
utterances than one launch of the scale kernel takes, ``apply`` against ``apply_packed``, and reproducibility on
another stream."""
import numpy as np
import pytest

from tests import reverb_model as rm

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import pydrobert_speech_amd as ps  # noqa: E402


def allowed(n):
    """the device's allowance for an utterance of n samples: the project's margin times the calibrated kappa"""
    return rm.MARGIN * rm.kappa_ref(n)


TAPS = (1, 2, 511, 512, 513, 1024, 1025, 1537)
LENGTHS = (0, 1, 2, 511, 512, 513, 1023, 1024, 1025, 2049, 5000)
NP_DTYPES = {"f32": np.float32, "f64": np.float64, "i16": np.int16}


def peaks_of(L):
    return sorted({d for d in (0, 1, 511, 512, L - 1) if d < L})


def bank(dtype):
    """[(L, d, taps)] for every tap count and peak of the suite, in `dtype`"""
    return [(L, d, rm.response(L, d, dtype=dtype)) for L in TAPS for d in peaks_of(L)]


def as_dtype(x, kind):
    if kind == "i16":
        return np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    return x.astype(NP_DTYPES[kind])


def pack(utts, dtype, gap_rng):
    """(buffer, offsets, lengths): odd offsets and gaps between the utterances; the gaps hold a recognisable value"""
    offs, pos = [], 3
    for u in utts:
        offs.append(pos)
        pos += len(u) + int(gap_rng.integers(0, 4)) * 2 + 1
    buf = np.full(pos + 5, 77, dtype=dtype)
    for o, u in zip(offs, utts):
        buf[o : o + len(u)] = u
    return buf, np.asarray(offs, dtype=np.int64), np.asarray([len(u) for u in utts], dtype=np.int64)


_SIGNALS = {}


def signals(n):
    if n not in _SIGNALS:
        _SIGNALS[n] = rm.signals(n, seed=2024 + n)
    return _SIGNALS[n]


@pytest.mark.parametrize("bank_kind", ["f64", "f32", "i16"])
@pytest.mark.parametrize("sig_kind", ["f32", "i16", "f64"])
def test_wet_signal_meets_the_error_model(sig_kind, bank_kind):
    rirs = bank(NP_DTYPES[bank_kind])
    rev = ps.pre.Reverb([h for _, _, h in rirs], normalize_output=False, seed=1)
    assert [int(d) for d in rev.rir_peaks] == [d for _, d, _ in rirs]
    utts, which = [], []
    for j in range(len(rirs)):
        for i, n in enumerate(LENGTHS):
            cases = signals(n)
            label, x = cases[(7 * j + 3 * i) % len(cases)]
            utts.append(as_dtype(x, sig_kind))
            which.append((j, label))
    buf, offs, lens = pack(utts, NP_DTYPES[sig_kind], np.random.default_rng(3))
    plan = ps.pre.ReverbPlan(np.asarray([j for j, _ in which], dtype=np.int64), np.ones(len(utts), dtype=bool))
    out = rev.apply_packed(torch.from_numpy(buf).cuda(), offs, lens, plan=plan).cpu().numpy()
    assert out.dtype == np.float32 and out.shape == buf.shape
    worst = (0.0, None)
    for (j, label), u, o, n in zip(which, utts, offs, lens):
        L, d, h = rirs[j]
        ok, k, msg = rm.check(out[o : o + n], u, h, d, allowed(n))
        assert ok, (L, d, n, label, msg)
        if k / allowed(n) > worst[0]:
            worst = (k / allowed(n), k, (L, d, int(n), label))
    print("worst share of the allowance, its kappa", worst, "allowances", allowed(1), allowed(512))
    if sig_kind == "f32":  # the gaps keep their bytes
        mask = np.ones(len(buf), dtype=bool)
        for o, n in zip(offs, lens):
            mask[o : o + n] = False
        assert out[mask].tobytes() == buf[mask].tobytes()


@pytest.mark.parametrize("d", [0, 1, 511, 512, 1536])
def test_a_unit_impulse_at_the_peak_returns_the_signal_byte_for_byte(d):
    h = np.zeros(1537, dtype=np.float32)
    h[d] = 1.0
    rng = np.random.default_rng(d)
    utts = [(3000 * rng.standard_normal(n)).astype(np.float32) for n in LENGTHS]
    buf, offs, lens = pack(utts, np.float32, rng)
    for normalize in (False, True):
        rev = ps.pre.Reverb([h], normalize_output=normalize, seed=1)
        assert int(rev.rir_peaks[0]) == d
        out = rev.apply_packed(torch.from_numpy(buf).cuda(), offs, lens).cpu().numpy()
        assert out.tobytes() == buf.tobytes()


def _normalisation_batch():
    rng = np.random.default_rng(11)
    rirs = [rm.response(700, 30), np.zeros(40), rm.response(5, 2)]
    utts = [(3000 * rng.standard_normal(n)) for n in (5000, 40000, 700, 513, 1, 33000)]
    utts[2][:] = 0.0  # a silent utterance
    rir_of = np.asarray([0, 2, 0, 1, 2, 0], dtype=np.int64)  # (utterance 3 meets the all-zero response)
    return rirs, utts, rir_of


@pytest.mark.parametrize("sig_kind", ["f32", "i16", "f64"])
def test_normalisation_has_the_models_bits_given_the_wet_signal(sig_kind):
    rirs, utts, rir_of = _normalisation_batch()
    utts = [as_dtype(u, sig_kind) for u in utts]
    buf, offs, lens = pack(utts, NP_DTYPES[sig_kind], np.random.default_rng(5))
    plan = ps.pre.ReverbPlan(rir_of, np.ones(len(utts), dtype=bool))
    x = torch.from_numpy(buf).cuda()
    out, wet = ps.pre.Reverb(rirs, seed=1).apply_packed(x, offs, lens, plan=plan, return_wet=True)
    raw = ps.pre.Reverb(rirs, normalize_output=False, seed=1).apply_packed(x, offs, lens, plan=plan)
    out, wet, raw = out.cpu().numpy(), wet.cpu().numpy(), raw.cpu().numpy()
    for b, (u, o, n) in enumerate(zip(utts, offs, lens)):
        assert raw[o : o + n].tobytes() == wet[o : o + n].tobytes()  # without the normalisation: the wet bytes
        ps_, py, c, want = rm.normalise(u, wet[o : o + n])
        print(b, "Ps", ps_, "Py", py, "c", c)
        assert out[o : o + n].tobytes() == want.tobytes(), b
        if b in (2, 3):  # silence in, or an all-zero response: nothing to scale, the wet signal stands
            assert c == 0.0 and out[o : o + n].tobytes() == wet[o : o + n].tobytes()
            assert not wet[o : o + n].any()
        else:
            assert c > 0.0
            assert abs(float(np.mean(out[o : o + n].astype(np.float64) ** 2)) / float(ps_) - 1.0) < 1e-5


def _alone(rev, u, j):
    n = len(u)
    plan = ps.pre.ReverbPlan(np.asarray([j]), np.ones(1, dtype=bool))
    return rev.apply_packed(torch.from_numpy(u).cuda(), [0], [n], plan=plan).cpu().numpy()


@pytest.mark.parametrize("sig_kind", ["f32", "i16"])
def test_an_utterances_bytes_do_not_depend_on_batch_offset_or_order(sig_kind):
    rng = np.random.default_rng(21)
    rirs = [rm.response(1537, 512), rm.response(513, 0), rm.response(7, 3)]
    rev = ps.pre.Reverb(rirs, seed=1)
    utts = [as_dtype(3000 * rng.standard_normal(n), sig_kind) for n in (2049, 513, 5000, 1, 1024)]
    rir_of = np.asarray([0, 1, 2, 0, 1], dtype=np.int64)
    alone = [_alone(rev, u, j) for u, j in zip(utts, rir_of)]
    for order, lead in ((range(5), 0), (range(5), 1), (range(5), 4), (reversed(range(5)), 3), ([2, 0, 4], 64)):
        order = list(order)
        pieces, offs, pos = [], [], lead
        for b in order:
            offs.append(pos)
            pos += len(utts[b]) + 1 + (b % 3)
        buf = np.zeros(pos, dtype=NP_DTYPES[sig_kind])
        for b, o in zip(order, offs):
            buf[o : o + len(utts[b])] = utts[b]
        plan = ps.pre.ReverbPlan(rir_of[order], np.ones(len(order), dtype=bool))
        out = rev.apply_packed(torch.from_numpy(buf).cuda(), offs, [len(utts[b]) for b in order], plan=plan)
        out = out.cpu().numpy()
        for b, o in zip(order, offs):
            assert out[o : o + len(utts[b])].tobytes() == alone[b].tobytes(), (order, lead, b)
        del pieces


@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("L,d", [(1537, 512), (513, 1), (2, 0)])
def test_a_bad_sample_spoils_only_its_window_and_no_other_utterance(L, d, bad):
    rng = np.random.default_rng(31)
    h = rm.response(L, d)
    P = rm.partitions(L)
    rev = ps.pre.Reverb([h], normalize_output=False, seed=1)
    n = 6000
    clean = [(3000 * rng.standard_normal(m)).astype(np.float32) for m in (n, 700)]
    buf, offs, lens = pack(clean, np.float32, rng)
    base = rev.apply_packed(torch.from_numpy(buf).cuda(), offs, lens).cpu().numpy()
    for i in (0, 1700, 2047, 2048, n - 1):
        dirty = buf.copy()
        dirty[offs[0] + i] = bad
        got = rev.apply_packed(torch.from_numpy(dirty).cuda(), offs, lens).cpu().numpy()
        t = np.arange(n)
        b0 = rm.BLOCK * ((t + d) // rm.BLOCK)
        inside = (b0 - rm.BLOCK * (P + 2) <= i) & (i < b0 + 3 * rm.BLOCK)
        a, b = got[offs[0] : offs[0] + n], base[offs[0] : offs[0] + n]
        assert a[~inside].tobytes() == b[~inside].tobytes(), (i, int(np.flatnonzero(a != b)[0]))
        # the outputs the definition's sum reaches are spoilt
        reached = (t + d - i >= 0) & (t + d - i < L) & (np.asarray(h)[np.clip(t + d - i, 0, L - 1)] != 0)
        assert not np.isfinite(a[reached]).any()
        assert got[offs[1] : offs[1] + 700].tobytes() == base[offs[1] : offs[1] + 700].tobytes()
    # with the normalisation it spoils its own utterance's scale, and never another utterance
    norm = ps.pre.Reverb([h], seed=1)
    dirty = buf.copy()
    dirty[offs[0] + 100] = bad
    want = norm.apply_packed(torch.from_numpy(buf).cuda(), offs, lens).cpu().numpy()
    got = norm.apply_packed(torch.from_numpy(dirty).cuda(), offs, lens).cpu().numpy()
    assert got[offs[1] : offs[1] + 700].tobytes() == want[offs[1] : offs[1] + 700].tobytes()


def _payloads(n, rng):
    x = (3000 * rng.standard_normal(n)).astype(np.float32)
    bits = x.view(np.uint32)
    if n >= 8:
        bits[1], bits[2], bits[3], bits[5] = 0x7FC12345, 0xFF800001, 0x80000000, 0x00000001
    return x


@pytest.mark.parametrize("sig_kind", ["f32", "i16", "f64"])
def test_utterances_that_are_not_applied_are_copied(sig_kind):
    rng = np.random.default_rng(41)
    if sig_kind == "f32":
        utts = [_payloads(n, rng) for n in LENGTHS]
    else:
        utts = [as_dtype(3000 * rng.standard_normal(n) + 0.123456789, sig_kind) for n in LENGTHS]
    buf, offs, lens = pack(utts, NP_DTYPES[sig_kind], rng)
    x = torch.from_numpy(buf).cuda()
    h = rm.response(600, 100)
    none = ps.pre.Reverb([h], prob=0.0, seed=4).apply_packed(x, offs, lens, seeds=list(range(len(utts))))
    none = none.cpu().numpy()
    for u, o, n in zip(utts, offs, lens):
        assert none[o : o + n].tobytes() == rm.copied(u).tobytes()
    if sig_kind == "f32":
        assert none.tobytes() == buf.tobytes()  # gaps included
    half = ps.pre.Reverb([h], prob=0.5, seed=4)
    plan = half.plan(len(utts), seeds=list(range(100, 100 + len(utts))))
    assert plan.applied.any() and not plan.applied.all()
    some, wet = half.apply_packed(x, offs, lens, plan=plan, return_wet=True)
    some, wet = some.cpu().numpy(), wet.cpu().numpy()
    for b, (u, o, n) in enumerate(zip(utts, offs, lens)):
        if not plan.applied[b]:
            assert some[o : o + n].tobytes() == rm.copied(u).tobytes(), b
        elif sig_kind != "f32":  # (the float32 utterances carry NaN: their bound is the locality test's)
            ok, _, msg = rm.check(wet[o : o + n], u, h, 100, allowed(n))
            assert ok, (b, msg)
            assert some[o : o + n].tobytes() == rm.normalise(u, wet[o : o + n])[3].tobytes(), b


def test_more_utterances_than_one_launch_takes():
    B, n = 65537, 3
    rng = np.random.default_rng(51)
    x = (3000 * rng.standard_normal(B * n)).astype(np.float32)
    h = np.asarray([0.5, -1.0])
    rev = ps.pre.Reverb([h], seed=1)
    offs, lens = np.arange(B, dtype=np.int64) * n, np.full(B, n, dtype=np.int64)
    plan = ps.pre.ReverbPlan(np.zeros(B, dtype=np.int64), np.ones(B, dtype=bool))
    out, wet = rev.apply_packed(torch.from_numpy(x).cuda(), offs, lens, plan=plan, return_wet=True)
    out, wet = out.cpu().numpy().reshape(B, n), wet.cpu().numpy().reshape(B, n)
    X = x.reshape(B, n).astype(np.float64)
    # d = 1: wet[t] = -x[t] + 0.5 x[t + 1] (the tail past the last sample is dropped)
    want = -X
    want[:, :-1] += 0.5 * X[:, 1:]
    E = (X * X).sum(axis=1, keepdims=True)  # (the whole utterance lies in every output's window)
    bound = rm.RTOL * np.abs(want) + allowed(n) * rm.EPS32 * np.sqrt(1.25) * np.sqrt(E)
    assert (np.abs(wet - want) <= bound).all()
    from tests import mix_model

    with np.errstate(all="ignore"):
        c = np.sqrt(mix_model.energy_rows(x.reshape(B, n)) / np.float64(n) / (mix_model.energy_rows(wet) / np.float64(n)))
    assert out.tobytes() == (wet.astype(np.float64) * c[:, None]).astype(np.float32).tobytes()


def test_apply_equals_apply_packed_and_one_plan_serves_two_views():
    rng = np.random.default_rng(61)
    rirs = [rm.response(L, d) for L, d in ((300, 10), (513, 0), (1025, 600), (40, 39))]
    X = (3000 * rng.standard_normal((3, 4, 700))).astype(np.float32)
    got = ps.pre.Reverb(rirs, seed=9).apply(X)
    assert got.shape == X.shape and got.dtype == X.dtype
    rows = X.reshape(-1, 700)
    offs, lens = np.arange(12, dtype=np.int64) * 700, np.full(12, 700, dtype=np.int64)
    want = ps.pre.Reverb(rirs, seed=9).apply_packed(torch.from_numpy(rows.reshape(-1)).cuda(), offs, lens)
    assert got.tobytes() == want.cpu().numpy().tobytes()
    along = ps.pre.Reverb(rirs, seed=9).apply(np.ascontiguousarray(np.moveaxis(X, -1, 0)), axis=0)
    assert np.moveaxis(along, 0, -1).tobytes() == got.tobytes()
    t = ps.pre.Reverb(rirs, seed=9).apply(torch.from_numpy(X).cuda())
    assert t.is_cuda and t.cpu().numpy().tobytes() == got.tobytes()
    # one plan on two views of the same utterances: the same response for both
    rev = ps.pre.Reverb(rirs, prob=0.7, seed=2)
    plan = rev.plan(12, seeds=list(range(12)))
    assert (plan.rir == rev.plan(12, seeds=list(range(12))).rir).all()
    view2 = (rows * np.float32(0.5)).reshape(-1)  # an exact scaling: the wet signal scales with it
    a, wa = rev.apply_packed(torch.from_numpy(rows.reshape(-1)).cuda(), offs, lens, plan=plan, return_wet=True)
    b, wb = rev.apply_packed(torch.from_numpy(view2).cuda(), offs, lens, plan=plan, return_wet=True)
    assert (wa.cpu().numpy() * np.float32(0.5)).tobytes() == wb.cpu().numpy().tobytes()


def test_the_result_is_the_same_run_twice_and_on_another_stream():
    rng = np.random.default_rng(71)
    rirs = [rm.response(1537, 511), rm.response(4000, 50)]
    utts = [(3000 * rng.standard_normal(n)).astype(np.float32) for n in (5000, 513, 20000)]
    buf, offs, lens = pack(utts, np.float32, rng)
    x = torch.from_numpy(buf).cuda()
    seeds = [5, 6, 7]
    first = ps.pre.Reverb(rirs, seed=1).apply_packed(x, offs, lens, seeds=seeds).cpu().numpy()
    again = ps.pre.Reverb(rirs, seed=1).apply_packed(x, offs, lens, seeds=seeds).cpu().numpy()
    assert first.tobytes() == again.tobytes()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        other = ps.pre.Reverb(rirs, seed=1).apply_packed(x, offs, lens, seeds=seeds)
    stream.synchronize()
    assert other.cpu().numpy().tobytes() == first.tobytes()
    plan = ps.pre.Reverb(rirs, seed=1).plan(3, seeds=seeds)
    want_rir, want_applied = rm.plan(ps.pre.dither_keys(seeds), 2, 1.0)
    assert (plan.rir == want_rir).all() and (plan.applied == want_applied).all()
