"""Batched streaming of short-integration computers on the GPU (multistream_si.SiStreamBatch) and the per-utterance
start of the kernels under it (pds_si_batch_starts_*).

The C ABI: pds_si_batch_starts_* against pds_si_batch_* with the scalar start, bit for bit, for direct filtering in
float32 and float64 and the 1024- and 2048-point overlap-save forms.  SiStreamBatch: every call's rows against a
private ShortIntegrationFrameComputer fed the same chunks (np.array_equal: the work span of a stream is the private
computer's kept tail, `start` and the frame count are the same numbers, so the kernels see the same inputs at the same
alignment) and against the reference's recorded frame counts and features (tests/golden/si_stream_random.npz)."""
import json
import os

import numpy as np
import pytest

from pydrobert_speech_amd import _native
from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg
from pydrobert_speech_amd.compute import FrameComputer
from pydrobert_speech_amd.multistream_si import SiStreamBatch
from pydrobert_speech_amd.post import Deltas
from pydrobert_speech_amd.pre import Preemphasize
from tests.conftest import GOLDEN
from tests.test_gpu_si import F32, META, NAMES, close

pytestmark = pytest.mark.gpu

CAPACITY = 8
IDS = [7, 0, 2, 3, 5, 6]  # stream i of a configuration's six chunkings; ids 1 and 4 stay idle, one sits on capacity - 1
LONG_SHIFT = {"name": "si", "bank": {"name": "gabor", "scaling_function": "mel", "num_filts": 4,
                                     "sampling_rate": 48000}, "frame_shift_ms": 50, "use_power": True}
LONG_SUPPORT = {"name": "si", "bank": {"name": "fbank", "num_filts": 40}}


def build(cfg):
    if isinstance(cfg, str):
        cfg = META["configs"][cfg]
    return alias_factory_subclass_from_arg(FrameComputer, json.loads(json.dumps(cfg)))


@pytest.fixture(scope="module")
def master():
    with np.load(os.path.join(GOLDEN, "si.npz")) as z:
        return z["master"]


@pytest.fixture(scope="module")
def chunkings():
    with np.load(os.path.join(GOLDEN, "si_stream_random.npz")) as z:
        return {k: z[k] for k in z.files}


# ---- the C ABI -----------------------------------------------------------------------------------------------------

ABI_CONFIGS = ["s1_gabor_mel", "s3_tri_energy_nolog", "s6_fbank_long"]  # complex taps; real taps; real, 2048-point
FORMS = ["direct_f32", "direct_f64", "fft"]


def si_call(comp, form, signal, offsets, lengths, nframes, start=None, starts=None):
    """pds_si_batch_* (scalar `start`) or pds_si_batch_starts_* (`starts` per utterance) over the packed host `signal`;
    the rows as a host array, NaN where nothing was written"""
    import torch

    lib = _native.lib()
    plan = comp._native_plan()
    f64 = form == "direct_f64"
    sig = torch.from_numpy(np.ascontiguousarray(signal, dtype=np.float64 if f64 else np.float32)).cuda()
    B = len(lengths)
    rows = np.concatenate([[0], np.cumsum(nframes)])
    meta = [offsets, lengths, nframes, rows[:-1]] + ([starts] if starts is not None else [])
    d_meta = torch.from_numpy(np.asarray(meta, dtype=np.int64)).cuda()
    out = torch.full((int(rows[-1]), comp.num_coeffs), float("nan"), dtype=sig.dtype, device="cuda")
    most = int(max(nframes))
    stream = torch.cuda.current_stream().cuda_stream
    head = (plan.handle, sig.data_ptr()) + tuple(d_meta[r].data_ptr() for r in range(len(meta))) + (B, most)
    if starts is None:
        head += (int(start),)
    tail = (out.data_ptr(), out.stride(0), stream)
    if f64:
        fn = lib.pds_si_batch_f64 if starts is None else lib.pds_si_batch_starts_f64
        rc = fn(*head, *tail)
    else:
        need = int(lib.pds_si_scratch_len(plan.handle, B, most)) if form == "fft" else 0
        assert (need > 0) == (form == "fft")
        scratch = torch.empty(max(need, 1), dtype=torch.float32, device="cuda")
        fn = lib.pds_si_batch_f32 if starts is None else lib.pds_si_batch_starts_f32
        rc = fn(*head, scratch.data_ptr() if need else None, *tail)
    _native.check(rc, "pds_si_batch")
    return out.cpu().numpy(), rows


def test_the_abi_configurations_cover_the_four_forms():
    sizes = {name: build(name).fft_size for name in ABI_CONFIGS}
    assert sizes == {"s1_gabor_mel": 1024, "s3_tri_energy_nolog": 1024, "s6_fbank_long": 2048}
    assert not build("s1_gabor_mel")._real and build("s3_tri_energy_nolog")._real


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ABI_CONFIGS)
def test_equal_starts_give_the_scalar_calls_bits(master, name, form):
    comp = build(name)
    lengths = [2239, 2240, 4001]
    signal = np.concatenate([master[:n] for n in lengths])
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    nframes = [comp.num_frames(n) for n in lengths]
    assert min(nframes) > 0
    for start in (comp._skip0 - comp._lead, comp._max_support - 1 + 2 * comp.frame_shift):
        want, _ = si_call(comp, form, signal, offsets, lengths, nframes, start=start)
        got, _ = si_call(comp, form, signal, offsets, lengths, nframes, starts=[start] * 3)
        assert np.isfinite(want).all() and want.std() > 0
        assert np.array_equal(got, want)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ABI_CONFIGS)
def test_different_starts_give_each_utterances_scalar_call(master, name, form):
    comp = build(name)
    S, M = comp.frame_shift, comp._max_support
    lengths = [2239, 2240, 4001, 3000, 1500]
    signal = np.concatenate([master[i : i + n] for i, n in enumerate(lengths)])
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    starts = [-S, 0, M - 1, M - 1 + 3 * S, M - 1 + S]
    nframes = [3, 1, 11, 5, 0]
    got, rows = si_call(comp, form, signal, offsets, lengths, nframes, starts=starts)
    assert not np.isnan(got).any()  # every row was written
    for b in range(len(lengths)):
        if nframes[b]:
            x = signal[offsets[b] : offsets[b] + lengths[b]]
            want, _ = si_call(comp, form, x, [0], [lengths[b]], [nframes[b]], start=starts[b])
            assert np.array_equal(got[rows[b] : rows[b + 1]], want), (b, starts[b])
    # rows of different starts do differ (the starts act)
    same, _ = si_call(comp, form, signal, offsets, lengths, nframes, starts=[starts[2]] * 5)
    assert not np.array_equal(same[rows[0] : rows[1]], got[rows[0] : rows[1]])


def test_null_starts_are_refused(master):
    import torch

    comp = build("s1_gabor_mel")
    lib = _native.lib()
    plan = comp._native_plan()
    meta = torch.zeros((4, 1), dtype=torch.int64, device="cuda")
    for fn, dtype, extra in ((lib.pds_si_batch_starts_f32, torch.float32, (None,)),
                             (lib.pds_si_batch_starts_f64, torch.float64, ())):
        sig = torch.zeros(16, dtype=dtype, device="cuda")
        out = torch.zeros((1, comp.num_coeffs), dtype=dtype, device="cuda")
        rc = fn(plan.handle, sig.data_ptr(), meta[0].data_ptr(), meta[1].data_ptr(), meta[2].data_ptr(),
                meta[3].data_ptr(), None, 1, 1, *extra, out.data_ptr(), out.stride(0), None)
        assert rc == -1 and "d_starts" in _native.last_error()


# ---- SiStreamBatch against a private computer ------------------------------------------------------------------------


def pieces_of(x, cuts):
    return np.split(x, np.asarray(cuts, dtype=np.int64))


_PRIVATE = {}


def private(key, cfg, signals, cuts):
    """per stream the outputs of a private computer's compute_chunk calls and its finalize; computed once per `key`"""
    if key not in _PRIVATE:
        comp = build(cfg)
        outs = []
        for x, c in zip(signals, cuts):
            outs.append([comp.compute_chunk(p) for p in pieces_of(x, c)] + [comp.finalize()])
        for stream in outs:
            for o in stream:
                o.flags.writeable = False
        _PRIVATE[key] = outs
    return _PRIVATE[key]


def fixture_streams(chunkings, master, name, dtype):
    signals, cuts = [], []
    for case in range(6):
        n = int(chunkings[f"{name}/{case}/n"])
        signals.append(master[7 : 7 + n].astype(dtype))
        cuts.append(chunkings[f"{name}/{case}/cuts"])
    return signals, cuts


def drive(sb, signals, cuts, ids, order=None, alone=(), packed=False):
    """stream i's j-th chunk goes in tick j under id ``ids[i]``; a stream whose chunks are done is finalized in the next
    tick.  `order`: permutation of the streams inside every call; `alone`: streams that get calls of their own;
    `packed`: through compute_chunks_packed / finalize_packed.  Returns per stream the list of its calls' outputs"""
    import torch

    pieces = [pieces_of(x, c) for x, c in zip(signals, cuts)]
    outs = [[] for _ in signals]
    order = list(range(len(signals))) if order is None else list(order)

    def call(streams, final, tick):
        if not streams:
            return
        sel = [ids[i] for i in streams]
        if final:
            if packed:
                feats, rows = sb.finalize_packed(sel)
                got = [feats[rows[q] : rows[q + 1]].cpu().numpy() for q in range(len(sel))]
            else:
                got = sb.finalize(sel)
        else:
            chunks = [pieces[i][tick] for i in streams]
            if packed:
                flat = np.concatenate(chunks) if chunks else np.zeros(0, sb.dtype)
                d = torch.from_numpy(np.ascontiguousarray(flat)).cuda()
                feats, rows = sb.compute_chunks_packed(sel, d, [len(c) for c in chunks])
                got = [feats[rows[q] : rows[q + 1]].cpu().numpy() for q in range(len(sel))]
            else:
                got = sb.compute_chunks(sel, chunks)
        for i, o in zip(streams, got):
            outs[i].append(o)

    for tick in range(max(map(len, pieces)) + 1):
        feed = [i for i in order if tick < len(pieces[i])]
        fin = [i for i in order if tick == len(pieces[i])]
        for group, final in ((feed, False), (fin, True)):
            call([i for i in group if i not in alone], final, tick)
            for i in group:
                if i in alone:
                    call([i], final, tick)
    return outs


def assert_same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert [o.shape for o in g] == [o.shape for o in w], i
        for call, (a, b) in enumerate(zip(g, w)):
            assert a.dtype == b.dtype and np.array_equal(a, b), (i, call)


@pytest.mark.parametrize("dtype", ["f4", "f8"])
@pytest.mark.parametrize("name", NAMES)
def test_random_chunkings_as_concurrent_streams(chunkings, master, name, dtype):
    signals, cuts = fixture_streams(chunkings, master, name, dtype)
    want = private((name, dtype), name, signals, cuts)
    comp = build(name)
    with SiStreamBatch(comp, capacity=CAPACITY, dtype=dtype) as sb:
        assert sb.num_coeffs == comp.num_coeffs and sb.lookahead == 0
        got = drive(sb, signals, cuts, IDS)
        assert not sb.started(np.arange(CAPACITY)).any()
        idle = sb.finalize([1, 4])  # never started
        assert all(o.shape == (0, comp.num_coeffs) and o.dtype == np.float64 for o in idle)
    for case in range(6):
        assert [len(o) for o in got[case]] == chunkings[f"{name}/{case}/counts"].tolist(), (name, case)
        close(np.concatenate(got[case]), chunkings[f"{name}/{case}/feats"], **F32)
    assert_same(got, want)
    assert not comp.started  # the computer's own streaming state was not touched


@pytest.mark.parametrize("name", ["s1_gabor_mel", "s6_fbank_long", "s5_gabor_causal"])
def test_order_and_subsets_do_not_matter(chunkings, master, name):
    signals, cuts = fixture_streams(chunkings, master, name, "f4")
    want = private((name, "f4"), name, signals, cuts)
    comp = build(name)
    with SiStreamBatch(comp, capacity=CAPACITY) as sb:
        assert_same(drive(sb, signals, cuts, IDS, order=[4, 1, 5, 0, 3, 2]), want)
        # the same object again (every stream was finalized), the longest stream in calls of its own
        assert_same(drive(sb, signals, cuts, IDS[::-1], alone={5}), want)


@pytest.mark.parametrize("dtype", ["f4", "f8"])
def test_packed_calls_equal_the_host_calls(chunkings, master, dtype):
    name = "s1_gabor_mel"
    signals, cuts = fixture_streams(chunkings, master, name, dtype)
    want = private((name, dtype), name, signals, cuts)
    with SiStreamBatch(build(name), capacity=CAPACITY, dtype=dtype) as sb:
        got = drive(sb, signals, cuts, IDS, packed=True)
    # (an idle finalize aside, packed calls keep the working dtype; the private computer's rows have it too)
    assert_same(got, want)


def test_reuse_after_finalize(chunkings, master):
    name = "s3_tri_energy_nolog"
    signals, cuts = fixture_streams(chunkings, master, name, "f4")
    first, second = (signals[5], cuts[5]), (signals[4][::-1].copy(), cuts[4])
    with SiStreamBatch(build(name), capacity=4) as fresh:
        want = drive(fresh, [second[0]], [second[1]], [3])
    with SiStreamBatch(build(name), capacity=4) as sb:
        drive(sb, [first[0]], [first[1]], [3])
        assert not sb.started([3])[0]
        got = drive(sb, [second[0]], [second[1]], [3])
    assert sum(len(o) for o in want[0]) > 0
    assert_same(got, want)


@pytest.mark.parametrize("dtype", ["f4", "f8"])
@pytest.mark.parametrize("which", ["long_shift", "long_support"])
def test_long_shift_and_long_supports(master, which, dtype):
    cfg = LONG_SHIFT if which == "long_shift" else LONG_SUPPORT
    comp = build(cfg)
    if which == "long_shift":
        # the FFT form declines, the direct kernel takes several passes of its thread block per tile
        assert comp.frame_shift == 2400 and comp.fft_size == 0
    else:
        assert comp._max_support > 2048 and comp.fft_size == 0  # direct form only
    signals = [master[:6000].astype(dtype), master[100:5400].astype(dtype)]
    cuts = [[1000, 2500, 2501, 5200], [3000, 5299]]
    want = private((which, dtype), cfg, signals, cuts)
    assert sum(len(o) for o in want[0]) > 1 and sum(len(o) for o in want[1]) > 1
    with SiStreamBatch(comp, capacity=2, dtype=dtype) as sb:
        assert_same(drive(sb, signals, cuts, [1, 0]), want)


@pytest.mark.parametrize("dtype", ["f4", "f8"])
def test_pcm_chunks_with_preemphasis_and_deltas(chunkings, master, dtype):
    name = "s1_gabor_mel"
    dtype = np.dtype(dtype)
    raw, cuts = fixture_streams(chunkings, master, name, "f8")
    raw, cuts = raw[2:], cuts[2:]  # 321, 803, 1500 and 4000 samples
    pcm = [np.rint(x).astype(np.int16) for x in raw]
    pre = [Preemphasize(0.97).apply(x.astype(dtype)) for x in pcm]
    assert all(p.dtype == dtype for p in pre)
    statics = private(("composition", dtype.str), name, pre, cuts)
    deltas = Deltas(2)
    comp = build(name)
    with SiStreamBatch(comp, capacity=4, dtype=dtype, deltas=deltas, preemphasis=0.97) as sb:
        H = sb.lookahead
        assert H == 4 and sb.num_coeffs == 3 * comp.num_coeffs
        got = drive(sb, pcm, cuts, [3, 1, 0, 2])
    for i in range(4):
        X = np.concatenate(statics[i])
        seen = np.cumsum([len(o) for o in statics[i]])
        given = np.cumsum([len(o) for o in got[i]])
        # delayed by the look-ahead, completed by finalize
        assert given[:-1].tolist() == np.maximum(0, seen[:-1] - H).tolist() and given[-1] == len(X), i
        rows = np.concatenate(got[i])
        assert rows.dtype == dtype
        if len(X):
            assert np.array_equal(rows, deltas.apply(X, axis=0)), i
    assert len(np.concatenate(statics[3])) > 2 * H


def test_memory_and_close():
    comp = build("s6_fbank_long")
    for dtype in (np.float32, np.float64):
        sb = SiStreamBatch(comp, capacity=16, dtype=dtype)
        row = max(comp._max_support - 1, comp._skip0) + 2 * comp.frame_shift
        assert sb.state.row_length == row
        assert sb._pool.numel() * sb._pool.element_size() == 2 * 16 * row * np.dtype(dtype).itemsize
        assert sb._prev is None and "deltas" not in sb._stages
        sb.close()
        assert sb._pool is None
        for use in (lambda: sb.compute_chunks([0], [np.zeros(10, dtype)]), lambda: sb.finalize([0]),
                    lambda: sb.finalize_packed([0]), lambda: sb.started([0])):
            with pytest.raises(ValueError, match="closed"):
                use()
