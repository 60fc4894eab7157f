"""Frame stacking of batched streaming on the host, no device (multistream.StackState, multistream.streaming_stack):
the row count of every call against post.Stack over the whole sequence, the index logic of pds_multistream_stack
(pending rows in a ping-pong pool, groups across ticks, the padded last group of a finalize) emulated in numpy from the
header's metadata contract alone, the constructor contract, the binding and the upload layout."""
import ctypes
import json
import os

import numpy as np
import pytest

from pydrobert_speech_amd import _native
from pydrobert_speech_amd.multistream import StackState, StreamBatch, _tick_layout, streaming_stack
from pydrobert_speech_amd.multistream_si import SiStreamBatch
from pydrobert_speech_amd.post import Deltas, Stack
from tests.conftest import GOLDEN
from tests.test_multistream_host import build, golden_configs

NVS = [1, 2, 3, 5]
FLAG_HALF, FLAG_FINAL = 1, 2
PAD_NONE, PAD_CONSTANT, PAD_EDGE = 0, 1, 2
# pad code of pds_multistream_stack, fill, and the post.Stack settings that mean the same
PADS = {
    "none": (PAD_NONE, 0.0, {}),
    "edge": (PAD_EDGE, 0.0, dict(pad_mode="edge")),
    "constant": (PAD_CONSTANT, -1.5, dict(pad_mode="constant", constant_values=-1.5)),
    "zeros": (PAD_CONSTANT, 0.0, dict(pad_mode="constant")),
}


def stack_totals(nv):
    """the total row counts at which a group fills, or the last one is partial"""
    return sorted({0, 1, nv - 1, nv, nv + 1, 2 * nv - 1, 2 * nv, 40})


def whole(X, nv, pad):
    """post.Stack over the whole sequence (the host numpy path)"""
    return Stack(nv, **PADS[pad][2]).apply(X, axis=-1)


def total_rows(T, nv, pad):
    return -(-T // nv) if pad != "none" else T // nv


# ---- 1. row counts ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("pad", ["none", "edge", "constant"])
@pytest.mark.parametrize("nv", NVS)
def test_row_counts_are_those_of_stack_over_the_whole_sequence(nv, pad):
    B = 16
    state = StackState(B, nv, pad=pad != "none")
    assert state.pool_rows == nv - 1
    rng = np.random.default_rng(10 * nv + len(pad))
    fed = [0] * B  # rows given / returned in the stream's current life
    got = [0] * B
    lives, partial = 0, 0
    for _ in range(150):
        ids = np.flatnonzero(rng.random(B) < 0.5)
        rng.shuffle(ids)
        m = rng.integers(0, 2 * nv + 3, size=len(ids))
        m[rng.random(len(ids)) < 0.3] = 0
        m[rng.random(len(ids)) < 0.3] = 1
        step = state.step(ids, m)
        assert (state.pending[ids] == step["pending"]).all()  # (step changes nothing)
        for i, mm, G, keep in zip(ids.tolist(), m.tolist(), step["groups"].tolist(), step["keep"].tolist()):
            fed[i] += mm
            assert G == fed[i] // nv - got[i] and keep == fed[i] % nv, (i, fed[i], got[i], G, keep)
            got[i] += G
        state.commit(ids, step)
        assert (state.pending[ids] == step["keep"]).all() and (state.pending < nv).all()
        fin = np.flatnonzero(rng.random(B) < 0.1)  # (ids are reused afterwards)
        rng.shuffle(fin)
        last = rng.integers(0, 3, size=len(fin))
        step = state.step(fin, last, final=True)
        for i, mm, G in zip(fin.tolist(), last.tolist(), step["groups"].tolist()):
            fed[i] += mm
            got[i] += G
            X = np.arange(fed[i] * 2, dtype=np.float64).reshape(fed[i], 2)
            assert got[i] == len(whole(X, nv, pad)) == total_rows(fed[i], nv, pad), (i, fed[i], got[i])
            partial += fed[i] % nv > 0
            fed[i] = got[i] = 0
            lives += 1
        assert not step["keep"].any()
        state.commit(fin, step)
        assert not state.pending[fin].any()
    assert lives > 20 and (partial > 5 or nv == 1)


# ---- 2. index logic against post.Stack ------------------------------------------------------------------------------


def emulate_tick(pool, nv, pad, fill, kstate, ids, fresh, final):
    """pds_multistream_stack of one tick in numpy, from the metadata StackState.fill_meta writes, as include/pds_amd.h
    states the contract: `pool` is float64[2, capacity, nv - 1, C], `fresh` the list of the streams' new rows.  Returns
    each stream's stacked rows and advances `pool` and `kstate`."""
    C = pool.shape[-1]
    ids = np.asarray(ids, dtype=np.int64)
    m = np.asarray([len(x) for x in fresh], dtype=np.int64)
    rows = np.concatenate(fresh) if len(fresh) else np.zeros((0, C))
    step = kstate.step(ids, m, final=final)
    out_rows = np.concatenate([[0], np.cumsum(step["groups"])])
    new_rows = np.concatenate([[0], np.cumsum(m)])
    meta = np.full((len(ids), 8), -1, dtype=np.int64)
    prefix = np.full(len(ids) + 1, -1, dtype=np.int64)
    total = kstate.fill_meta(meta, prefix, ids, step, new_rows[:-1], out_rows[:-1], C)
    out = np.full((int(out_rows[-1]), nv * C), np.nan)
    new_pool = pool.copy()
    elems = 0
    for e, (s, flags, r, mm, row, G, orow, reserved) in enumerate(meta.tolist()):
        half, fin = flags & FLAG_HALF, bool(flags & FLAG_FINAL)
        assert fin == final and reserved == 0 and flags in range(4) and 0 <= r < nv
        seq = np.concatenate([pool[half, s, :r], rows[row : row + mm]])
        V = len(seq)
        assert G * nv - V < nv and (fin and pad != PAD_NONE or G * nv <= V)
        keep = 0 if fin else V - G * nv
        assert prefix[e] == elems
        elems += (G * nv + keep) * C
        if G:
            shown = seq[: G * nv]
            if G * nv > V:
                tail = np.full((G * nv - V, C), fill) if pad == PAD_CONSTANT else np.repeat(seq[-1:], G * nv - V, axis=0)
                shown = np.concatenate([seq, tail])
            out[orow : orow + G] = shown.reshape(G, nv * C)
        if keep:
            new_pool[1 - half, s, :keep] = seq[G * nv :]
    assert total == elems == prefix[-1]
    pool[...] = new_pool
    kstate.commit(ids, step)
    assert not np.isnan(out).any()
    return [out[a:b] for a, b in zip(out_rows[:-1], out_rows[1:])]


def split_rows(total, nv, rng):
    """rows per compute_chunks call of a stream of `total` rows: runs of 0-row ticks, mostly one row, now and then more
    than a group"""
    ms, left = [0, 0], total
    while left:
        if rng.random() < 0.3:
            ms += [0] * int(rng.integers(1, 4))
        m = min(left, int(rng.choice([1, 1, 1, 2, nv - 1, nv, nv + 1, 2 * nv + 1])))
        ms.append(m)
        left -= m
    return ms + [0] * int(rng.integers(0, 3))


@pytest.mark.parametrize("pad", sorted(PADS))
@pytest.mark.parametrize("nv", NVS[1:])
def test_emulated_kernel_equals_whole_utterance_stack(nv, pad):
    C, B = 5, 16
    code, fill, _ = PADS[pad]
    rng = np.random.default_rng(100 * nv + len(pad))
    kstate = StackState(B, nv, pad=code != PAD_NONE)
    pool = rng.standard_normal((2, B, nv - 1, C))  # (stale rows must never be read)
    totals = stack_totals(nv)
    # two rounds over the same ids, the totals on other streams in the second, every tick naming its streams in a
    # random order
    sids = rng.permutation(B)[: len(totals)]
    saw_copy = saw_many = False
    for _ in range(2):
        order = rng.permutation(len(totals))
        plan = [(totals[t], split_rows(totals[t], nv, rng)) for t in order]
        X = [rng.standard_normal((total, C)) for total, _ in plan]
        at = [0] * len(plan)  # rows fed
        nxt = [0] * len(plan)  # calls made
        got = [[] for _ in plan]
        done = [False] * len(plan)
        while not all(done):
            live = [i for i in range(len(plan)) if not done[i]]
            tick = [i for i in live if rng.random() < 0.6] or live[:1]
            rng.shuffle(tick)
            feed = [i for i in tick if nxt[i] < len(plan[i][1])]
            fin = [i for i in tick if nxt[i] >= len(plan[i][1])]
            if feed:
                fresh = [X[i][at[i] : at[i] + plan[i][1][nxt[i]]] for i in feed]
                before = kstate.pending[sids[feed]].copy()
                for i, r, y in zip(feed, before, emulate_tick(pool, nv, code, fill, kstate, sids[feed], fresh, False)):
                    saw_copy |= r > 0 and len(y) == 0  # a tick that only moves pending rows to the other half
                    saw_many |= len(y) > 1
                    at[i] += plan[i][1][nxt[i]]
                    nxt[i] += 1
                    assert len(y) == at[i] // nv - sum(len(g) for g in got[i])
                    got[i].append(y)
            if fin:
                # the last rows arrive with the finalize, as the frames of StreamBatch.finalize do
                last = [X[i][at[i] :] for i in fin]
                for i, y in zip(fin, emulate_tick(pool, nv, code, fill, kstate, sids[fin], last, True)):
                    at[i] = len(X[i])
                    got[i].append(y)
                    done[i] = True
                assert not kstate.pending[sids[fin]].any()
        for i, (total, ms) in enumerate(plan):
            assert at[i] == total == sum(ms)
            rows = np.concatenate(got[i])
            want = whole(X[i], nv, pad)
            assert rows.shape == want.shape == (total_rows(total, nv, pad), nv * C), (nv, pad, total, ms)
            assert np.array_equal(rows, want), (nv, pad, total, ms)
    assert saw_copy and saw_many


def test_finalize_brings_its_own_rows():
    # finalize usually adds frames: they join the sequence before the last group is cut or padded
    nv, C = 3, 4
    rng = np.random.default_rng(5)
    for pad in sorted(PADS):
        code, fill, _ = PADS[pad]
        for total, last in [(1, 1), (nv + 1, 1), (2 * nv + 2, 2), (3, 3), (4, 0), (0, 0)]:
            kstate = StackState(4, nv, pad=code != PAD_NONE)
            pool = rng.standard_normal((2, 4, nv - 1, C))
            X = rng.standard_normal((total, C))
            got = emulate_tick(pool, nv, code, fill, kstate, [2], [X[: total - last]], False)
            got += emulate_tick(pool, nv, code, fill, kstate, [2], [X[total - last :]], True)
            assert np.array_equal(np.concatenate(got), whole(X, nv, pad)), (pad, total, last)


def test_metadata_words():
    kstate = StackState(8, 3, pad=True)
    ids = np.asarray([5, 2, 7])
    step = kstate.step(ids, [2, 0, 4])
    assert step["groups"].tolist() == [0, 0, 1] and step["keep"].tolist() == [2, 0, 1]
    kstate.commit(ids, step)
    assert kstate.pending[[5, 2, 7]].tolist() == [2, 0, 1] and kstate.half[[5, 2, 7]].tolist() == [1, 1, 1]
    step = kstate.step(ids, [2, 3, 0])
    meta = np.full((3, 8), 99, dtype=np.int64)
    prefix = np.full(4, 99, dtype=np.int64)
    total = kstate.fill_meta(meta, prefix, ids, step, np.asarray([0, 2, 5]), np.asarray([0, 1, 2]), 10)
    assert meta.tolist() == [[5, FLAG_HALF, 2, 2, 0, 1, 0, 0], [2, FLAG_HALF, 0, 3, 2, 1, 1, 0], [7, FLAG_HALF, 1, 0, 5, 0, 2, 0]]
    assert prefix.tolist() == [0, 40, 70, 80] and total == 80
    kstate.commit(ids, step)
    assert kstate.pending[[5, 2, 7]].tolist() == [1, 0, 1] and kstate.half[[5, 2, 7]].tolist() == [0, 0, 0]
    step = kstate.step(ids, [0, 0, 1], final=True)  # padded: a partial group counts, and nothing where nothing is left
    kstate.fill_meta(meta, prefix, ids, step, np.asarray([0, 0, 0]), np.asarray([0, 1, 1]), 10)
    assert meta.tolist() == [[5, FLAG_FINAL, 1, 0, 0, 1, 0, 0], [2, FLAG_FINAL, 0, 0, 0, 0, 1, 0], [7, FLAG_FINAL, 1, 1, 0, 1, 1, 0]]
    assert prefix.tolist() == [0, 30, 30, 60]
    kstate.commit(ids, step)
    assert not kstate.pending.any()
    drop = StackState(8, 3)
    drop.commit(ids, drop.step(ids, [2, 0, 4]))
    assert drop.step(ids, [0, 0, 1], final=True)["groups"].tolist() == [0, 0, 0]
    for bad in [(0, 3), (4, 0)]:
        with pytest.raises(ValueError):
            StackState(*bad)


# ---- 3. the constructor contract ----------------------------------------------------------------------------------


class _NoDevice:
    """stands in for _native while a constructor runs: a device or the library being asked for is an error"""

    @staticmethod
    def require_device():
        raise AssertionError("the device was touched")

    lib = require_device


def test_stack_settings_are_checked(monkeypatch):
    from pydrobert_speech_amd import multistream

    comp = build(golden_configs()["c1_kaldi_fbank"])
    si = build({"name": "si", "bank": {"name": "gabor", "scaling_function": "mel"}})
    bad = [
        Deltas(2),
        {"name": "deltas", "num_deltas": 2},
        Stack(3, time_axis=1),
        Stack(3, time_axis=-1),
        Stack(3, pad_mode="reflect"),
        Stack(3, pad_mode="wrap"),
        Stack(3, pad_mode="mean"),
        Stack(3, pad_mode="symmetric"),
        Stack(3, pad_mode=lambda vector, width, axis, kwargs: None),
        Stack(3, pad_mode="edge", constant_values=1.0),  # pad arguments
        Stack(3, constant_values=1.0),
        Stack(3, pad_mode="constant", constant_values=(0.0, 1.0)),
        Stack(3, pad_mode="constant", constant_values=[1.0]),
        Stack(3, pad_mode="constant", constant_values="1"),
        Stack(3, pad_mode="constant", end_values=1.0),
        Stack(3, pad_mode="constant", constant_values=1.0, stat_length=2),
        {"name": "stack", "num_vectors": 3, "pad_mode": "maximum"},
        {"name": "stack", "num_vectors": 3, "time_axis": 1},
        {"num_vectors": 3},
        3,
    ]
    monkeypatch.setattr(multistream, "_native", _NoDevice)
    for s in bad:
        with pytest.raises(ValueError):
            streaming_stack(s)
        with pytest.raises(ValueError):  # (before anything touches a device)
            StreamBatch(comp, capacity=4, stack=s)
        with pytest.raises(ValueError):
            SiStreamBatch(si, capacity=4, stack=s)
    with pytest.raises(ValueError) as info:
        streaming_stack(Stack(3, pad_mode="reflect"))
    assert "whole utterance" in str(info.value)
    good = [
        (Stack(3), (3, PAD_NONE, 0.0)),
        (Stack(2, time_axis=-2, pad_mode="edge"), (2, PAD_EDGE, 0.0)),
        (Stack(5, pad_mode="constant"), (5, PAD_CONSTANT, 0.0)),
        (Stack(4, 0, "constant", constant_values=-1), (4, PAD_CONSTANT, -1.0)),
        ({"name": "stack", "num_vectors": 3}, (3, PAD_NONE, 0.0)),
        (json.loads('{"alias": "stack", "num_vectors": 2, "pad_mode": "constant", "constant_values": 0.5}'),
         (2, PAD_CONSTANT, 0.5)),
    ]
    for s, want in good:
        inst, *rest = streaming_stack(s)
        assert isinstance(inst, Stack) and tuple(rest) == want
        with pytest.raises(AssertionError, match="the device was touched"):  # (accepted: the device comes next)
            StreamBatch(comp, capacity=4, stack=s)
    # num_vectors == 1 is accepted and means no stacking: no state
    assert streaming_stack(None) is None and streaming_stack(Stack(1)) is None
    assert streaming_stack({"name": "stack", "num_vectors": 1}) is None
    assert streaming_stack(Stack(1, pad_mode="edge")) is None
    with pytest.raises(ValueError):
        streaming_stack(Stack(1, pad_mode="reflect"))  # (still checked)


class _FakeTorch:
    """as much of torch as a constructor asks of it, with no device behind it"""

    float32, float64 = "f4", "f8"

    class cuda:
        @staticmethod
        def current_device():
            return 0

    @staticmethod
    def device(*args):
        return args

    @staticmethod
    def zeros(shape, **kwargs):
        return ("zeros", tuple(shape))

    @staticmethod
    def empty(shape, **kwargs):
        return ("empty", tuple(shape))


class _FakeLib:
    """a library from before the stage: it has no pds_multistream_stack_*"""

    pds_multistream_assemble_f32 = pds_multistream_assemble_f64 = None
    pds_multistream_deltas_f32 = pds_multistream_deltas_f64 = None
    pds_multistream_cmvn_f32, pds_multistream_cmvn_f64 = "cmvn_f32", "cmvn_f64"

    @staticmethod
    def pds_multistream_tile():
        return 1024


class _FakeLibWithStack(_FakeLib):
    pds_multistream_stack_f32, pds_multistream_stack_f64 = "stack_f32", "stack_f64"


class _FakeStagesLib:
    pds_multistream_sliding_f32, pds_multistream_sliding_f64 = "sliding_f32", "sliding_f64"


def fake_batch(monkeypatch, lib, torch=_FakeTorch, **kwargs):
    from pydrobert_speech_amd import multistream

    class Native:
        require_device = staticmethod(lambda: torch)
        stages_lib = staticmethod(lambda: _FakeStagesLib)

    Native.lib = staticmethod(lambda: lib)
    monkeypatch.setattr(multistream, "_native", Native)
    comp = build(golden_configs()["c2_tri_mel40"])
    monkeypatch.setattr(type(comp), "_native_plan", lambda self, device=None: None)
    monkeypatch.setattr(Deltas, "_filters_on", lambda self, device: (None, None))
    return comp, StreamBatch(comp, capacity=4, **kwargs)


def test_no_stack_builds_no_state_and_asks_for_no_symbol(monkeypatch):
    for stack in (None, Stack(1), {"name": "stack", "num_vectors": 1}):
        comp, sb = fake_batch(monkeypatch, _FakeLib, stack=stack)
        assert sb.kstate is None and "stack" not in sb._stages
        assert sb.num_vectors == 1 and sb.num_coeffs == comp.num_coeffs and sb.lookahead == 0
    with pytest.raises(AttributeError):
        fake_batch(monkeypatch, _FakeLib, stack=Stack(2))  # (a stale library is an error, not a fall-back)


def test_stack_sizes_the_pool_and_the_rows(monkeypatch):
    comp, sb = fake_batch(monkeypatch, _FakeLibWithStack, stack=Stack(3, pad_mode="edge"), deltas=Deltas(2),
                          dtype=np.float64)
    F = comp.num_coeffs
    assert isinstance(sb.kstate, StackState) and sb.kstate.nv == 3 and sb.kstate.pad
    assert sb.num_vectors == 3 and sb.num_coeffs == 3 * 3 * F and sb.lookahead == 4
    stage = sb._stages["stack"]
    assert stage.pools == {"pending": ("empty", (2, 4, 2, 3 * F))} and stage._fn == "stack_f64"
    sb.close()
    assert stage.pools == {}
    comp, sb = fake_batch(monkeypatch, _FakeLibWithStack, stack=Stack(2, pad_mode="constant", constant_values=0.1))
    stage = sb._stages["stack"]
    assert sb.num_coeffs == 2 * F and stage.pools == {"pending": ("empty", (2, 4, 1, F))} and stage._fn == "stack_f32"
    assert stage.fill == float(np.float32(0.1)) != 0.1 and not sb.kstate.half.any()  # (rounded to the batch dtype)


# ---- 4. the binding and the layout ----------------------------------------------------------------------------------


def test_native_table_and_header_have_the_entry_points():
    want = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_double, ctypes.c_void_p,
            ctypes.c_void_p]
    for name in ("pds_multistream_stack_f32", "pds_multistream_stack_f64"):
        restype, argtypes = _native.SIGNATURES[name]
        assert restype is ctypes.c_int32 and argtypes == want
    with open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "pds_amd.h")) as fh:
        header = " ".join(fh.read().split())
    for T in ("float", "double"):
        proto = (f"int32_t pds_multistream_stack_f{32 if T == 'float' else 64}(const {T} *d_rows, {T} *d_pool, "
                 "int64_t capacity, int32_t num_vectors, int32_t coeffs, const int64_t *d_meta, "
                 "const int64_t *d_elem_prefix, int32_t n, int64_t total_elems, int32_t pad, double fill, "
                 f"{T} *d_out, void *stream);")
        assert proto in header, proto


@pytest.mark.parametrize("chunks", [True, False])
@pytest.mark.parametrize("deltas", [True, False])
@pytest.mark.parametrize("cmvn", [True, False])
def test_layout_without_stack_is_the_six_argument_layout(chunks, deltas, cmvn):
    for n, E, launch_rows in [(5, 3, 4), (1, 1, 5), (0, 0, 4), (4, 0, 5)]:
        six = _tick_layout(n, E, launch_rows, chunks, deltas, cmvn)
        assert _tick_layout(n, E, launch_rows, chunks, deltas, cmvn, False) == six
        at, words = _tick_layout(n, E, launch_rows, chunks, deltas, cmvn, True)
        # with the stage: the same sections where they were, then the stack metadata and its element prefix
        assert list(at)[: len(six[0])] == list(six[0]) and all(at[name] == six[0][name] for name in six[0])
        assert list(at)[len(six[0]) :] == ["stack", "stack_elems"]
        assert at["stack"] == (six[1], 8 * n, (n, 8), (8, 1))
        assert at["stack_elems"] == (six[1] + 8 * n, n + 1, (n + 1,), (1,))
        assert words == six[1] + 8 * n + n + 1
