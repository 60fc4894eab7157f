"""The host side of sliding-window CMVN (CPU only): the ``SlidingCMVN`` arguments and aliases, what batched streaming
refuses, ``SlidingState`` and its metadata fed to a numpy emulation of the streaming kernel (ring included) over random
tick schedules, the upload layout, and the second library's header against its signature table."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

from pydrobert_speech_amd import _native
from pydrobert_speech_amd import post as post_module
from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg
from pydrobert_speech_amd.multistream import SlidingState, StreamBatch, _tick_layout, streaming_sliding_cmvn
from pydrobert_speech_amd.multistream_si import SiStreamBatch
from pydrobert_speech_amd.post import Deltas, PostProcessor, SlidingCMVN, Standardize
from tests.conftest import ROOT
from tests.sliding_model import same_bits, sliding_cmvn
from tests.test_multistream_host import build, golden_configs

FLAG_FRESH = 1

# ---- 1. the post-processor's arguments ----------------------------------------------------------------------------


def test_aliases_and_json_construction():
    assert "SlidingCMVN" in post_module.__all__
    for alias in ("sliding_cmvn", "cmvn_sliding", "sliding"):
        inst = alias_factory_subclass_from_arg(PostProcessor, alias)
        assert type(inst) is SlidingCMVN
        assert (inst.cmn_window, inst.min_window, inst.center, inst.norm_vars, inst.refresh) == (600, 100, False, False, 600)
    inst = alias_factory_subclass_from_arg(
        PostProcessor, {"name": "sliding_cmvn", "cmn_window": 300, "min_window": 50, "center": True, "norm_vars": True})
    assert (inst.cmn_window, inst.min_window, inst.center, inst.norm_vars, inst.refresh) == (300, 50, True, True, 300)
    inst = alias_factory_subclass_from_arg(PostProcessor, {"alias": "sliding", "cmn_window": 8, "refresh": 3})
    assert (inst.cmn_window, inst.refresh) == (8, 3)
    assert SlidingCMVN(np.int64(7), np.int32(2), np.bool_(True)).cmn_window == 7
    # the older normalisation keeps its aliases
    assert type(alias_factory_subclass_from_arg(PostProcessor, "cmvn")) is Standardize


@pytest.mark.parametrize("kwargs", [
    dict(cmn_window=0), dict(cmn_window=-3), dict(cmn_window=2.0), dict(cmn_window="600"), dict(cmn_window=True),
    dict(cmn_window=None), dict(cmn_window=1 << 31), dict(min_window=0), dict(min_window=1.5), dict(min_window=False),
    dict(center=1), dict(center="yes"), dict(center=None), dict(norm_vars=0), dict(norm_vars="no"), dict(refresh=0),
    dict(refresh=-1), dict(refresh=2.5), dict(refresh=True)])
def test_arguments_are_positive_integers_or_bools(kwargs):
    with pytest.raises(ValueError):
        SlidingCMVN(**kwargs)


# ---- 2. what batched streaming refuses ----------------------------------------------------------------------------


def test_streaming_refusals():
    ok = SlidingCMVN(4, 1)
    assert streaming_sliding_cmvn(ok) is ok and streaming_sliding_cmvn(None) is None
    made = streaming_sliding_cmvn({"name": "sliding_cmvn", "cmn_window": 9, "min_window": 1, "refresh": 2})
    assert type(made) is SlidingCMVN and (made.cmn_window, made.refresh) == (9, 2)
    comp = build(golden_configs()["c1_kaldi_fbank"])
    si = build({"name": "si", "bank": {"name": "gabor", "scaling_function": "mel"}})
    for bad, why in ((SlidingCMVN(4, 1, center=True), "future"), (SlidingCMVN(4, 2), "wait"), (SlidingCMVN(), "wait"),
                     ("sliding_cmvn", "wait"), ({"name": "sliding", "min_window": 1, "center": True}, "future")):
        with pytest.raises(ValueError, match=why):
            streaming_sliding_cmvn(bad)
        for cls, c in ((StreamBatch, comp), (SiStreamBatch, si)):
            with pytest.raises(ValueError, match=why):  # (before anything touches a device)
                cls(c, capacity=4, sliding_cmvn=bad)
    for bad in (Standardize(), "cmvn", Deltas(2), 600, {"cmn_window": 4}, {"name": "sliding", "cmn_window": 0}):
        with pytest.raises(ValueError):
            streaming_sliding_cmvn(bad)
        with pytest.raises(ValueError):
            StreamBatch(comp, capacity=4, sliding_cmvn=bad)
    for cls, c in ((StreamBatch, comp), (SiStreamBatch, si)):
        with pytest.raises(ValueError, match="one of them"):
            cls(c, capacity=4, cmvn=Standardize(), sliding_cmvn=ok)
    # what is no Standardize is still refused as `cmvn`, a SlidingCMVN included
    for bad in (Deltas(2), ok, "sliding_cmvn"):
        with pytest.raises(ValueError, match="Standardize"):
            StreamBatch(comp, capacity=4, cmvn=bad)
    for args in ((0, 4), (4, 0), (4, 4, 0)):
        with pytest.raises(ValueError):
            SlidingState(*args)


# ---- 3. SlidingState and the streaming kernel's walk --------------------------------------------------------------


def emulate_tick(ring, sums, wstate, ids, fresh_rows, final, norm_vars, dtype):
    """pds_multistream_sliding of one tick in numpy, from the metadata SlidingState.fill_meta writes
    (include/pds_amd_stages.h): `ring` is dtype[capacity, W + 1, F], `sums` float64[capacity, 2, F], `fresh_rows` the
    list of the streams' new static rows.  Returns each stream's normalised rows and advances `ring`, `sums` and
    `wstate`."""
    W, refresh = wstate.window, wstate.refresh
    slots = W + 1
    F = ring.shape[-1]
    ids = np.asarray(ids, dtype=np.int64)
    k = np.asarray([len(x) for x in fresh_rows], dtype=np.int64)
    statics = np.concatenate(fresh_rows).astype(dtype) if len(fresh_rows) else np.zeros((0, F), dtype=dtype)
    static_rows = np.concatenate([[0], np.cumsum(k)])
    step = wstate.step(ids, k, final=final)
    meta = np.full((len(ids), 8), -1, dtype=np.int64)
    wstate.fill_meta(meta, ids, step, static_rows[:-1])
    assert not meta[:, 5:].any()
    with np.errstate(all="ignore"):
        for s, flags, row, kk, t in meta[:, :5].tolist():
            assert flags in (0, FLAG_FRESH) and (flags == FLAG_FRESH) == (t == 0)
            if kk <= 0:
                continue
            if flags & FLAG_FRESH:
                s1, s2 = np.zeros(F), np.zeros(F)
            else:
                s1, s2 = sums[s, 0].copy(), sums[s, 1].copy()
            slot, phase = t % slots, t % refresh
            for r in range(kk):
                v = statics[row + r].copy()
                d = v.astype(np.float64)
                n = min(t, W) + 1
                if phase == 0:
                    s1, s2 = np.zeros(F), np.zeros(F)
                    q = (slot - (n - 1)) % slots
                    for _ in range(n - 1):
                        u = ring[s, q].astype(np.float64)
                        s1, s2 = s1 + u, s2 + u * u
                        q = (q + 1) % slots
                    s1, s2 = s1 + d, s2 + d * d
                else:
                    if t > W:
                        u = ring[s, slot].astype(np.float64)
                        s1, s2 = s1 - u, s2 - u * u
                    s1, s2 = s1 + d, s2 + d * d
                ring[s, slot] = v
                mean = s1 / float(n)
                y = d - mean
                if norm_vars:
                    if n == 1:
                        y = np.zeros(F)
                    else:
                        var = s2 / float(n) - mean * mean
                        y = y * (1.0 / np.sqrt(np.where(var > 1e-10, var, 1e-10)))
                statics[row + r] = y.astype(dtype)
                slot, phase, t = (slot + 1) % slots, (phase + 1) % refresh, t + 1
            sums[s, 0], sums[s, 1] = s1, s2
    wstate.commit(ids, step)
    return [statics[a:b] for a, b in zip(static_rows[:-1], static_rows[1:])]


@pytest.mark.parametrize("W,refresh,norm_vars,dtype", [(4, 3, False, np.float32), (4, 7, True, np.float64),
                                                      (3, 1, True, np.float32), (5, 1000, False, np.float64)])
def test_state_over_random_tick_schedules(W, refresh, norm_vars, dtype):
    B, F = 12, 3
    rng = np.random.default_rng(100 * W + refresh)
    post = SlidingCMVN(W, 1, False, norm_vars, refresh)
    wstate = SlidingState(B, post.cmn_window, post.refresh)
    assert wstate.fresh.all() and wstate.ring_rows == W + 1
    ring = rng.standard_normal((B, W + 1, F)).astype(dtype)  # (stale rows and sums must never be read)
    ring[::2] = np.nan
    sums = np.full((B, 2, F), np.nan)
    rows = [[] for _ in range(B)]  # the current life's statics and outputs
    outs = [[] for _ in range(B)]
    lives = empties = restarts = longest = 0
    ended = set()
    for _ in range(260):
        ids = np.flatnonzero(rng.random(B) < 0.5)
        rng.shuffle(ids)
        k = rng.integers(0, 6, size=len(ids))
        k[rng.random(len(ids)) < 0.4] = 0  # ticks without rows
        empties += int((k == 0).sum())
        new = [(20.0 + 5.0 * rng.standard_normal((kk, F))).astype(dtype) for kk in k]
        seen = np.asarray([sum(len(r) for r in rows[i]) for i in ids], dtype=np.int64)
        step = wstate.step(ids, k)
        assert (step["fresh"] == (seen == 0)).all() and (step["seen"] == seen).all()
        assert (wstate.seen[ids] == seen).all()  # (step changes nothing)
        for i, x, y in zip(ids.tolist(), new, emulate_tick(ring, sums, wstate, ids, new, False, norm_vars, dtype)):
            restarts += int(i in ended and not rows[i] and len(x) > 0)
            rows[i].append(x)
            outs[i].append(y)
        assert (wstate.seen[ids] == seen + k).all()
        fin = np.flatnonzero(rng.random(B) < 0.04)  # (ids are reused afterwards)
        rng.shuffle(fin)
        last = [(20.0 + 5.0 * rng.standard_normal((int(kk), F))).astype(dtype) for kk in rng.integers(0, 3, size=len(fin))]
        for i, x, y in zip(fin.tolist(), last, emulate_tick(ring, sums, wstate, fin, last, True, norm_vars, dtype)):
            X = np.concatenate(rows[i] + [x])
            got = np.concatenate(outs[i] + [y])
            want, _, _ = sliding_cmvn(X, W, 1, False, norm_vars, refresh)
            assert same_bits(got, want), (i, len(X))
            assert not np.isnan(got).any()
            longest = max(longest, len(X))
            rows[i], outs[i] = [], []
            ended.add(i)
            lives += 1
        assert wstate.fresh[fin].all()
    # utterances well past several wraps of the ring, streams restarted on their ids, ticks without rows
    assert lives > 20 and empties > 100 and restarts > 10 and longest > 6 * (W + 1)


def test_metadata_words():
    wstate = SlidingState(8, 4, 3)
    ids = np.asarray([5, 2, 7])
    step = wstate.step(ids, [2, 0, 4])
    wstate.commit(ids, step)
    step = wstate.step(ids, [1, 3, 0])
    meta = np.full((3, 8), 99, dtype=np.int64)
    wstate.fill_meta(meta, ids, step, np.asarray([0, 1, 4]))
    assert meta.tolist() == [[5, 0, 0, 1, 2, 0, 0, 0], [2, FLAG_FRESH, 1, 3, 0, 0, 0, 0], [7, 0, 4, 0, 4, 0, 0, 0]]
    wstate.commit(ids, step)
    assert wstate.seen[[5, 2, 7]].tolist() == [3, 3, 4]
    wstate.commit(ids[:1], wstate.step(ids[:1], [2], final=True))
    assert wstate.seen[[5, 2, 7]].tolist() == [0, 3, 4] and wstate.fresh[5]
    assert SlidingState(2, 9).refresh == 9  # (refresh defaults to the window)


# ---- 4. the upload --------------------------------------------------------------------------------------------------


def test_the_layout_without_the_stage_is_the_old_one():
    for n, E, chunks in ((5, 3, True), (5, 0, True), (4, 4, False), (0, 0, True)):
        for deltas in (False, True):
            for cmvn in (False, True):
                old = _tick_layout(n, E, 4, chunks, deltas, cmvn)
                assert _tick_layout(n, E, 4, chunks, deltas, cmvn, False, False, False) == old
                for stack in (False, True):
                    for dither in (False, True):
                        old = _tick_layout(n, E, 4, chunks, deltas, cmvn, stack, dither)
                        assert _tick_layout(n, E, 4, chunks, deltas, cmvn, stack, dither, False) == old
                        at, words = _tick_layout(n, E, 4, chunks, deltas, cmvn, stack, dither, True)
                        # the new section lies behind all the others and moves none of them
                        assert words == old[1] + 8 * n
                        assert at.pop("sliding") == (old[1], 8 * n, (n, 8), (8, 1)) and at == old[0]


# ---- 5. the second library's binding --------------------------------------------------------------------------------


def test_stages_header_and_signature_table_name_the_same_set():
    with open(os.path.join(ROOT, "include", "pds_amd_stages.h")) as fh:
        header = fh.read()
    declared = set(re.findall(r"\b(pds_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_native.STAGES_SIGNATURES), declared ^ set(_native.STAGES_SIGNATURES)
    assert {"pds_stages_version", "pds_stages_last_error"} <= declared
    assert not declared & set(_native.SIGNATURES)  # (the first library's table gained nothing)
    for name in ("pds_sliding_cmvn_rows_f32", "pds_sliding_cmvn_rows_f64"):
        restype, argtypes = _native.STAGES_SIGNATURES[name]
        assert restype is ctypes.c_int32 and len(argtypes) == 15
    for name in ("pds_multistream_sliding_f32", "pds_multistream_sliding_f64"):
        restype, argtypes = _native.STAGES_SIGNATURES[name]
        assert restype is ctypes.c_int32 and len(argtypes) == 11
    assert "int32_t pds_multistream_sliding_f32(float *d_statics, float *d_ring, double *d_sums, int64_t capacity," in header


def test_stages_library_exports_every_declared_symbol():
    lib = _native.stages_lib()  # (NativeError if it was not built: there is no fallback)
    for name in _native.STAGES_SIGNATURES:
        assert getattr(lib, name) is not None
    assert lib.pds_stages_version() >= 100
    assert isinstance(lib.pds_stages_last_error(), bytes)
    # argument errors are reported before any HIP call, through the library's own error string
    assert lib.pds_sliding_cmvn_rows_f32(None, 4, None, None, 2, 5, 4, 0, 1, 0, 0, 1, None, 4, None) == -1
    assert b"positive" in lib.pds_stages_last_error()
    assert lib.pds_sliding_cmvn_rows_f32(None, 4, None, None, 2, 5, 4, 3, 1, 0, 0, 1, None, 4, None) == -1
    assert b"null pointer" in lib.pds_stages_last_error()
    assert lib.pds_sliding_cmvn_rows_f64(None, 3, None, None, 2, 5, 4, 3, 1, 0, 0, 1, None, 4, None) == -1
    assert b"stride" in lib.pds_stages_last_error()
    assert lib.pds_sliding_cmvn_rows_f64(None, 4, None, None, 0, 5, 4, 3, 1, 0, 0, 1, None, 4, None) == 0
    assert lib.pds_sliding_cmvn_rows_f64(None, 1 << 20, None, None, 1 << 30, 1 << 40, 1 << 20, 3, 1, 0, 0, 1, None,
                                         1 << 20, None) == -1
    assert b"too many lanes" in lib.pds_stages_last_error()
    assert lib.pds_multistream_sliding_f32(None, None, None, 4, 3, 4, 0, 4, None, 0, None) == 0
    assert lib.pds_multistream_sliding_f32(None, None, None, 4, 3, 4, 0, 4, None, 2, None) == -1
    assert lib.pds_multistream_sliding_f64(None, None, None, 4, 0, 4, 0, 4, None, 2, None) == -1
    with pytest.raises(ValueError, match="multistream_sliding"):
        _native.check_stages(-1, "pds_multistream_sliding")


def test_the_first_header_is_the_one_it_was():
    """include/pds_amd.h byte for byte as before the stages library: its entry points live in a header of their own
    (a change of pds_amd.h that is meant brings its new digest here)"""
    with open(os.path.join(ROOT, "include", "pds_amd.h"), "rb") as fh:
        data = fh.read()
    assert b"sliding" not in data and b"pds_stages" not in data
    assert hashlib.sha256(data).hexdigest() == "4a7234611063b1cc40841f1201883cb0246e7f92200260f33a031d551fc960f8"
