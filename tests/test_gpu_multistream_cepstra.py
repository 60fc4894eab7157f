"""The cepstra stage of batched streaming on the GPU (``StreamBatch(cepstra=...)``, ``SiStreamBatch(cepstra=...)``).

The stage is stateless and runs first, so a stream's rows are the offline chain over its whole utterance, byte for
byte: ``stack(deltas(cmvn(cepstra(statics))))`` with whichever stages are present, the statics being the rows of a
batch built without any of them.  A batch built without `cepstra` uploads what it uploaded before there was one."""
import functools

import numpy as np
import pytest

from pydrobert_speech_amd.multistream import StreamBatch, _tick_layout, streaming_cepstra
from pydrobert_speech_amd.multistream_si import SiStreamBatch
from pydrobert_speech_amd.post import Cepstra, Deltas, Stack, Standardize
from tests.test_gpu_multistream import build
from tests.test_gpu_multistream_si import build as build_si
from tests.test_multistream_cmvn_host import running_cmvn
from tests.test_multistream_host import golden_configs

pytestmark = pytest.mark.gpu

IDS = [4, 0, 7, 2, 5]  # the five streams; one sits on capacity - 1
CAPACITY = 8
LENGTHS = [0, 1, 399, 4000, 16001]
CUTTINGS = ["regular", "irregular"]
DTYPES = [np.float32, np.float64]
SI_CONFIG = {"name": "si", "bank": {"name": "fbank", "num_filts": 40}}


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def computer():
    comp = build(golden_configs()["c1_kaldi_fbank"])  # 40 filters, no energy
    assert comp.num_coeffs == 40
    return comp


@functools.lru_cache(maxsize=None)
def signals(dtype):
    rng = np.random.default_rng(11)
    return tuple((3000 * rng.standard_normal(n)).astype(dtype) for n in LENGTHS)


def pieces_of(x, cutting):
    """a signal's chunks: 160 samples each, or an irregular cutting with empty chunks in it"""
    if cutting == "regular":
        return [x[a : a + 160] for a in range(0, len(x), 160)] or [x]
    rng = np.random.default_rng(len(x) + 1)
    cuts = [0]
    while cuts[-1] < len(x):
        step = int(rng.choice([0, 0, 1, 37, 160, 161, 399, 400, 401, 1000, 2500]))
        cuts.append(min(len(x), cuts[-1] + step))
    out = [x[a:b] for a, b in zip(cuts[:-1], cuts[1:])] + [x[:0]]
    assert any(len(p) == 0 for p in out)
    return out


def drive(sb, dtype, cutting, ids=IDS):
    """every stream gets its chunks, one per tick, in the order of `ids`, then its finalize in a tick of its own kind;
    returns each stream's rows, concatenated over its calls"""
    chunks = [pieces_of(x, cutting) for x in signals(dtype)]
    rows = [[] for _ in ids]
    for t in range(max(map(len, chunks))):
        live = [i for i in range(len(ids)) if t < len(chunks[i])]
        outs = sb.compute_chunks([ids[i] for i in live], [chunks[i][t] for i in live])
        for i, o in zip(live, outs):
            assert o.dtype == dtype and o.shape[1] == sb.num_coeffs
            rows[i].append(o)
    for i, o in enumerate(sb.finalize(ids)):
        rows[i].append(o if len(o) else o.astype(dtype))  # (a stream that never started returns float64 rows)
    return [np.concatenate(r) for r in rows]


@functools.lru_cache(maxsize=None)
def statics(kind, dtype, cutting):
    """the rows of a batch without any post stage, per stream: computed once per case and left unchanged"""
    if kind == "stft":
        sb = StreamBatch(computer(), capacity=CAPACITY, dtype=dtype)
    else:
        sb = SiStreamBatch(build_si(SI_CONFIG), capacity=CAPACITY, dtype=dtype)
    with sb:
        rows = drive(sb, dtype, cutting)
    assert len(rows[0]) == 0 and len(rows[3]) >= 24 and len(rows[4]) >= 99
    return tuple(rows)


@pytest.mark.parametrize("cutting", CUTTINGS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_are_cepstra_of_the_plain_rows(dtype, cutting):
    post = Cepstra(13)
    with StreamBatch(computer(), capacity=CAPACITY, dtype=dtype, cepstra=post) as sb:
        assert sb.num_coeffs == 13 and sb.lookahead == 0 and sb.num_vectors == 1
        got = drive(sb, dtype, cutting)
        assert not sb.started(IDS).any()
        # the streams are reused after their finalize, in another order
        again = drive(sb, dtype, cutting, ids=IDS[::-1])
    for g, a, x in zip(got, again, statics("stft", dtype, cutting)):
        want = post.apply(x)
        assert want.shape == (len(x), 13)
        assert same_bytes(g, want) and same_bytes(a, want)


@pytest.mark.parametrize("spec", ["mfcc", {"name": "dct", "num_ceps": 12, "lifter": 0, "energy": False}])
def test_configuration_forms(spec):
    post = streaming_cepstra(spec)
    assert isinstance(post, Cepstra) and streaming_cepstra(post) is post and streaming_cepstra(None) is None
    with StreamBatch(computer(), capacity=CAPACITY, cepstra=spec) as sb:
        got = drive(sb, np.float32, "regular")
    for g, x in zip(got, statics("stft", np.float32, "regular")):
        assert same_bytes(g, post.apply(x))


def test_constructor_refuses_what_is_no_cepstra():
    for bad in ("cmvn", Deltas(2), {"name": "mfcc", "norm": "x"}, 13, {"num_ceps": 13}):
        with pytest.raises(ValueError):
            StreamBatch(computer(), capacity=2, cepstra=bad)
    with pytest.raises(ValueError, match="num_ceps"):
        StreamBatch(computer(), capacity=2, cepstra=Cepstra(41))  # the width is known here
    prior = np.zeros((2, 41))
    prior[0, -1] = 3
    cmvn = Standardize()
    cmvn._stats = prior
    with pytest.raises(ValueError, match="statistics"):  # the statistics must have the cepstral width
        StreamBatch(computer(), capacity=2, cepstra=Cepstra(13), cmvn=cmvn)


@pytest.mark.parametrize("cutting", CUTTINGS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_whole_chain_is_the_offline_chain(dtype, cutting):
    post, deltas, stack = Cepstra(13), Deltas(2), Stack(3)
    with StreamBatch(computer(), capacity=CAPACITY, dtype=dtype, cepstra=post, cmvn=Standardize(), deltas=Deltas(2),
                     stack=Stack(3)) as sb:
        assert sb.num_coeffs == 3 * 3 * 13 and sb.lookahead == 4 and sb.num_vectors == 3
        tables = sb.cmvn_stats(IDS)
        assert tables.shape == (5, 2, 14) and not tables.any()
        got = drive(sb, dtype, cutting)
        assert not sb.cmvn_stats(IDS).any()  # (every stream is finalized)
    for g, x in zip(got, statics("stft", dtype, cutting)):
        ceps = post.apply(x)
        normed = running_cmvn(ceps)[0].astype(dtype)  # Standardize frame by frame: accumulate(x_t); apply(x_t)
        if len(x):
            want = stack.apply(deltas.apply(normed, axis=0))
        else:
            want = np.zeros((0, 117), dtype=dtype)
        assert want.shape == (len(x) // 3, 117)
        assert same_bytes(g, want)


def test_cmvn_stats_have_the_cepstral_width():
    dtype = np.float32
    post = Cepstra(13)
    x = signals(dtype)[4]
    with StreamBatch(computer(), capacity=CAPACITY, cepstra=post, cmvn=Standardize()) as sb, \
            StreamBatch(computer(), capacity=CAPACITY) as plain:
        out = sb.compute_chunks([3], [x])[0]
        ceps = post.apply(plain.compute_chunks([3], [x])[0])
        normed, table = running_cmvn(ceps)
        assert same_bytes(out, normed.astype(dtype))
        got = sb.cmvn_stats([3, 1])
        assert got.shape == (2, 2, 14) and np.array_equal(got[0], table) and not got[1].any()


def test_short_integration_streams():
    dtype = np.float64
    post = Cepstra(13, norm=None)
    comp = build_si(SI_CONFIG)
    assert comp.num_coeffs == 40
    with SiStreamBatch(comp, capacity=CAPACITY, dtype=dtype, cepstra=post, deltas=Deltas(1)) as sb:
        assert sb.num_coeffs == 26 and sb.lookahead == 2
        got = drive(sb, dtype, "irregular")
    rows = 0
    for g, x in zip(got, statics("si", dtype, "irregular")):
        ceps = post.apply(x)
        want = Deltas(1).apply(ceps, axis=0) if len(x) else np.zeros((0, 26), dtype=dtype)
        assert same_bytes(g, want)
        rows += len(x)
    assert rows > 100


def documented_words(n, E, launch_rows, chunks, deltas, cmvn, stack, dither):
    """the words of a tick's upload behind the samples, from the sections the module documents: assemble metadata
    ``n x 8`` and tile prefix ``n + 1`` (a ``compute_chunks`` tick), launch metadata ``rows x E``, deltas metadata
    ``n x 8`` and element prefix ``n + 1``, cmvn metadata ``n x 8``, stack metadata ``n x 8`` and element prefix
    ``n + 1``, two words per stream for the dither (a ``compute_chunks`` tick)"""
    words = launch_rows * E
    if chunks:
        words += 8 * n + n + 1
    if deltas:
        words += 8 * n + n + 1
    if cmvn:
        words += 8 * n
    if stack:
        words += 8 * n + n + 1
    if dither and chunks:
        words += 2 * n
    return words


def test_the_upload_is_what_it_was(monkeypatch):
    # the stage has no metadata: the layout function takes no argument for it, and what a tick asks of it -- with and
    # without `cepstra` -- is the documented sections and nothing else
    from pydrobert_speech_amd import multistream

    for n, E, chunks in ((5, 3, True), (5, 0, True), (4, 4, False), (0, 0, True)):
        for deltas in (False, True):
            for cmvn in (False, True):
                for stack in (False, True):
                    for dither in (False, True):
                        _, words = _tick_layout(n, E, 4, chunks, deltas, cmvn, stack, dither)
                        assert words == documented_words(n, E, 4, chunks, deltas, cmvn, stack, dither)
    asked = []
    real = multistream._tick_layout

    def spy(*args):
        asked.append(args)
        return real(*args)

    monkeypatch.setattr(multistream, "_tick_layout", spy)
    x = signals(np.float32)
    per_kind = {}
    for kind, kwargs in (("plain", {}), ("cepstra", dict(cepstra=Cepstra(13))),
                         ("chain", dict(cmvn=Standardize(), deltas=Deltas(2), stack=Stack(3))),
                         ("cepstra_chain", dict(cepstra=Cepstra(13), cmvn=Standardize(), deltas=Deltas(2),
                                                stack=Stack(3)))):
        del asked[:]
        with StreamBatch(computer(), capacity=CAPACITY, **kwargs) as sb:
            sb.compute_chunks([1, 6], [x[3], x[2]])
            sb.compute_chunks([6], [x[1]])
            sb.finalize([6, 1, 0])
        per_kind[kind] = list(asked)
        assert len(asked) == 3
    assert per_kind["plain"] == per_kind["cepstra"] and per_kind["chain"] == per_kind["cepstra_chain"]
    # ... and the batch without the stage asks for what it asked before: the documented sections of its n streams,
    # four launch rows, no section of a stage it does not have
    for kind, stages in (("plain", False), ("chain", True)):
        assert [a[0] for a in per_kind[kind]] == [2, 1, 3]
        for a, chunks in zip(per_kind[kind], (True, True, False)):
            n, E = a[:2]
            assert a == (n, E, 4, chunks, stages, stages, stages, False, False) and 0 <= E <= n
            assert real(*a)[1] == documented_words(n, E, 4, chunks, stages, stages, stages, False)
    assert per_kind["plain"][0][1] == 2  # (the two streams of the first tick emit frames)
