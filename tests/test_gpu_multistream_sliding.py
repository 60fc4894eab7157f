"""The sliding-window CMVN stage of batched streaming on the GPU (``StreamBatch(sliding_cmvn=...)``,
``SiStreamBatch(sliding_cmvn=...)``).

A stream's rows, concatenated over its calls, are ``SlidingCMVN.apply`` of its whole statics, bit for bit -- the
statics being the rows of a batch built without any post stage and given the same chunks -- whatever the cuts: ticks
bring a stream no row, one row or several, and two streams are finalized and restarted on their ids while the others
run on.  With `cepstra` in front and `deltas` and `stack` behind the rows are the offline chain's."""
import functools

import numpy as np
import pytest

from pydrobert_speech_amd.multistream import StreamBatch
from pydrobert_speech_amd.multistream_si import SiStreamBatch
from pydrobert_speech_amd.post import Cepstra, Deltas, SlidingCMVN, Stack
from tests.sliding_model import same_bits, sliding_cmvn
from tests.test_gpu_multistream import build
from tests.test_gpu_multistream_si import build as build_si
from tests.test_multistream_host import golden_configs

pytestmark = pytest.mark.gpu

IDS = [4, 0, 7, 2, 5, 3]  # the six streams; one sits on capacity - 1
CAPACITY = 8
# samples per utterance: 1, 4, 9, 16, 23 and 30 frames of the STFT computer; streams 1 and 3 then run a second one
LENGTHS = [[160], [700, 1000], [1500], [2600, 2000], [3700], [4800]]
FIRST_FRAMES = [1, 4, 9, 16, 23, 30]
W = 4
DTYPES = [np.float32, np.float64]
SI_CONFIG = {"name": "si", "bank": {"name": "fbank", "num_filts": 40}}


@functools.lru_cache(maxsize=None)
def computer(kind):
    if kind == "si":
        return build_si(SI_CONFIG)
    comp = build(golden_configs()["c1_kaldi_fbank"])  # 40 filters, no energy
    assert comp.num_coeffs == 40
    return comp


@functools.lru_cache(maxsize=None)
def signals(dtype):
    """per stream the utterances it runs, one after the other (int16: 16-bit PCM)"""
    rng = np.random.default_rng(21)
    return tuple(tuple(np.clip(np.rint(3000 * rng.standard_normal(n)), -32768, 32767).astype(dtype) for n in ns)
                 for ns in LENGTHS)


def pieces_of(x, seed):
    """an irregular cutting with empty chunks in it: ticks bring a stream 0, 1 and several frames"""
    rng = np.random.default_rng(seed)
    cuts = [0]
    while cuts[-1] < len(x):
        step = int(rng.choice([0, 0, 1, 37, 160, 161, 399, 400, 401, 1000]))
        cuts.append(min(len(x), cuts[-1] + step))
    return [x[a:b] for a, b in zip(cuts[:-1], cuts[1:])] + [x[:0]]


def drive(sb, dtype, packed=False):
    """every stream gets the chunks of its utterances, one per tick; a stream whose utterance is over is finalized in a
    tick of its own while the others run on, and starts its next utterance, if it has one, on the same id.  Returns
    ``{(stream index, utterance): rows}`` and the row counts the ticks brought"""
    import torch

    queues = [[pieces_of(x, 100 * i + u) for u, x in enumerate(utts)] for i, utts in enumerate(signals(dtype))]
    at = [[0, 0] for _ in IDS]  # per stream: utterance, piece
    got, brought = {}, []

    def take(key, rows):
        got.setdefault(key, []).append(rows)

    while True:
        live = [i for i in range(len(IDS)) if at[i][0] < len(queues[i])]
        if not live:
            break
        chunks = [queues[i][at[i][0]][at[i][1]] for i in live]
        ids = [IDS[i] for i in live]
        if packed:
            d = torch.from_numpy(np.concatenate(chunks)).cuda()
            feats, rows = sb.compute_chunks_packed(ids, d, [len(c) for c in chunks])
            host = feats.cpu().numpy()
            outs = [host[a:b] for a, b in zip(rows[:-1], rows[1:])]
        else:
            outs = sb.compute_chunks(ids, chunks)
        for i, o in zip(live, outs):
            assert o.shape[1] == sb.num_coeffs
            take((i, at[i][0]), o)
            brought.append(len(o))
            at[i][1] += 1
        over = [i for i in live if at[i][1] == len(queues[i][at[i][0]])]
        if over:
            ids = [IDS[i] for i in over]
            if packed:
                feats, rows = sb.finalize_packed(ids)
                host = feats.cpu().numpy()
                outs = [host[a:b] for a, b in zip(rows[:-1], rows[1:])]
            else:
                outs = sb.finalize(ids)
            assert not sb.started(ids).any()
            for i, o in zip(over, outs):
                take((i, at[i][0]), o)
                at[i] = [at[i][0] + 1, 0]
    work = np.float32 if sb.dtype == np.float32 else np.float64
    return {key: np.concatenate([r.astype(work) if not len(r) else r for r in rows]) for key, rows in got.items()}, brought


@functools.lru_cache(maxsize=None)
def statics(kind, dtype, sample_dtype=None, packed=False):
    """the rows of a batch without any post stage, per (stream, utterance): computed once per case, left unchanged"""
    cls = StreamBatch if kind == "stft" else SiStreamBatch
    with cls(computer(kind), capacity=CAPACITY, dtype=dtype) as sb:
        rows, brought = drive(sb, sample_dtype or dtype, packed)
    assert len(rows) == 8 and min(len(x) for x in rows.values()) >= 1
    assert 0 in brought and max(brought) >= 2
    if kind == "stft":
        assert [len(rows[i, 0]) for i in range(len(IDS))] == FIRST_FRAMES and 1 in brought
        assert max(len(x) for x in rows.values()) == 30
    return rows


@pytest.mark.parametrize("norm_vars", [False, True], ids=["mean", "meanvar"])
@pytest.mark.parametrize("refresh", [3, 7])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_are_the_offline_rows(dtype, refresh, norm_vars):
    post = SlidingCMVN(W, 1, False, norm_vars, refresh)
    with StreamBatch(computer("stft"), capacity=CAPACITY, dtype=dtype, sliding_cmvn=post) as sb:
        assert sb.num_coeffs == 40 and sb.lookahead == 0 and sb.num_vectors == 1
        got, _ = drive(sb, dtype)
        assert sb.wstate.fresh.all()  # (every stream is finalized)
    ref = statics("stft", dtype)
    assert got.keys() == ref.keys()
    for key, x in ref.items():
        want = post.apply(x)
        assert want.dtype == dtype and same_bits(got[key], want), key
        assert same_bits(want, sliding_cmvn(x, W, 1, False, norm_vars, refresh)[0]), key  # ... which is the model's


@pytest.mark.parametrize("refresh", [3, 7])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_whole_chain_is_the_offline_chain(dtype, refresh):
    ceps, post, deltas, stack = Cepstra(13), SlidingCMVN(W, 1, False, True, refresh), Deltas(2), Stack(3)
    spec = {"name": "sliding_cmvn", "cmn_window": W, "min_window": 1, "norm_vars": True, "refresh": refresh}
    with StreamBatch(computer("stft"), capacity=CAPACITY, dtype=dtype, cepstra=ceps, sliding_cmvn=spec, deltas=Deltas(2),
                     stack=Stack(3)) as sb:
        assert sb.num_coeffs == 3 * 3 * 13 and sb.lookahead == 4 and sb.num_vectors == 3
        got, _ = drive(sb, dtype)
    for key, x in statics("stft", dtype).items():
        want = stack.apply(deltas.apply(post.apply(ceps.apply(x)), axis=0))
        assert want.shape == (len(x) // 3, 117)
        assert same_bits(got[key], want), key


def test_short_integration_streams():
    dtype = np.float64
    post = SlidingCMVN(W, 1, refresh=3)
    with SiStreamBatch(computer("si"), capacity=CAPACITY, dtype=dtype, sliding_cmvn=post) as sb:
        assert sb.num_coeffs == 40
        got, _ = drive(sb, dtype)
    rows = 0
    for key, x in statics("si", dtype).items():
        assert same_bits(got[key], post.apply(x)), key
        rows += len(x)
    assert rows > 60


def test_packed_int16_chunks():
    dtype = np.float32
    post = SlidingCMVN(W, 1, False, True, 7)
    with StreamBatch(computer("stft"), capacity=CAPACITY, dtype=dtype, sliding_cmvn=post) as sb:
        got, _ = drive(sb, np.int16, packed=True)
    for key, x in statics("stft", dtype, np.int16, True).items():
        assert same_bits(got[key], post.apply(x)), key


def test_a_tick_without_rows_launches_nothing_and_keeps_the_state():
    dtype = np.float32
    post = SlidingCMVN(W, 1, refresh=3)
    x = signals(dtype)[5][0]
    with StreamBatch(computer("stft"), capacity=CAPACITY, dtype=dtype, sliding_cmvn=post) as sb, \
            StreamBatch(computer("stft"), capacity=CAPACITY, dtype=dtype) as plain:
        cuts = [0, 2000, 2000, 2010, 4800]
        outs, refs = [], []
        for a, b in zip(cuts[:-1], cuts[1:]):
            outs.append(sb.compute_chunks([6], [x[a:b]])[0])
            refs.append(plain.compute_chunks([6], [x[a:b]])[0])
        assert [len(o) for o in outs][1:3] == [0, 0] and sb.wstate.seen[6] == sum(len(o) for o in outs)
        outs.append(sb.finalize([6])[0])
        refs.append(plain.finalize([6])[0])
    assert same_bits(np.concatenate(outs), post.apply(np.concatenate(refs)))
