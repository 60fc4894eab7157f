"""The PCEN stage of batched streaming on the GPU (``StreamBatch(pcen=...)``, ``SiStreamBatch(pcen=...)``).

Five streams, seeded random cuts with empty chunks among them, float32, float64 and int16 chunks.  A stream's rows,
concatenated over its ticks and its ``finalize``, are ``PCEN.apply`` of its whole statics -- the rows of a batch built
without any post stage and given the same chunks -- bit for bit, whatever the cuts; with `cepstra`, `cmvn`, `deltas`
and `stack` behind the stage they are the offline chain's.  Two streams are finalized and restarted on their ids while
the others run on: the second utterance starts from ``M = E``.  ``pcen_smooth`` reads the model's last M, NaN for a
fresh stream, and ids a tick does not name keep their state."""
import functools

import numpy as np
import pytest

from pydrobert_speech_amd.multistream import StreamBatch
from pydrobert_speech_amd.multistream_si import SiStreamBatch
from pydrobert_speech_amd.post import PCEN, Cepstra, Deltas, Stack, Standardize
from tests.pcen_model import pcen_model, same_bits, within_tolerance
from tests.test_gpu_multistream import build
from tests.test_multistream_cmvn_host import running_cmvn
from tests.test_multistream_host import golden_configs

pytestmark = pytest.mark.gpu

IDS = [4, 0, 7, 2, 5]  # the five streams; one sits on capacity - 1
CAPACITY = 8
# samples per utterance: 1, 4, 9, 16 and 30 frames of the STFT computer; streams 1 and 3 then run a second one
LENGTHS = [[160], [700, 1000], [1500], [2600, 2000], [4800]]
DTYPES = [np.float32, np.float64]
SI_CONFIG = {"name": "si", "bank": {"name": "fbank", "num_filts": 40}, "use_log": False}


@functools.lru_cache(maxsize=None)
def computer(kind):
    if kind == "si":
        comp = build(SI_CONFIG)
    else:
        comp = build(dict(golden_configs()["c1_kaldi_fbank"], use_log=False))  # 40 filters, no energy, linear
    assert comp.num_coeffs == 40 and not comp._log
    return comp


@functools.lru_cache(maxsize=None)
def signals(dtype):
    """per stream the utterances it runs, one after the other (int16: 16-bit PCM)"""
    rng = np.random.default_rng(31)
    return tuple(tuple(np.clip(np.rint(3000 * rng.standard_normal(n)), -32768, 32767).astype(dtype) for n in ns)
                 for ns in LENGTHS)


def pieces_of(x, seed):
    """a seeded random cutting with empty chunks in it: ticks bring a stream 0, 1 and several frames"""
    rng = np.random.default_rng(seed)
    cuts = [0]
    while cuts[-1] < len(x):
        step = int(rng.choice([0, 0, 1, 37, 160, 161, 399, 400, 401, 1000]))
        cuts.append(min(len(x), cuts[-1] + step))
    return [x[a:b] for a, b in zip(cuts[:-1], cuts[1:])] + [x[:0]]


def drive(sb, dtype, packed=False, watch=None):
    """every stream gets the chunks of its utterances, one per tick; a stream whose utterance is over is finalized in a
    tick of its own while the others run on, and starts its next utterance, if it has one, on the same id.  Returns
    ``{(stream index, utterance): rows}`` and the row counts the ticks brought.  `watch`, if given, is called after
    every tick and finalize with the rows so far and every stream's (utterance, piece) position"""
    import torch

    queues = [[pieces_of(x, 100 * i + u) for u, x in enumerate(utts)] for i, utts in enumerate(signals(dtype))]
    at = [[0, 0] for _ in IDS]  # per stream: utterance, piece
    got, brought = {}, []
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
            got.setdefault((i, at[i][0]), []).append(o)
            brought.append(len(o))
            at[i][1] += 1
        if watch is not None:
            watch(got, at)
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
                got.setdefault((i, at[i][0]), []).append(o)
                at[i] = [at[i][0] + 1, 0]
            if watch is not None:
                watch(got, at)
    work = np.float32 if sb.dtype == np.float32 else np.float64
    return {key: np.concatenate([r.astype(work) if not len(r) else r for r in rows]) for key, rows in got.items()}, brought


@functools.lru_cache(maxsize=None)
def statics(kind, dtype, sample_dtype=None, packed=False):
    """the rows of a batch without any post stage, per (stream, utterance): computed once per case, left unchanged"""
    cls = StreamBatch if kind == "stft" else SiStreamBatch
    with cls(computer(kind), capacity=CAPACITY, dtype=dtype) as sb:
        rows, brought = drive(sb, sample_dtype or dtype, packed)
    assert len(rows) == 7 and min(len(x) for x in rows.values()) >= 1
    assert 0 in brought and max(brought) >= 2
    if kind == "stft":
        assert [len(rows[i, 0]) for i in range(len(IDS))] == [1, 4, 9, 16, 30] and 1 in brought
        assert all((x >= 0).all() for x in rows.values())  # linear energies
    return rows


@pytest.mark.parametrize("spec", [PCEN(), {"name": "pcen", "smooth": 0.2, "gain": 0.7, "bias": 5.0, "power": 0.3}],
                         ids=["default", "config"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_are_the_offline_rows(dtype, spec):
    post = spec if isinstance(spec, PCEN) else PCEN(**{k: v for k, v in spec.items() if k != "name"})
    with StreamBatch(computer("stft"), capacity=CAPACITY, dtype=dtype, pcen=spec) as sb:
        assert sb.num_coeffs == 40 and sb.lookahead == 0 and sb.num_vectors == 1
        assert np.isnan(sb.pcen_smooth(IDS)).all() and sb.pcen_smooth(IDS).shape == (5, 40)
        got, _ = drive(sb, dtype)
        assert sb.estate.fresh.all()  # (every stream is finalized)
        assert np.isnan(sb.pcen_smooth(list(range(CAPACITY)))).all()
    ref = statics("stft", dtype)
    assert got.keys() == ref.keys()
    for key, x in ref.items():
        want = post.apply(x, axis=0)
        assert want.dtype == dtype and same_bits(got[key], want), key  # the second utterances too: they start from M = E
        assert within_tolerance(want, pcen_model(post, x)[0]), key  # ... which is the model's


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_whole_chain_is_the_offline_chain(dtype):
    post, ceps, deltas, stack = PCEN(), Cepstra(13), Deltas(2), Stack(3)
    with StreamBatch(computer("stft"), capacity=CAPACITY, dtype=dtype, pcen="pcen", cepstra=ceps, cmvn=Standardize(),
                     deltas=Deltas(2), stack=Stack(3)) as sb:
        assert list(sb._stages) == ["pcen", "cepstra", "cmvn", "deltas", "stack"]
        assert sb.num_coeffs == 3 * 3 * 13 and sb.lookahead == 4 and sb.num_vectors == 3
        got, _ = drive(sb, dtype)
    for key, x in statics("stft", dtype).items():
        normed = running_cmvn(ceps.apply(post.apply(x, axis=0)))[0].astype(dtype)  # Standardize frame by frame
        want = stack.apply(deltas.apply(normed, axis=0))
        assert want.shape == (len(x) // 3, 117)
        assert same_bits(got[key], want), key


def test_short_integration_streams():
    dtype = np.float64
    post = PCEN(smooth=0.05)
    with SiStreamBatch(computer("si"), capacity=CAPACITY, dtype=dtype, pcen=post) as sb:
        assert sb.num_coeffs == 40
        got, _ = drive(sb, dtype)
    rows = 0
    for key, x in statics("si", dtype).items():
        assert same_bits(got[key], post.apply(x, axis=0)), key
        rows += len(x)
    assert rows > 60


def test_packed_int16_chunks():
    dtype = np.float32
    post = PCEN()
    with StreamBatch(computer("stft"), capacity=CAPACITY, dtype=dtype, pcen=post) as sb:
        got, _ = drive(sb, np.int16, packed=True)
    for key, x in statics("stft", dtype, np.int16, True).items():
        assert same_bits(got[key], post.apply(x, axis=0)), key


@pytest.mark.parametrize("dtype", DTYPES)
def test_pcen_smooth_follows_the_streams(dtype):
    """after every tick: a stream's M is the model's last M over the statics of its current utterance so far, NaN
    while it has none and after its finalize"""
    post = PCEN()
    ref = statics("stft", dtype)
    seen = {"live": 0, "fresh": 0}
    with StreamBatch(computer("stft"), capacity=CAPACITY, dtype=dtype, pcen=post) as sb:

        def watch(got, at):
            m = sb.pcen_smooth(IDS)
            assert m.shape == (5, 40) and m.dtype == np.float64
            for i in range(len(IDS)):
                u = at[i][0]  # the stream's current utterance (one that has not begun after a finalize)
                n = sum(len(r) for r in got.get((i, u), []))
                if n == 0:
                    assert np.isnan(m[i]).all() and sb.estate.fresh[IDS[i]], (i, u)
                    seen["fresh"] += 1
                else:
                    assert same_bits(m[i], pcen_model(post, ref[i, u][:n])[1][-1]), (i, u, n)
                    seen["live"] += 1

        drive(sb, dtype, watch=watch)
    assert seen["live"] > 20 and seen["fresh"] > 5


def test_ids_a_tick_does_not_touch_keep_their_state():
    dtype = np.float32
    post = PCEN()
    xs = signals(dtype)
    a, b = xs[4][0], xs[3][0]
    with StreamBatch(computer("stft"), capacity=CAPACITY, dtype=dtype, pcen=post) as sb, \
            StreamBatch(computer("stft"), capacity=CAPACITY, dtype=dtype) as plain:
        out_a = [sb.compute_chunks([6], [a[:2000]])[0]]
        ref_a = [plain.compute_chunks([6], [a[:2000]])[0]]
        m6 = sb.pcen_smooth([6])
        assert same_bits(m6[0], pcen_model(post, ref_a[0])[1][-1])
        # ticks that name other streams, a tick that brings stream 6 no row, a finalize of another stream
        out_b = [sb.compute_chunks([1, 3], [b[:900], b[:1300]])[1]]
        assert same_bits(sb.pcen_smooth([6]), m6)
        assert len(sb.compute_chunks([6], [a[2000:2000]])[0]) == 0 and len(sb.compute_chunks([6], [a[2000:2010]])[0]) == 0
        plain.compute_chunks([6], [a[2000:2010]])
        assert same_bits(sb.pcen_smooth([6]), m6)
        sb.finalize([1])
        assert same_bits(sb.pcen_smooth([6]), m6) and np.isnan(sb.pcen_smooth([1])).all()
        assert not np.isnan(sb.pcen_smooth([3])).any() and np.isnan(sb.pcen_smooth([0, 2])).all()
        out_a.append(sb.compute_chunks([6, 3], [a[2010:], b[1300:]])[0])
        ref_a.append(plain.compute_chunks([6], [a[2010:]])[0])
        out_a.append(sb.finalize([6])[0])
        ref_a.append(plain.finalize([6])[0])
        assert np.isnan(sb.pcen_smooth([6])).all()
        # the id starts anew: M = E at its first row
        again = sb.compute_chunks([6], [b[:700]])[0]
        first = plain.compute_chunks([6], [b[:700]])[0]
        assert len(first) >= 2 and same_bits(again, post.apply(first, axis=0))
        assert same_bits(sb.pcen_smooth([6])[0], pcen_model(post, first)[1][-1])
        with pytest.raises(ValueError, match="without pcen"):
            plain.pcen_smooth([6])
    whole = np.concatenate(ref_a)
    assert len(whole) == 30 and same_bits(np.concatenate(out_a), post.apply(whole, axis=0))
    del out_b


def test_a_computer_that_takes_logs_is_refused_on_the_device_too():
    logged = build(golden_configs()["c1_kaldi_fbank"])
    with pytest.raises(ValueError, match="PCEN takes linear energies"):
        StreamBatch(logged, capacity=CAPACITY, pcen=PCEN())
    with pytest.raises(ValueError, match="PCEN takes linear energies"):
        SiStreamBatch(build(dict(SI_CONFIG, use_log=True)), capacity=CAPACITY, pcen="pcen")
