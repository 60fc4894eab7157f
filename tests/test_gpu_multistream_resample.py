"""Rate conversion per stream across ticks (multistream_resample.ResampleBatch) on the GPU: whatever the cuts, a
stream's outputs over its calls and its ``finalize`` are ``Resample.apply`` of its whole signal bit for bit, tick by
tick as many as the model's due-count says; ids are reusable; and the batch feeds ``StreamBatch`` as it stands."""
import json

import numpy as np
import pytest

from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg
from pydrobert_speech_amd.compute import FrameComputer
from pydrobert_speech_amd.multistream import StreamBatch
from pydrobert_speech_amd.multistream_resample import ResampleBatch
from pydrobert_speech_amd.pre import Resample
from tests import resample_model as model

pytestmark = pytest.mark.gpu

RATE_PAIRS = [(3, 2), (2, 3), (44100, 16000)]
DTYPES = [np.float32, np.float64, np.int16]
FBANK = {"name": "stft", "bank": {"name": "fbank", "num_filts": 40}, "frame_length_ms": 25, "use_power": True}


def signal(rng, n, dtype):
    x = 3000 * rng.standard_normal(n)
    return np.rint(x).astype(np.int16) if dtype is np.int16 else x.astype(dtype)


class Driver:
    """one interface over the host-list and the packed calls"""

    def __init__(self, rb, packed):
        self.rb, self.packed = rb, packed

    def feed(self, ids, chunks):
        import torch

        if not self.packed:
            return self.rb.resample_chunks(ids, chunks)
        host = np.concatenate(chunks) if len(chunks) else np.zeros(0, self.rb.dtype)
        d_out, lens = self.rb.resample_chunks_packed(ids, torch.from_numpy(host).cuda(), [len(c) for c in chunks])
        return self.split(d_out, lens, len(ids))

    def finalize(self, ids):
        if not self.packed:
            return self.rb.finalize(ids)
        d_out, lens = self.rb.finalize_packed(ids)
        return self.split(d_out, lens, len(ids))

    def split(self, d_out, lens, n):
        import torch

        assert d_out.is_cuda and d_out.dim() == 1 and d_out.dtype == getattr(torch, self.rb.out_dtype.name)
        assert isinstance(lens, np.ndarray) and lens.dtype == np.int64 and len(lens) == n
        assert d_out.numel() == int(lens.sum())
        host = d_out.cpu().numpy()
        ends = np.cumsum(lens)
        return [host[e - k : e] for e, k in zip(ends.tolist(), lens.tolist())]


@pytest.mark.parametrize("packed", [False, True], ids=["host", "packed"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("rates", RATE_PAIRS, ids=lambda r: f"{r[0]}to{r[1]}")
def test_streams_equal_the_offline_call_whatever_the_cuts(rates, dtype, packed):
    rs = Resample(*rates)
    rng = np.random.default_rng(100 * rates[0] + rates[1] + 7 * packed)
    sizes = [0, 1, 2, 7, rs.max_taps - 2, rs.max_taps, 3 * rs.in_unit + 1]
    sids = [6, 1, 4, 0, 3]  # five streams of a batch of eight, of different lengths
    span = 3 * rs.in_unit + 1 + rs.max_taps
    lengths = [2 * span + 3, 2 * span + span // 2, 3 * span - 1, 3 * span + 10, 4 * span]
    out_dtype = np.float64 if dtype is np.float64 else np.float32

    def due(n):
        return model.due(n, rs.in_unit, rs.out_unit, rs.first, rs.ntaps)

    with ResampleBatch(rs, 8, dtype) as rb:
        drv = Driver(rb, packed)
        assert [len(y) for y in drv.finalize([7, 2])] == [0, 0]  # finalize of a fresh stream gives nothing
        for life in range(2):  # (the second utterance of every stream: nothing of the first may leak into it)
            sigs = [signal(rng, n + life, dtype) for n in lengths]
            want = [rs.apply(x) for x in sigs]
            pos, outs = [0] * 5, [[] for _ in sigs]
            tick = empties = partial = 0
            while any(pos[i] < len(sigs[i]) for i in range(5)):
                live = [i for i in range(5) if pos[i] < len(sigs[i])]
                if tick == 0:
                    part = list(live)
                elif tick == 1:
                    part = live[::2]
                else:
                    part = [i for i in live if rng.random() < 0.7] or live[:1]
                rng.shuffle(part)
                partial += 0 < len(part) < len(live)
                chunks = []
                for i in part:
                    c = 0 if (tick == 0 and i == part[1]) else min(int(rng.choice(sizes)), len(sigs[i]) - pos[i])
                    chunks.append(sigs[i][pos[i] : pos[i] + c])
                    pos[i] += c
                    empties += c == 0
                got = drv.feed([sids[i] for i in part], chunks)
                for i, y in zip(part, got):
                    assert y.dtype == out_dtype
                    outs[i].append(y)
                    # after every tick a stream has emitted the model's due-count of what it has been given
                    assert sum(map(len, outs[i])) == due(pos[i]), (life, tick, i, pos[i])
                seen, emitted = rb.pending([sids[i] for i in part])
                assert seen.tolist() == [pos[i] for i in part]
                assert emitted.tolist() == [sum(map(len, outs[i])) for i in part]
                tick += 1
            assert empties > 0 and partial > 0 and tick > 8
            for i, y in zip(range(5), drv.finalize(sids)):
                outs[i].append(y)
                assert len(y) == model.num_output_samples(len(sigs[i]), *rates) - due(len(sigs[i])) > 0
            assert all(v == 0 for v in np.concatenate(rb.pending(sids)).tolist())  # fresh again
            for i in range(5):
                assert model.same_bits(np.concatenate(outs[i]), want[i]), (life, i)
    with pytest.raises(ValueError, match="closed"):
        rb.finalize([0])


def test_contract():
    import torch

    rs = Resample(3, 2)
    for bad in (Resample, "preemphasis", 16000, None):
        with pytest.raises(ValueError):
            ResampleBatch(bad, 4)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError):
            ResampleBatch(rs, bad)
    with pytest.raises(ValueError):
        ResampleBatch(rs, 4, dtype=np.int32)
    made = ResampleBatch({"name": "resample", "from_rate": 8000, "to_rate": 16000}, 4)
    assert type(made.resample) is Resample and made.resample.out_unit == 2
    made.close()
    with ResampleBatch(rs, 4) as rb:
        x = np.ones(30, np.float32)
        for bad in ([1, 1], [4], [-1]):
            with pytest.raises(ValueError):
                rb.resample_chunks(bad, [x] * len(bad))
            with pytest.raises(ValueError):
                rb.finalize(bad)
        with pytest.raises(ValueError):
            rb.resample_chunks([0, 1], [x])
        with pytest.raises(ValueError):
            rb.resample_chunks([0], [x.astype(np.float64)])
        with pytest.raises(ValueError):
            rb.resample_chunks_packed([0], torch.ones(30, dtype=torch.float64, device="cuda"), [30])
        with pytest.raises(ValueError):
            rb.resample_chunks_packed([0], torch.ones(30, device="cuda"), [31])
        assert rb.pending([0, 1, 2, 3])[0].tolist() == [0, 0, 0, 0]  # (nothing ran)
        assert rb.resample_chunks([], []) == []
    # equal rates: the chunks themselves, widened, and nothing held back
    with ResampleBatch(Resample(16000, 16000), 4, np.int16) as rb:
        a, b = np.arange(5, dtype=np.int16), np.arange(-3, 0, dtype=np.int16)
        got = rb.resample_chunks([2, 0], [a, b])
        assert model.same_bits(got[0], a.astype(np.float32)) and model.same_bits(got[1], b.astype(np.float32))
        assert [len(y) for y in rb.finalize([2, 0])] == [0, 0]


def test_in_front_of_a_stream_batch():
    """8 kHz chunks through ``ResampleBatch`` into ``StreamBatch.compute_chunks_packed``: every stream's rows over the
    ticks, the flush chunk and ``StreamBatch.finalize`` are ``compute_full(Resample.apply(signal))`` bit for bit.  (The
    computer's chunked and full paths frame the same samples for these signals: with 400-sample frames every 160, the
    last frame's right reflection -- at most 200 samples -- stays within the samples the stream still holds.)"""
    import torch

    comp = alias_factory_subclass_from_arg(FrameComputer, json.loads(json.dumps(FBANK)))
    rs = Resample(8000, 16000)
    rng = np.random.default_rng(21)
    sids = [3, 0, 5, 2]
    sigs = [signal(rng, n, np.float32) for n in (1500, 2111, 1800, 2600)]
    resampled = [rs.apply(x) for x in sigs]
    want = [comp.compute_full(y) for y in resampled]
    assert min(len(w) for w in want) > 15 and want[0].shape[1] == 40
    rb, sb = ResampleBatch(rs, 8), StreamBatch(comp, capacity=8)
    try:
        pos, rows, samples = [0] * 4, [[] for _ in sigs], [[] for _ in sigs]

        def through(part, d_out, out_lens):
            assert d_out.dtype == torch.float32
            feats, offs = sb.compute_chunks_packed([sids[i] for i in part], d_out, out_lens)
            feats, host, ends = feats.cpu().numpy(), d_out.cpu().numpy(), np.cumsum(out_lens)
            for j, i in enumerate(part):
                rows[i].append(feats[offs[j] : offs[j + 1]])
                samples[i].append(host[ends[j] - out_lens[j] : ends[j]])

        while any(pos[i] < len(sigs[i]) for i in range(4)):
            part = [i for i in range(4) if pos[i] < len(sigs[i]) and rng.random() < 0.8]
            if not part:
                continue
            lens = [min(int(rng.integers(0, 400)), len(sigs[i]) - pos[i]) for i in part]
            chunks = [sigs[i][pos[i] : pos[i] + c] for i, c in zip(part, lens)]
            for i, c in zip(part, lens):
                pos[i] += c
            d_samples = torch.from_numpy(np.concatenate(chunks) if chunks else np.zeros(0, np.float32)).cuda()
            through(part, *rb.resample_chunks_packed([sids[i] for i in part], d_samples, lens))
        through(list(range(4)), *rb.finalize_packed(sids))  # the flush chunk
        feats, offs = sb.finalize_packed(sids)
        feats = feats.cpu().numpy()
        for i in range(4):
            rows[i].append(feats[offs[i] : offs[i + 1]])
    finally:
        rb.close()
        sb.close()
    for i in range(4):
        assert model.same_bits(np.concatenate(samples[i]), resampled[i]), i  # (a mismatch below is then the framing's)
        got = np.concatenate(rows[i])
        assert got.dtype == want[i].dtype == np.float32 and got.shape == want[i].shape, (i, got.shape, want[i].shape)
        assert np.array_equal(got, want[i]), (i, float(np.abs(got.astype("f8") - want[i]).max()))
