"""Bookkeeping of pre-emphasis and PCM chunks in batched streaming on the host, no device: StreamState.has_sample -- the
stream has been given a sample since its start or last reset, so a pre-emphasis has a previous sample -- over random
schedules, and how StreamBatch reads its `preemphasis` argument."""
import numpy as np
import pytest

from pydrobert_speech_amd import multistream
from pydrobert_speech_amd.multistream import StreamBatch, StreamState, streaming_preemphasis
from pydrobert_speech_amd.pre import Dither, Preemphasize
from tests.test_multistream_host import EXTRA, build, golden_configs, state_of

GEOMETRIES = ["shift_gt_length", "c1_kaldi_fbank"]


def computer(name):
    return build(EXTRA.get(name) or golden_configs()[name])


def replay_with_flags(state, pieces, rounds, rng):
    """tests/test_multistream_host.py::replay with a model of the flag beside it: all streams of `pieces` (one list of
    chunk lengths each) concurrently, a random subset per tick in random order, a stream whose chunks are done
    finalized in a later random tick -- and then started again, `rounds` times in all.  After every tick the state's
    flags must be the model's: a stream has a sample iff a chunk of positive length went to it since its last
    finalize.  Returns the number of (stream, tick) pairs in which a whole non-empty chunk was dropped."""
    B = len(pieces)
    nxt, left = [0] * B, [rounds] * B
    want = np.zeros(state.capacity, dtype=bool)
    whole_drops = 0
    while any(left):
        live = [i for i in range(B) if left[i]]
        tick = [i for i in live if rng.random() < 0.6] or live[:1]
        rng.shuffle(tick)
        feed = [i for i in tick if nxt[i] < len(pieces[i])]
        fin = [i for i in tick if nxt[i] >= len(pieces[i])]
        if feed:
            ids = np.asarray(feed)
            lens = np.asarray([pieces[i][nxt[i]] for i in feed])
            before = state.has_sample.copy()
            step = state.chunk_step(ids, lens)
            assert (state.has_sample == before).all()  # (chunk_step changes nothing)
            whole_drops += int(((step["drop"] == lens) & (lens > 0)).sum())
            state.commit_chunks(ids, step)
            want[ids] |= lens > 0
            for i in feed:
                nxt[i] += 1
        assert (state.has_sample == want).all()
        if fin:
            ids = np.asarray(fin)
            state.finalize_step(ids)
            assert (state.has_sample == want).all()  # (finalize_step changes nothing either)
            state.reset(ids)
            want[ids] = False
            for i in fin:
                nxt[i] = 0
                left[i] -= 1
        assert (state.has_sample == want).all()
    return whole_drops


@pytest.mark.parametrize("name", GEOMETRIES)
def test_flag_follows_the_samples_given(name):
    comp = computer(name)
    L, S = comp.frame_length, comp.frame_shift
    rng = np.random.default_rng(21)
    B = 24
    pieces = []
    for b in range(B):
        lens = rng.integers(0, 3 * L + 1, size=int(rng.integers(3, 12)))
        lens[rng.random(len(lens)) < 0.25] = 0
        lens[rng.random(len(lens)) < 0.25] = 1
        pieces.append(lens.tolist())
    pieces[0] = [0, 0, 5, 0, 7, 0]  # empty chunks before, between and after non-empty ones
    pieces[1] = [0, 0, 0]  # never a sample: finalized and reused without ever having one
    pieces[2] = [L, 1, 1, 0, 1, S]  # with frame_shift > frame_length: chunks of one sample swallowed by the skip
    state = state_of(comp, B + 3)
    whole_drops = replay_with_flags(state, pieces, 3, rng)
    assert not state.has_sample.any() and not state.started.any()  # (everyone was finalized)
    if name == "shift_gt_length":
        assert S > L and whole_drops > 0
    else:
        assert whole_drops == 0


def test_a_chunk_dropped_whole_still_counts():
    comp = computer("shift_gt_length")
    L, S = comp.frame_length, comp.frame_shift
    assert S > L + 2
    state = state_of(comp, 2)
    ids = np.asarray([1])
    # enough for the first frame: the samples up to the next frame's start are to be skipped
    step = state.chunk_step(ids, np.asarray([L]))
    state.commit_chunks(ids, step)
    assert step["k"][0] == 1 and state.skip[1] > 1 and state.has_sample.tolist() == [False, True]
    state.reset(ids)
    assert not state.has_sample.any() and state.skip[1] == 0
    # ... and the same for a stream whose only sample so far was dropped: stream 0 is fed an empty chunk (no sample),
    # then the first frame, then one sample that the skip swallows
    ids = np.asarray([0])
    for n, flag in ((0, False), (L, True)):
        state.commit_chunks(ids, state.chunk_step(ids, np.asarray([n])))
        assert bool(state.has_sample[0]) is flag
    step = state.chunk_step(ids, np.asarray([1]))
    assert step["drop"][0] == 1 and step["avail"][0] == 0  # no work span, hence no tile
    state.commit_chunks(ids, step)
    assert state.has_sample[0]
    # a fresh stream whose first chunk of samples is a later one: empty chunks do not set the flag
    state.reset(ids)
    for n, flag in ((0, False), (0, False), (1, True), (0, True)):
        state.commit_chunks(ids, state.chunk_step(ids, np.asarray([n])))
        assert bool(state.has_sample[0]) is flag


def test_half_flips_with_every_tick_that_names_a_stream():
    # the previous samples live in the half the carries do: a tick writes the other half for every stream it names,
    # with or without a work span, so the half must flip for all of them
    state = StreamState(4, 400, 160, 0)
    ids = np.asarray([2, 0])
    for n in (0, 1, 0, 1000, 0):
        before = state.half.copy()
        state.commit_chunks(ids, state.chunk_step(ids, np.asarray([n, 0])))
        assert (state.half[ids] == before[ids] ^ 1).all() and (state.half[[1, 3]] == before[[1, 3]]).all()


def test_preemphasis_argument():
    assert streaming_preemphasis(None) == 0.0
    assert streaming_preemphasis(0) == 0.0 and streaming_preemphasis(0.0) == 0.0
    assert streaming_preemphasis(0.97) == 0.97 and streaming_preemphasis(np.float32(0.5)) == 0.5
    assert streaming_preemphasis(1) == 1.0
    assert streaming_preemphasis(Preemphasize(0.9)) == 0.9
    assert streaming_preemphasis(Preemphasize(0)) == 0.0
    assert streaming_preemphasis("preemph") == Preemphasize().coeff == 0.97
    assert streaming_preemphasis({"name": "preemphasize", "coeff": 0.95}) == 0.95
    for bad in ("dither", Dither(), {"name": "dither"}, "no_such_alias", {"coeff": 0.97}, {"name": "preemph", "c": 1},
                [0.97], float("nan"), float("inf"), True, Preemphasize("0.97"), object()):
        with pytest.raises(ValueError):
            streaming_preemphasis(bad)


class _NoDevice:
    """stands in for torch and the library where StreamBatch's constructor wants them: the argument checks and the
    pools it allocates are host logic"""

    float32, float64, int64 = "float32", "float64", "int64"

    class cuda:
        @staticmethod
        def current_device():
            return 0

    @staticmethod
    def device(*args):
        return args

    def __init__(self):
        self.allocated = []

    def zeros(self, shape, dtype=None, device=None):
        self.allocated.append((tuple(shape), dtype))
        return ("zeros", tuple(shape), dtype)

    def pds_multistream_tile(self):
        return 1024

    pds_multistream_assemble_f32 = pds_multistream_assemble_f64 = None


@pytest.fixture
def no_device(monkeypatch):
    fake = _NoDevice()
    monkeypatch.setattr(multistream._native, "require_device", lambda: fake)
    monkeypatch.setattr(multistream._native, "lib", lambda: fake)
    comp = computer("c1_kaldi_fbank")
    monkeypatch.setattr(type(comp), "_native_plan", lambda self, device: None)
    return fake, comp


def test_constructor_reads_preemphasis_before_it_touches_a_device(monkeypatch):
    comp = computer("c1_kaldi_fbank")

    def no_device():
        raise AssertionError("the argument is checked first")

    monkeypatch.setattr(multistream._native, "require_device", no_device)
    for bad in ("dither", float("nan"), [0.97], True):
        with pytest.raises(ValueError):
            StreamBatch(comp, capacity=4, preemphasis=bad)
    with pytest.raises(TypeError):
        StreamBatch(comp, capacity=4, dtype=np.int16, preemphasis=0.97)


def test_no_previous_sample_pool_without_preemphasis(no_device):
    fake, comp = no_device
    L = comp.frame_length
    for none in (None, 0, 0.0, Preemphasize(0)):
        fake.allocated.clear()
        sb = StreamBatch(comp, capacity=6, preemphasis=none)
        assert sb.preemphasis == 0.0 and sb._prev is None
        assert fake.allocated == [((2, 6, L), "float32")]  # the carry pool and nothing else
    assert StreamBatch(comp, capacity=6)._prev is None
    for dtype in (np.float32, np.float64):
        fake.allocated.clear()
        sb = StreamBatch(comp, capacity=6, dtype=dtype, preemphasis=Preemphasize(0.97))
        assert sb.preemphasis == 0.97
        name = np.dtype(dtype).name
        assert fake.allocated == [((2, 6, L), name), ((2, 6), name)]  # + 2 * capacity elements
        assert sb._prev == ("zeros", (2, 6), name)
        sb.close()
        assert sb._prev is None and sb._pool is None
