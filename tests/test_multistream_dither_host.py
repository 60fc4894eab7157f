"""The host side of the dither of batched streaming (multistream.StreamBatch(dither=...)): what `dither` may be, the
per-stream bookkeeping of positions, seeds and keys, and the tick's upload layout.  No device."""
import numpy as np
import pytest

from pydrobert_speech_amd.multistream import (_DFIELDS, _CFIELDS, _FIELDS, _KFIELDS, DitherState, _place, _tick_layout,
                                              streaming_dither)
from pydrobert_speech_amd.pre import Dither, Preemphasize, dither_keys

A, C = 6364136223846793005, 1442695040888963407  # the step from a Dither's state to its next key


def test_dither_keeps_its_seed_and_keys_follow_one_rule():
    assert Dither(1.0, seed=5).seed == 5 and Dither(2.0).seed is None
    with pytest.raises(AttributeError):
        Dither(1.0, seed=5).seed = 6
    for seed in (0, 5, 2 ** 40 + 1):
        d = Dither(1.0, seed=seed)
        state = int(np.random.SeedSequence(seed).generate_state(1, np.uint64)[0])
        assert d._seed == state  # (what _launch steps before its first launch)
        assert int(dither_keys([seed])[0]) == (state * A + C) % (1 << 64)
    keys = dither_keys([3, 4, 3])
    assert keys.dtype == np.uint64 and keys[0] == keys[2] != keys[1]
    assert dither_keys([]).shape == (0,)


def test_streaming_dither_accepts_a_dither_an_alias_dict_or_an_alias_string():
    assert streaming_dither(Dither(1.5, seed=3)) == (1.5, 3)
    assert streaming_dither({"name": "dither", "coeff": 2, "seed": 9}) == (2.0, 9)
    assert streaming_dither({"alias": "dithering", "coeff": 0.5}) == (0.5, None)
    assert streaming_dither("dither") == (1.0, None)
    assert streaming_dither(Dither(np.float32(0.25), seed=np.int64(7))) == (0.25, 7)
    assert streaming_dither(None) is None
    assert streaming_dither(Dither(0.0, seed=3)) is None and streaming_dither({"name": "dither", "coeff": 0}) is None


@pytest.mark.parametrize("bad", [
    Preemphasize(0.97), "preemph", {"name": "preemphasize"}, 1.5, 0, True, np.float64(1.0),
    Dither(float("nan")), Dither(float("inf")), Dither(-float("inf")), Dither("1.0"), Dither(True),
    "nonesuch", {"name": "nonesuch"}, {"coeff": 1.0}, {"name": "dither", "sigma": 1.0}, [Dither(1.0)],
    Dither(1.0, seed=2 ** 63),
], ids=repr)
def test_streaming_dither_refuses(bad):
    with pytest.raises(ValueError, match="StreamBatch"):
        streaming_dither(bad)


def test_dither_state_positions_count_raw_samples():
    st = DitherState(8, base=100)
    ids = np.array([5, 2])
    step = st.step(ids, [160, 7])
    assert step["pos"].tolist() == [0, 0] and step["next_pos"].tolist() == [160, 7]
    # (step alone changes nothing)
    assert st.pos.tolist() == [0] * 8 and st.seed.tolist() == [-1] * 8 and st.count == 0
    st.commit(ids, step)
    assert st.pos[[5, 2]].tolist() == [160, 7]
    # raw chunk lengths: a chunk of which the computer drops samples (frame_shift > frame_length) advances by all of it,
    # an empty chunk by nothing
    step = st.step(np.array([2, 5, 0]), np.array([0, 1025, 3]))
    assert step["pos"].tolist() == [7, 160, 0]
    st.commit(np.array([2, 5, 0]), step)
    assert st.pos[[2, 5, 0]].tolist() == [7, 1185, 3]
    meta = np.zeros((2, 2), dtype=np.int64)
    step = st.step(np.array([0, 5]), [1, 1])
    st.fill_meta(meta, step)
    assert meta[:, 0].tolist() == [3, 1185] and meta[:, 1].tolist() == step["key"].tolist()


def test_dither_state_seeds_in_tick_order_and_ids_order():
    st = DitherState(8, base=100)
    ids = np.array([5, 2, 7])
    step = st.step(ids, [1, 0, 3])  # (an empty first chunk begins the utterance too)
    st.commit(ids, step)
    assert st.seed[ids].tolist() == [100, 101, 102] and st.count == 3
    assert st.key[ids].tolist() == dither_keys([100, 101, 102]).view(np.int64).tolist()
    ids = np.array([7, 0, 5, 1])  # 7 and 5 go on; 0 and 1 begin, in this order
    step = st.step(ids, [1, 1, 1, 1])
    assert step["seed"].tolist() == [102, 103, 100, 104]
    assert st.count == 3 and st.seed[[0, 1]].tolist() == [-1, -1]  # (not committed yet)
    st.commit(ids, step)
    assert st.count == 5 and st.seed.tolist() == [103, 104, 101, -1, -1, 100, -1, 102]
    assert st.key[0] == dither_keys([103]).view(np.int64)[0]


def test_dither_state_finalize_resets_and_the_next_chunk_begins_anew():
    st = DitherState(4, base=0)
    ids = np.array([0, 1, 2])
    st.commit(ids, st.step(ids, [10, 20, 30]))
    st.reset(np.array([1]))
    assert st.seed.tolist() == [0, -1, 2, -1] and st.pos.tolist() == [10, 0, 30, 0] and st.count == 3
    step = st.step(np.array([2, 1]), [5, 5])
    assert step["seed"].tolist() == [2, 3] and step["pos"].tolist() == [30, 0]
    st.commit(np.array([2, 1]), step)
    assert st.pos.tolist() == [10, 5, 35, 0] and st.count == 4


def test_dither_state_refuses_what_it_cannot_count():
    with pytest.raises(ValueError):
        DitherState(0, base=0)
    with pytest.raises(ValueError):
        DitherState(4, base=-1)
    with pytest.raises(ValueError):
        DitherState(4, base=2 ** 63)
    st = DitherState(4, base=2 ** 63 - 2)
    st.commit(np.array([0, 1]), st.step(np.array([0, 1]), [1, 1]))
    assert st.seed[[0, 1]].tolist() == [2 ** 63 - 2, 2 ** 63 - 1]
    with pytest.raises(OverflowError):
        st.step(np.array([2]), [1])


@pytest.mark.parametrize("chunks", [True, False])
@pytest.mark.parametrize("deltas,cmvn,stack", [(False, False, False), (True, True, False), (True, False, True)])
def test_tick_layout_without_dither_is_what_it_was(chunks, deltas, cmvn, stack):
    n, E, rows = 7, 4, 5
    sections = [("assemble", (n if chunks else 0, _FIELDS)), ("tiles", (n + 1 if chunks else 0,)),
                ("launch", (rows, E)), ("deltas", (n if deltas else 0, _DFIELDS)), ("elems", (n + 1 if deltas else 0,)),
                ("cmvn", (n if cmvn else 0, _CFIELDS))]
    if stack:
        sections += [("stack", (n, _KFIELDS)), ("stack_elems", (n + 1,))]
    was = _place(tuple(sections))
    assert _tick_layout(n, E, rows, chunks, deltas, cmvn, stack) == was
    assert _tick_layout(n, E, rows, chunks, deltas, cmvn, stack, False) == was
    at, words = _tick_layout(n, E, rows, chunks, deltas, cmvn, stack, True)
    # one section more, behind everything else: int64[n][2] in a compute_chunks tick, nothing in a finalize
    assert {k: v for k, v in at.items() if k != "dither"} == was[0]
    assert at["dither"] == (was[1], 2 * n if chunks else 0, (n if chunks else 0, 2), (2, 1))
    assert words == was[1] + (2 * n if chunks else 0)
