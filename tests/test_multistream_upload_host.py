"""The layout of a tick's one upload in batched streaming (multistream._Upload over multistream._tick_layout), on the
host, without a device: the sections lie back to back in the documented order -- samples, assemble metadata ``n x 8``,
tile prefix ``n + 1``, launch metadata ``rows x E``, deltas metadata ``n x 8``, element prefix ``n + 1``, cmvn metadata
``n x 8`` --, their sum is what the tick asks of the staging, every view has its section's shape, and no two views share
a word.  The expected offsets are written out here by hand, as the ticks computed them before there was a helper."""
import numpy as np
import pytest

from pydrobert_speech_amd.multistream import _tick_layout, _Upload

ORDER = ["samples", "assemble", "tiles", "launch", "deltas", "elems", "cmvn"]
# n, E, sample words, deltas, cmvn, launch rows; a finalize tick has no samples, assemble metadata or tile prefix
CASES = [
    (5, 3, 100, False, False, 4),
    (5, 3, 100, True, True, 5),
    (5, 5, 7, True, False, 4),
    (1, 1, 1, False, True, 5),
    (0, 0, 0, True, True, 4),  # an empty tick
    (4, 0, 9, True, True, 5),  # no stream emits
    (4, 2, 0, True, True, 4),  # empty chunks, or samples already on the device
    (3, 0, 0, False, False, 4),
]


def expected(n, E, ns, deltas, cmvn, launch_rows, chunks):
    """name -> (first word, shape), and the total"""
    rest = 8 * n + (n + 1) if chunks else 0
    at = ns + 8 * n if chunks else ns
    words = ns + rest + launch_rows * E
    dwords = 8 * n + (n + 1) if deltas else 0
    want = {
        "samples": (0, (ns,)),
        "assemble": (ns, (n if chunks else 0, 8)),
        "tiles": (at, (n + 1 if chunks else 0,)),
        "launch": (ns + rest, (launch_rows, E)),
        "deltas": (words, (n if deltas else 0, 8)),
        "elems": (words + (8 * n if deltas else 0), (n + 1 if deltas else 0,)),
        "cmvn": (words + dwords, (n if cmvn else 0, 8)),
    }
    return want, words + dwords + (8 * n if cmvn else 0)


def check(up, want, total):
    assert ["samples"] + list(up.at) == ORDER
    assert up.words == total
    up.pinned = np.full(total + 3, -1, dtype=np.int64)  # (a staging buffer is larger than what is asked of it)
    end = 0
    for tag, name in enumerate(ORDER, 1):
        first, shape = want[name]
        view = up.host(name)
        assert view.shape == shape and view.dtype == np.int64 and view.base is not None
        assert first == end  # contiguous, in order
        view[...] = tag
        end = first + view.size
    assert end == total
    # every word of the upload was written through exactly one view, and none outside it
    flat = np.concatenate([np.full(int(np.prod(want[name][1])), tag) for tag, name in enumerate(ORDER, 1)] + [[-1] * 3])
    assert np.array_equal(up.pinned, flat)


@pytest.mark.parametrize("chunks", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_sections_lie_back_to_back_in_their_shapes(case, chunks):
    n, E, ns, deltas, cmvn, launch_rows = case
    if not chunks:
        ns = 0
    up = _Upload(ns, _tick_layout(n, E, launch_rows, chunks, deltas, cmvn))
    check(up, *expected(n, E, ns, deltas, cmvn, launch_rows, chunks))


@pytest.mark.parametrize("case", CASES)
def test_sections_follow_the_samples_when_they_shrink(case):
    # a tick asks the staging for its samples as float words; when they travel as int16 they take fewer, and the
    # sections behind them are placed after that
    n, E, ns, deltas, cmvn, launch_rows = case
    up = _Upload(ns, _tick_layout(n, E, launch_rows, True, deltas, cmvn))
    asked = up.words
    assert asked == expected(n, E, ns, deltas, cmvn, launch_rows, True)[1]
    fewer = (ns + 1) // 2
    up.sample_words = fewer
    assert up.words == asked - (ns - fewer)
    check(up, *expected(n, E, fewer, deltas, cmvn, launch_rows, True))


def test_device_views_are_the_host_views_of_the_copy():
    import torch

    for n, E, ns, deltas, cmvn, launch_rows in CASES:
        up = _Upload(ns, _tick_layout(n, E, launch_rows, True, deltas, cmvn))
        up.pinned = np.arange(up.words, dtype=np.int64)
        up.device = torch.from_numpy(np.append(up.pinned, 0))  # (as _send: at least one word)
        for name in ORDER:
            assert np.array_equal(up.dev(name).numpy(), up.host(name)) and tuple(up.dev(name).shape) == up.host(name).shape
