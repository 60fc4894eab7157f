"""The post stages of batched streaming as the constructor lists them, no device (multistream._Stage and its
subclasses): for every subset of the stages the order of the list, the widths folded through it, every stage's pools
and the host states the batch shows; that ``close`` leaves no stage a pool; and the flags a tick passes to
``_tick_layout``."""
import inspect
import itertools

import numpy as np
import pytest

from pydrobert_speech_amd.multistream import CmvnState, DeltaState, SlidingState, StackState, _TickBatch
from pydrobert_speech_amd.post import Cepstra, Deltas, SlidingCMVN, Stack, Standardize
from pydrobert_speech_amd.pre import Dither
from tests.test_multistream_stack_host import _FakeLibWithStack, _FakeTorch, fake_batch

CAP = 4  # (fake_batch's capacity)
NORMS = (None, "cmvn", "cmvn_fixed", "sliding")  # nothing, running cmvn, cmvn_running=False, sliding_cmvn
# (cepstra, deltas, stack) -> _F, _C, num_coeffs on a 40-coefficient computer with Cepstra(13), Deltas(2), Stack(3)
WIDTHS = {
    (False, False, False): (40, 40, 40),
    (False, False, True): (40, 40, 120),
    (False, True, False): (40, 120, 120),
    (False, True, True): (40, 120, 360),
    (True, False, False): (13, 13, 13),
    (True, False, True): (13, 13, 39),
    (True, True, False): (13, 39, 39),
    (True, True, True): (13, 39, 117),
}
SUBSETS = list(itertools.product((False, True), NORMS, (False, True), (False, True)))


class _TypedTorch(_FakeTorch):
    """an allocation also says its dtype, and ``from_numpy(a).to(device)`` is a copy of `a`'s shape and dtype"""

    @staticmethod
    def zeros(shape, dtype=None, device=None):
        return ("zeros", tuple(shape), dtype)

    @staticmethod
    def empty(shape, dtype=None, device=None):
        return ("empty", tuple(shape), dtype)

    @staticmethod
    def from_numpy(a):
        class Host:
            to = staticmethod(lambda device: ("copy", a.shape, a.dtype.name))

        return Host


def batch(monkeypatch, dtype, cepstra, norm, deltas, stack, dither=False):
    kwargs = {}
    if cepstra:
        kwargs["cepstra"] = Cepstra(13)
    if norm == "cmvn":
        kwargs["cmvn"] = Standardize()
    elif norm == "cmvn_fixed":
        fixed = Standardize()  # with the statistics of three frames (sums | count, sums of squares | unused)
        fixed._stats = np.ones((2, WIDTHS[cepstra, False, False][0] + 1))
        fixed._stats[:, -1] = 3, 0
        kwargs.update(cmvn=fixed, cmvn_running=False)
    elif norm == "sliding":
        kwargs["sliding_cmvn"] = SlidingCMVN(4, 1)
    if deltas:
        kwargs["deltas"] = Deltas(2)
    if stack:
        kwargs["stack"] = Stack(3)
    if dither:
        kwargs["dither"] = Dither(1.0, seed=3)
    comp, sb = fake_batch(monkeypatch, _FakeLibWithStack, torch=_TypedTorch, dtype=dtype, **kwargs)
    assert comp.num_coeffs == 40
    return sb


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_order_widths_pools_and_states_of_every_subset(monkeypatch, dtype):
    T = "f4" if dtype == np.float32 else "f8"  # (_FakeTorch's names of the dtypes)
    for cepstra, norm, deltas, stack in SUBSETS:
        sb = batch(monkeypatch, dtype, cepstra, norm, deltas, stack)
        F, C, width = WIDTHS[cepstra, deltas, stack]
        present = (("cepstra", cepstra), ("cmvn", norm in ("cmvn", "cmvn_fixed")), ("sliding", norm == "sliding"),
                   ("deltas", deltas), ("stack", stack))
        assert list(sb._stages) == [name for name, on in present if on]  # pipeline order
        assert (sb._F0, sb._F, sb._C, sb.num_coeffs) == (40, F, C, width)
        assert sb.lookahead == (4 if deltas else 0) and sb.num_vectors == (3 if stack else 1)
        # the pools, and the entry point of the batch's dtype
        bits = "f32" if dtype == np.float32 else "f64"
        pools = {name: stage.pools for name, stage in sb._stages.items()}
        if cepstra:
            assert pools["cepstra"] == {} and sb._stages["cepstra"].state is None
        if norm == "cmvn":
            assert pools["cmvn"] == {"sums": ("empty", (CAP, 2, F), "f8")}
        if norm == "cmvn_fixed":  # (no running sums; the prior without its count)
            assert pools["cmvn"] == {"prior": ("copy", (2, F), "float64")}
        if norm in ("cmvn", "cmvn_fixed"):
            assert sb._stages["cmvn"]._fn == "cmvn_" + bits
        if norm == "sliding":
            assert pools["sliding"] == {"ring": ("empty", (CAP, 4 + 1, F), T), "sums": ("empty", (CAP, 2, F), "f8")}
            assert sb._stages["sliding"]._fn == "sliding_" + bits
        if deltas:
            assert pools["deltas"] == {"hist": ("zeros", (2, CAP, 2 * 4, F), T)}
        if stack:
            assert pools["stack"] == {"pending": ("empty", (2, CAP, 3 - 1, C), T)}
            assert sb._stages["stack"]._fn == "stack_" + bits
        # the states the batch shows are those of the stages present, and None otherwise
        for attr, name, kind in (("cstate", "cmvn", CmvnState), ("wstate", "sliding", SlidingState),
                                 ("dstate", "deltas", DeltaState), ("kstate", "stack", StackState)):
            if dict(present)[name]:
                assert isinstance(getattr(sb, attr), kind) and getattr(sb, attr) is sb._stages[name].state
            else:
                assert getattr(sb, attr) is None and name not in sb._stages
        if sb.cstate is not None:
            assert sb.cstate.running == (norm == "cmvn") and sb.cstate.prior_count == (0 if norm == "cmvn" else 3)
        assert sb.nstate is None


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_close_leaves_no_stage_a_pool(monkeypatch, dtype):
    for norm in ("cmvn", "cmvn_fixed", "sliding"):
        sb = batch(monkeypatch, dtype, True, norm, True, True)
        stages = list(sb._stages.values())
        assert len(stages) == 4 and all(stage.pools for stage in stages[1:])
        sb._check_open()
        sb.close()
        assert all(stage.pools == {} for stage in stages)
        with pytest.raises(ValueError, match="closed"):
            sb._check_open()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_layout_flags_are_the_stages_asked_for(monkeypatch, dtype):
    # (the one call of _tick_layout passes them as they are; the spy of test_gpu_multistream_cepstra.py sees the call)
    assert "not final, *self._layout_flags))" in inspect.getsource(_TickBatch._tick)
    for (cepstra, norm, deltas, stack), dither in itertools.product(SUBSETS, (False, True)):
        sb = batch(monkeypatch, dtype, cepstra, norm, deltas, stack, dither)
        # _tick_layout(n, E, launch_rows, chunks, deltas, cmvn, stack, dither, sliding)
        assert sb._layout_flags == (deltas, norm in ("cmvn", "cmvn_fixed"), stack, dither, norm == "sliding")
