"""The short-integration kernels at every launch shape they take, against the pinned oracle.

csrc/si_fft.hip sizes its grid by the batch (csrc/si_shape.h): with few workgroups the filters of a stretch are dealt
to up to eight workgroups (grid.z), with many one workgroup walks all of them.  A batch of one to eight utterances --
all the other SI tests feed -- only ever takes the finest split, so these tests ask pds_si_launch_shape (host
arithmetic, nothing hard-coded to a CU count) for batch sizes that give one group, one group over several workgroups per
utterance, an intermediate split with a short last group and a split into single filters, run them, and assert that the
launch made had that shape.  The direct form (csrc/si.hip, the only float64 path) is run at frame counts around its
tile edges, at the clamp of its tile to short batches and with utterances that end before the batch's last tile.

Inputs are Gaussian noise; tolerances are those of tests/test_gpu_si.py.  Bit-for-bit claims: a copy of a signal gives
the same rows wherever it stands in a batch, and a signal's rows do not depend on the launch shape (a (utterance,
transform, filter) sum is formed by the same instructions whichever workgroup walks the filter).

Noise is the most forgiving input a filter bank can get, and close() forgives everything below 1e-3 max|want|: what the
kernels compute on tones, DC, Nyquist, impulses, chirps, steps, levels from 1e-3 to 1e7 and non-finite samples is
tests/test_gpu_si_structured.py, under the float32 error model of tests/si_structured.py (calibrated on the CPU by
tests/test_si_structured_model.py, never from a kernel's output).  There the FFT form needed at most 11 % of its
allowance MARGIN x KAPPA_REF_FFT (0.105 of 0.96), the direct form 20 % of MARGIN x KAPPA_REF_DIRECT (0.034 of 0.168),
and the float64 direct kernel passed the strict rule alone (profiles/r15a_si_structured_parity.txt)."""
import ctypes

import numpy as np
import pytest

from oracle import si_oracle as so
from pydrobert_speech_amd import _native
from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg
from pydrobert_speech_amd.compute import FrameComputer
from pydrobert_speech_amd.multistream_si import SiStreamBatch
from tests.test_gpu_si import F32, close

pytestmark = pytest.mark.gpu

F64 = dict(rtol=1e-9, atol=1e-9)
SHAPE_FIELDS = ("form", "grid_x", "groups", "c_per_group", "blocks", "nw", "per_wg", "cus")


def launch_shape(comp, B, max_frames, direct=False):
    """pds_si_launch_shape as a dict (direct form: `blocks` is JB, `nw` the passes of the thread block)"""
    out = (ctypes.c_int32 * 8)()
    rc = _native.lib().pds_si_launch_shape(comp._native_plan().handle, int(B), int(max_frames), int(direct), out)
    _native.check(rc, "pds_si_launch_shape")
    return dict(zip(SHAPE_FIELDS, out))


def si_computer(bank, num_filts, rate, shift_ms, use_power=True, use_log=True, include_energy=False):
    return alias_factory_subclass_from_arg(
        FrameComputer, {"name": "si", "bank": {"name": bank, "scaling_function": "mel", "num_filts": num_filts,
                                               "sampling_rate": rate},
                        "frame_shift_ms": shift_ms, "use_power": use_power, "use_log": use_log,
                        "include_energy": include_energy})


def oracle_params(comp):
    return so.SiParams(comp.frame_shift, comp._max_support, comp._translation, comp.dft_size, comp.taps,
                       comp._window.reshape(-1), comp.frame_style == "centered", comp._power, comp._log)


def length_with_frames(comp, frames):
    """the shortest signal that yields `frames` frames"""
    n = max(0, frames - 3) * comp.frame_shift
    while comp.num_frames(n) < frames:
        n += 1
    assert comp.num_frames(n) == frames
    return n


def noise(rng, n):
    return (1000 * rng.standard_normal(n)).astype("f4")


def run_packed(comp, signals, idx, dtype="f4", direct=False, out=None):
    """the utterances ``signals[i] for i in idx`` packed back to back (no gaps: a read past an utterance's end lands in
    its neighbour) through compute_packed; returns (rows as a host array, row offsets, max frames)"""
    import torch

    lens = np.array([len(signals[i]) for i in idx], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    flat = np.concatenate([signals[i] for i in idx]).astype(dtype)
    x = torch.from_numpy(flat if len(flat) else np.zeros(1, dtype)).cuda()
    nframes = np.array([comp.num_frames(int(n)) for n in lens], dtype=np.int64)
    feats, rows = comp.compute_packed(x, offs, lens, nframes, direct=direct, out=out)
    return feats.cpu().numpy(), rows, int(nframes.max())


def assert_copies(got, rows, idx):
    """every copy of a signal has the bits of its first copy in the batch; returns {signal: rows of the first copy}"""
    first = {}
    for b, i in enumerate(idx):
        mine = got[rows[b] : rows[b + 1]]
        if i not in first:
            first[i] = mine
        else:
            assert np.array_equal(mine, first[i]), (b, i)
    return first


# ---- the FFT form ---------------------------------------------------------------------------------------------------

FFT_BANKS = {
    # name: (constructor arguments, transform size, C)
    "gabor41_1024": (dict(bank="gabor", num_filts=40, rate=16000, shift_ms=10, include_energy=True), 1024, 41),
    "gammatone40_2048": (dict(bank="gammatone", num_filts=40, rate=48000, shift_ms=2.5), 2048, 40),
    "gabor5_1024": (dict(bank="gabor", num_filts=5, rate=16000, shift_ms=10, use_power=False), 1024, 5),  # magnitudes
    "gammatone5_2048": (dict(bank="gammatone", num_filts=5, rate=48000, shift_ms=5), 2048, 5),
}
_FFT = {}


class FftBank:
    """a computer, its distinct noise signals (the longest first, so that every batch has the same longest utterance),
    one long one for launches with several workgroups per utterance, the oracle's features of each (computed once)
    and each one's rows from a launch of its own (B = 1, the shape every other SI test runs)"""

    def __init__(self, name):
        kwargs, size, C = FFT_BANKS[name]
        self.comp = comp = si_computer(**kwargs)
        assert comp.fft_size == size and comp.num_coeffs == C
        S = comp.frame_shift
        one = launch_shape(comp, 1, 1)
        self.blocks, self.per_wg, self.cus = one["blocks"], one["per_wg"], one["cus"]
        assert one["form"] == size and self.blocks * S <= size - (comp._max_support - 1)
        # block count Tb + 1 an exact multiple of the transform's blocks (its last transform is full), and one frame more
        full = length_with_frames(comp, 2 * self.blocks - 1)
        lens = [41 * S + S // 2, length_with_frames(comp, 2 * self.blocks), full, 3 * S + 7, S - 1, 1, 0]
        rng = np.random.default_rng(size + C)
        self.signals = [noise(rng, n) for n in lens]
        assert (comp.num_frames(full) + 1) % self.blocks == 0 and comp.num_frames(lens[0]) <= 45
        # more frames than one workgroup's transforms yield: grid.x >= 2
        self.signals.append(noise(rng, length_with_frames(comp, self.per_wg * self.blocks + 3)))
        self.long = len(self.signals) - 1
        p = oracle_params(comp)
        self.want = [so.compute_full(x.astype("f8"), p) for x in self.signals]  # (float64: the oracle rounds to its input's type)
        self.anchor = []
        for i, x in enumerate(self.signals):
            got, rows, most = run_packed(comp, self.signals, [i])
            self.anchor.append(got)
            assert got.shape == self.want[i].shape
        for a in self.anchor + self.want:
            a.flags.writeable = False

    def frames(self, i):
        return self.want[i].shape[0]


def fft_bank(name):
    if name not in _FFT:
        _FFT[name] = FftBank(name)
    return _FFT[name]


def find_batch(comp, max_frames, wanted, lo, hi=65535, last=False):
    """the smallest (`last`: the largest) batch size in lo .. hi whose launch shape satisfies `wanted`, or None"""
    found = None
    for B in range(lo, hi + 1):
        if wanted(launch_shape(comp, B, max_frames)):
            found = B
            if not last:
                break
    return found


def skip_or_fail_unreachable(what):
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus != 256, f"{what} must be reachable on an MI355X"
    pytest.skip(f"no batch of up to 65535 utterances gives {what} on a device of {cus} CUs")


FFT_CASES = [(name, shape) for name in ("gabor41_1024", "gammatone40_2048")
             for shape in ("anchor", "one_group", "one_group_two_x", "ragged_split", "ragged_split_coarse")]
FFT_CASES += [(name, shape) for name in ("gabor5_1024", "gammatone5_2048") for shape in ("anchor", "unit_groups", "one_group")]


@pytest.mark.parametrize("name,shape", FFT_CASES)
def test_fft_form_at_every_launch_shape(name, shape):
    """anchor: each signal alone (B = 1: the filters split eight ways, as in every other SI test) against the oracle.
    one_group: grid.z == 1, one workgroup walks all C filters (what bench.py measures and a tick of many streams takes).
    one_group_two_x: the same with one long utterance, so that grid.x >= 2.  ragged_split: fewer groups than the finest
    split has, the last one short (C % c_per_group != 0), at the smallest batch that gives one; ragged_split_coarse: at
    the largest (the fewest, longest groups).  unit_groups: c_per_group == 1, at the largest batch that still splits
    that far.  In every batch each distinct signal is within F32 of the oracle, every copy has the first copy's bits, and
    those are the bits of the signal's own B = 1 launch."""
    bk = fft_bank(name)
    comp, C = bk.comp, bk.comp.num_coeffs
    cycle = list(range(bk.long))  # the distinct signals without the long one
    if shape == "anchor":
        for i in range(len(bk.signals)):
            one = launch_shape(comp, 1, max(1, bk.frames(i)))
            # 2 * CUs / workgroups >= 8 on any device this runs on: the finest split
            assert one["c_per_group"] == -(-C // min(8, max(1, 2 * bk.cus // one["grid_x"])))
            assert one["groups"] == -(-C // one["c_per_group"]) and one["groups"] > 1
            close(bk.anchor[i], bk.want[i], **F32)
        assert launch_shape(comp, 1, bk.frames(bk.long))["grid_x"] == 2
        return
    most = bk.frames(bk.long) if shape == "one_group_two_x" else bk.frames(0)
    wanted = {
        "one_group": lambda s: s["groups"] == 1 and s["c_per_group"] == C and s["grid_x"] == 1,
        "one_group_two_x": lambda s: s["groups"] == 1 and s["c_per_group"] == C and s["grid_x"] >= 2,
        # (an intermediate split: fewer groups than the finest one)
        "ragged_split": lambda s: 1 < s["groups"] < -(-C // -(-C // 8)) and C % s["c_per_group"] != 0,
        "ragged_split_coarse": lambda s: 1 < s["groups"] < -(-C // -(-C // 8)) and C % s["c_per_group"] != 0,
        "unit_groups": lambda s: s["c_per_group"] == 1 and s["groups"] == C,
    }[shape]
    last = shape in ("unit_groups", "ragged_split_coarse")  # (a split needs 2 * CUs >= 2 * B: the search can stop early)
    B = find_batch(comp, most, wanted, lo=len(cycle) + 1, hi=4096 if last else 65535, last=last)
    if B is None:
        skip_or_fail_unreachable(shape)
    head = [bk.long] if shape == "one_group_two_x" else []
    idx = head + [cycle[b % len(cycle)] for b in range(B - len(head))]
    got, rows, max_frames = run_packed(comp, bk.signals, idx)
    made = launch_shape(comp, len(idx), max_frames)  # (compute_packed makes one call: B <= 65535)
    assert max_frames == most and wanted(made), made
    assert not np.isnan(got).any()
    first = assert_copies(got, rows, idx)
    assert sorted(first) == sorted(set(cycle) | set(head))
    for i, mine in first.items():
        close(mine, bk.want[i], **F32)
        assert np.array_equal(mine, bk.anchor[i]), (shape, i, made)


@pytest.mark.parametrize("name", list(FFT_BANKS))
def test_fft_form_writes_only_its_own_rows_and_columns(name):
    """an `out` wider than C and with spare rows, filled with NaN, at the one-group shape: the spare columns and rows
    keep their NaN, everything else is written (and finite)"""
    import torch

    bk = fft_bank(name)
    comp, C = bk.comp, bk.comp.num_coeffs
    cycle = list(range(bk.long))
    B = find_batch(comp, bk.frames(0), lambda s: s["groups"] == 1, lo=len(cycle) + 1)
    if B is None:
        skip_or_fail_unreachable("one group")
    idx = [cycle[b % len(cycle)] for b in range(B)]
    total = sum(bk.frames(i) for i in idx)
    out = torch.full((total + 3, C + 3), float("nan"), dtype=torch.float32, device="cuda")
    got, rows, max_frames = run_packed(comp, bk.signals, idx, out=out)
    assert launch_shape(comp, B, max_frames)["groups"] == 1 and rows[-1] == total
    assert got.shape == (total + 3, C + 3)
    assert np.isnan(got[:, C:]).all() and np.isnan(got[total:]).all()
    assert np.isfinite(got[:total, :C]).all()
    first = assert_copies(got[:, :C], rows, idx)
    for i, mine in first.items():
        assert np.array_equal(mine, bk.anchor[i]), i


# ---- the direct form ------------------------------------------------------------------------------------------------

# (rate, shift_ms, S, JB of a batch long enough not to clamp it, bank, num_filts); JB = max(2, 2304 / S)
DIRECT = [
    (8000, 5, 40, 57, "gabor", 3), (8000, 5, 40, 57, "tri", 4),
    (16000, 10, 160, 14, "gabor", 8), (16000, 10, 160, 14, "tri", 3),
    (16000, 25, 400, 5, "gabor", 4), (16000, 25, 400, 5, "tri", 10),
    (48000, 25, 1200, 2, "gabor", 7), (48000, 25, 1200, 2, "tri", 3),      # the floor of JB; two passes of the thread block
    (48000, 50, 2400, 2, "gabor", 12), (48000, 50, 2400, 2, "tri", 3),    # a tile of 4800 samples: three passes
]
_DIRECT = {}


def direct_computer(rate, shift_ms, bank, num_filts):
    # complex taps with powers and logs, real taps with magnitudes and raw sums
    return si_computer(bank, num_filts, rate, shift_ms, use_power=bank != "tri", use_log=bank != "tri")


def test_direct_banks_cover_the_tap_padding():
    """taps are padded to a multiple of 9: supports with M % 9 == 0 (no padding), 1 (eight zero taps) and 8 (one), for
    complex and for real taps"""
    rest = {"gabor": set(), "tri": set()}
    for rate, shift_ms, S, _, bank, num_filts in DIRECT:
        comp = direct_computer(rate, shift_ms, bank, num_filts)
        assert comp.frame_shift == S and comp._real == (bank == "tri")
        rest[bank].add(comp._max_support % 9)
    assert {0, 1, 8} <= rest["gabor"] | rest["tri"], rest
    assert {0, 8} <= rest["gabor"] and {0, 1, 8} <= rest["tri"], rest


class DirectBank:
    def __init__(self, rate, shift_ms, S, JB, bank, num_filts):
        self.comp = comp = direct_computer(rate, shift_ms, bank, num_filts)
        # frame counts around one and two tiles' worth of frames, those that clamp the tile, and no frame at all
        counts = {k * (JB - 1) + e for k in (1, 2) for e in (-1, 0, 1)} | {1, 2, 3}
        self.counts = sorted(c for c in counts if c > 0)
        rng = np.random.default_rng(rate + S + num_filts)
        self.signals = [noise(rng, length_with_frames(comp, c)) for c in self.counts] + [noise(rng, 1), noise(rng, 0)]
        p = oracle_params(comp)
        self.want = [so.compute_full(x.astype("f8"), p) for x in self.signals]  # (float64: the oracle rounds to its input's type)
        assert [w.shape[0] for w in self.want] == self.counts + [0, 0]


@pytest.mark.parametrize("dtype", ["f4", "f8"])
@pytest.mark.parametrize("rate,shift_ms,S,JB,bank,num_filts", DIRECT)
def test_direct_form_at_its_tile_edges(rate, shift_ms, S, JB, bank, num_filts, dtype):
    """si_conv_kernel with k (JB - 1) + {-1, 0, 1} frames per utterance (k = 1, 2), 300 or more utterances in one ragged
    launch (the short ones' later workgroups leave at once: j0 >= Tb) and batches of at most 1, 2 and 3 frames, which
    clamp JB to 2, 3 and 4: float32 against the oracle and (shifts of up to 1024 samples, which have one) the FFT form,
    float64 against the oracle to 1e-9, every copy of a signal bit-identical to the first.  (S = 2400: a tile of 4800
    samples is three passes of 2304, not two.)"""
    key = (rate, shift_ms, bank)
    if key not in _DIRECT:
        _DIRECT[key] = DirectBank(rate, shift_ms, S, JB, bank, num_filts)
    bk = _DIRECT[key]
    comp, tol = bk.comp, F32 if dtype == "f4" else F64
    nd = len(bk.signals)
    idx = [b % nd for b in range(nd * -(-300 // nd))]
    got, rows, most = run_packed(comp, bk.signals, idx, dtype=dtype, direct=True)
    made = launch_shape(comp, len(idx), most, direct=True)
    assert made["form"] == 0 and made["blocks"] == JB and most == bk.counts[-1], made
    assert made["nw"] == -(-JB * S // 2304) and (S < 2400 or made["nw"] >= 2)  # passes of the thread block
    # utterances that end before the launch's last tile starts
    assert made["grid_x"] >= 2 and bk.counts[0] <= (made["grid_x"] - 1) * (JB - 1)
    assert got.dtype == np.dtype(dtype) and not np.isnan(got).any()
    first = assert_copies(got, rows, idx)
    for i, mine in first.items():
        close(mine, bk.want[i], **tol)
    if dtype == "f4" and comp.fft_size:
        fft, fft_rows, _ = run_packed(comp, bk.signals, idx[:nd])
        assert launch_shape(comp, nd, most)["form"] == comp.fft_size
        for i in range(nd):
            close(first[i], fft[fft_rows[i] : fft_rows[i + 1]], **F32)
    for limit in (1, 2, 3):  # the clamp of JB to the batch's longest utterance
        few = [i for i in range(nd) if bk.want[i].shape[0] <= limit]
        got, rows, most = run_packed(comp, bk.signals, few, dtype=dtype, direct=True)
        assert most == limit and launch_shape(comp, len(few), most, direct=True)["blocks"] == min(JB, limit + 1)
        for b, i in enumerate(few):
            close(got[rows[b] : rows[b + 1]], bk.want[i], **tol)


# ---- streaming ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["gabor41_1024", "gammatone40_2048"])
def test_a_tick_of_many_streams_takes_the_one_group_shape(name):
    """SiStreamBatch with more active streams than twice the CUs: every tick that has frames, and the finalize, is one
    launch with grid.z == 1.  Three ticks of 10 ms chunks, the streams cycling through four signals: the first, the last
    and two middle streams of each signal give their private computer's compute_chunk / finalize rows bit for bit"""
    kwargs, _, C = FFT_BANKS[name]
    comp = si_computer(**kwargs)
    chunk = int(0.01 * comp.sampling_rate)
    cus = launch_shape(comp, 1, 1)["cus"]
    N = find_batch(comp, 1, lambda s: s["groups"] == 1, lo=8)
    assert N is not None, f"no one-group launch on a device of {cus} CUs"
    N += 3  # (not a multiple of four: the signals' stream counts differ)
    rng = np.random.default_rng(C)
    signals = [noise(rng, 3 * chunk) for _ in range(4)]
    private = []
    for x in signals:
        private.append([comp.compute_chunk(x[t * chunk : (t + 1) * chunk]) for t in range(3)] + [comp.finalize()])
    assert sum(len(o) for o in private[0]) == comp.num_frames(3 * chunk) > 0
    ids = list(range(N))
    sb = SiStreamBatch(comp, capacity=N)
    try:
        calls = [sb.compute_chunks(ids, [signals[i % 4][t * chunk : (t + 1) * chunk] for i in ids]) for t in range(3)]
        calls.append(sb.finalize(ids))
    finally:
        sb.close()
    one_group = 0
    for t, outs in enumerate(calls):
        counts = [len(o) for o in outs]
        assert counts == [len(private[i % 4][t]) for i in ids], t
        if max(counts):
            made = launch_shape(comp, sum(c > 0 for c in counts), max(counts))
            assert made["groups"] == 1 and made["c_per_group"] == C, (t, made)
            one_group += 1
        for k in range(4):
            mine = [i for i in ids if i % 4 == k]
            for i in (mine[0], mine[len(mine) // 3], mine[2 * len(mine) // 3], mine[-1]):
                assert outs[i].dtype == private[k][t].dtype and np.array_equal(outs[i], private[k][t]), (t, i)
    assert one_group >= 2  # a tick and the finalize at least
