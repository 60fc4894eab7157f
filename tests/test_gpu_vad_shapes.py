"""``vad_energy_kernel`` and ``select_rows_kernel`` (csrc/vad.hip) at the smallest shapes at which each launch can go
wrong, against ``tests/vad_model.py``: decisions are equal, selected rows are the same bytes.

Both are driven through their C entry points with buffers of the test's own.  The decision: utterances of 0 to 1000
frames around the wave's 64 and the unrolled 256 in one batch, contexts from 0 to beyond the utterance, and 70,000
utterances of one to three rows with one of 20,000 rows among them.  The selection: rows of 1, 40 and 257 values (the
copy runs from one kept row on into the next; 257 is more than a block), as 32-bit and as 64-bit elements, strides
larger than the rows, masks that keep all, none and every other row, rows of raw bit patterns (NaN payloads, -0.0).
What a kernel must not read is NaN or a huge energy (gap rows, pad columns); what it must not write holds canaries that
are compared afterwards, byte for byte."""
import functools

import numpy as np
import pytest

from pydrobert_speech_amd import _native
from tests.vad_model import threshold, vad_decide

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000]
CANARY = 0xAB
COUNT_CANARY = -7777


def layout(lens):
    """row offsets of utterances of `lens` rows with one gap row in front of each, and the buffer's rows"""
    lens = np.asarray(lens, dtype=np.int64)
    offs = 1 + np.cumsum(lens + 1) - (lens + 1)
    return offs, int(offs[-1] + lens[-1] + 2)


def launch_decide(energies, offs, lens, total, dtype, thr, scale, context, prop, lead=1, stride=3):
    """``pds_vad_energy_rows_*`` over the utterances' `energies` laid into column `lead` of a ``(total, stride)``
    buffer whose every other value is NaN.  Returns ``(voiced, counts)`` with their canaries checked: the uint8
    ``(total,)`` flags (CANARY where no utterance has a row) and the int64 ``(B,)`` counts"""
    import torch

    lib = _native.stages_lib()
    fn = lib.pds_vad_energy_rows_f32 if dtype == np.float32 else lib.pds_vad_energy_rows_f64
    buf = np.full((total, stride), np.nan, dtype=dtype)
    for e, o in zip(energies, offs):
        buf[o : o + len(e), lead] = e
    B = len(lens)
    d_in = torch.from_numpy(buf).cuda()
    d_meta = torch.from_numpy(np.stack([offs, lens]).astype(np.int64)).cuda()
    d_voiced = torch.full((total + 128,), CANARY, dtype=torch.uint8, device="cuda")  # 64 canaries on either side
    d_count = torch.full((B + 2,), COUNT_CANARY, dtype=torch.int64, device="cuda")  # one on either side
    assert (offs >= 1).all() and int((offs + lens).max()) < total
    rc = fn(d_in.data_ptr() + lead * buf.itemsize, stride, d_meta[0].data_ptr(), d_meta[1].data_ptr(), B,
            int(lens.max()), thr, scale, context, prop, d_voiced.data_ptr() + 64, d_count.data_ptr() + 8,
            torch.cuda.current_stream().cuda_stream)
    _native.check_stages(rc, "pds_vad_energy_rows")
    voiced, counts = d_voiced.cpu().numpy(), d_count.cpu().numpy()
    assert (voiced[:64] == CANARY).all() and (voiced[-64:] == CANARY).all()
    assert counts[0] == COUNT_CANARY and counts[-1] == COUNT_CANARY
    assert d_in.cpu().numpy().tobytes() == buf.tobytes()  # (the input is left alone)
    return voiced[64:-64], counts[1:-1]


def check_decide(energies, dtype, thr, scale, context, prop, what):
    lens = np.asarray([len(e) for e in energies], dtype=np.int64)
    offs, total = layout(lens)
    expect = np.full(total, CANARY, dtype=np.uint8)
    want_counts = []
    for e, o in zip(energies, offs):
        v = vad_decide(e, thr, scale, context, prop)
        expect[o : o + len(e)] = v
        want_counts.append(int(v.sum()))
    voiced, counts = launch_decide(energies, offs, lens, total, dtype, thr, scale, context, prop)
    bad = np.flatnonzero(voiced != expect)
    assert not len(bad), (what, len(bad), bad[:5].tolist(), voiced[bad[:5]].tolist(), expect[bad[:5]].tolist())
    assert counts.tolist() == want_counts, what
    return sum(want_counts), int(lens.sum())


@functools.lru_cache(maxsize=None)
def mixed_batch(dtype):
    """utterances of LENGTHS frames, shuffled, energies on both sides of their thresholds"""
    rng = np.random.default_rng(64)
    order = rng.permutation(len(LENGTHS))
    return tuple((12.0 + 6.0 * rng.standard_normal(LENGTHS[i])).astype(dtype) for i in order)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("context", [0, 1, 7])
def test_lengths_around_the_wave_and_the_unrolled_chunk(context, dtype):
    energies = mixed_batch(dtype)
    for scale, thr, prop in ((0.5, 5.0, 0.6), (0.0, 12.0, 0.5), (0.25, 12.0, 0.3)):
        kept, rows = check_decide(energies, dtype, thr, scale, context, prop, (scale, context))
        assert 0.1 * rows < kept < 0.9 * rows


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("beyond", [-1, 3], ids=["T-1", "T+3"])
def test_contexts_that_reach_the_utterances_ends(beyond, dtype):
    """``frames_context`` of T - 1 and T + 3 for every T of LENGTHS, with all the lengths in the batch each time: the
    window is the whole utterance for that T and the shorter ones, and is cut at one end or both for the longer"""
    energies = mixed_batch(dtype)
    for T in LENGTHS:
        context = T + beyond
        if context < 0:
            continue
        check_decide(energies, dtype, 5.0, 0.5, context, 0.6, (T, beyond))
    check_decide(energies, dtype, 5.0, 0.5, (1 << 31) - 1, 0.5, "the largest context")


def decide_columns(E, thr, scale, context, prop):
    """the model over utterances of one length side by side: `E` is ``(T, N)``; bool ``(T, N)``"""
    E = E.astype(np.float64)
    T = len(E)
    above = E > threshold(E, thr, scale)[None, :]
    out = np.zeros(E.shape, dtype=bool)
    for t in range(T):
        lo, hi = max(0, t - context), min(T - 1, t + context)
        out[t] = above[lo : hi + 1].sum(axis=0).astype(np.float64) >= float(hi - lo + 1) * prop
    return out


@functools.lru_cache(maxsize=None)
def many_utterances(dtype, context):
    """70,000 utterances of 1, 2, 3, 1, .. rows and one of 20,000 rows in the middle: their energies laid out with gap
    rows, and the model's decisions (utterances of one length are the columns of one call)"""
    B, long_at, long_rows = 70000, 35000, 20000
    rng = np.random.default_rng(70 + context)
    lens = 1 + np.arange(B, dtype=np.int64) % 3
    lens[long_at] = long_rows
    offs, total = layout(lens)
    energy = np.full(total, 1e6, dtype=dtype)  # (a gap row read by mistake moves a threshold)
    expect = np.full(total, CANARY, dtype=np.uint8)
    counts = np.zeros(B, dtype=np.int64)
    for T in (1, 2, 3):
        idx = np.flatnonzero(lens == T)
        E = (12.0 + 6.0 * rng.standard_normal((T, len(idx)))).astype(dtype)
        rows = offs[idx][None, :] + np.arange(T)[:, None]
        energy[rows] = E
        V = decide_columns(E, 5.0, 0.5, context, 0.5)
        expect[rows] = V
        counts[idx] = V.sum(axis=0)
    e = (12.0 + 6.0 * rng.standard_normal(long_rows)).astype(dtype)
    v = vad_decide(e, 5.0, 0.5, context, 0.5)
    # (the vectorised model is the model: checked on the long utterance's first rows as three short ones)
    assert (decide_columns(e[:3, None], 5.0, 0.5, context, 0.5)[:, 0] == vad_decide(e[:3], 5.0, 0.5, context, 0.5)).all()
    energy[offs[long_at] : offs[long_at] + long_rows] = e
    expect[offs[long_at] : offs[long_at] + long_rows] = v
    counts[long_at] = v.sum()
    return lens, offs, total, energy, expect, counts


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("context", [0, 1])
def test_seventy_thousand_short_utterances_and_a_long_one(context, dtype):
    """70,000 waves, most with one to three frames; one walks 20,000 frames.  Then the selection of the same batch:
    70,000 x 79 blocks, all but a few of which find their tile past the utterance's end"""
    import torch

    lens, offs, total, energy, expect, want_counts = many_utterances(dtype, context)
    lib = _native.stages_lib()
    fn = lib.pds_vad_energy_rows_f32 if dtype == np.float32 else lib.pds_vad_energy_rows_f64
    B = len(lens)
    d_energy = torch.from_numpy(energy).cuda()
    d_meta = torch.from_numpy(np.stack([offs, lens])).cuda()
    d_voiced = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    d_count = torch.full((B + 2,), COUNT_CANARY, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rc = fn(d_energy.data_ptr(), 1, d_meta[0].data_ptr(), d_meta[1].data_ptr(), B, int(lens.max()), 5.0, 0.5, context,
            0.5, d_voiced.data_ptr(), d_count.data_ptr() + 8, stream)
    _native.check_stages(rc, "pds_vad_energy_rows")
    voiced, counts = d_voiced.cpu().numpy(), d_count.cpu().numpy()
    bad = np.flatnonzero(voiced != expect)
    assert not len(bad), (len(bad), bad[:5].tolist(), voiced[bad[:5]].tolist(), expect[bad[:5]].tolist())
    assert counts[0] == COUNT_CANARY and counts[-1] == COUNT_CANARY and (counts[1:-1] == want_counts).all()
    assert 0.2 * lens.sum() < want_counts.sum() < 0.8 * lens.sum()
    # the selection, with the mask as the decision left it: CANARY (not 0) in the gap rows, which are nobody's
    C, in_stride, out_stride = 3, 4, 5
    rng = np.random.default_rng(context)
    rows_in = rng.integers(0, 1 << 32, size=(total, in_stride), dtype=np.uint32)
    out_offs = np.concatenate([[0], np.cumsum(want_counts)]).astype(np.int64)
    kept_rows = int(out_offs[-1])
    before = rng.integers(0, 1 << 32, size=(kept_rows + 2, out_stride), dtype=np.uint32)
    member = np.zeros(total, dtype=bool)
    member[np.repeat(offs, lens) + (np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens))] = True
    assert member.sum() == lens.sum() and (expect[~member] == CANARY).all()
    want = before.copy()
    want[1 : 1 + kept_rows, 1 : 1 + C] = rows_in[member & (expect == 1)][:, :C]  # (utterances lie in ascending rows)
    d_in, d_out = torch.from_numpy(rows_in).cuda(), torch.from_numpy(before).cuda()
    d_out_offs = torch.from_numpy(out_offs[:-1] + 1).cuda()  # (one row of canaries in front)
    rc = lib.pds_select_rows_w32(d_in.data_ptr(), in_stride, C, d_meta[0].data_ptr(), d_meta[1].data_ptr(), B,
                                 int(lens.max()), d_voiced.data_ptr(), d_out_offs.data_ptr(), d_out.data_ptr() + 4,
                                 out_stride, stream)
    _native.check_stages(rc, "pds_select_rows")
    got = d_out.cpu().numpy()
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:5].tolist()


# ---- the selection -------------------------------------------------------------------------------------------------


def masks(total, rng):
    alternate = (np.arange(total) % 2).astype(np.uint8)
    random = (rng.random(total) < 0.4).astype(np.uint8) * rng.integers(1, 256, size=total).astype(np.uint8)
    return {"all": np.full(total, 1, np.uint8), "none": np.zeros(total, np.uint8), "alternate": alternate,
            "other": (1 - alternate).astype(np.uint8), "random": random}


@pytest.mark.parametrize("per", [1, 2], ids=["w32", "w64"])
@pytest.mark.parametrize("C", [1, 40, 257])
def test_selection_of_rows_of_every_width(C, per):
    """rows of `C` elements of `per` 32-bit words, input rows 2 elements and output rows 3 elements longer than that,
    both starting one element into their buffers"""
    import torch

    lib = _native.stages_lib()
    rng = np.random.default_rng(100 * C + per)
    lens = np.asarray([LENGTHS[i] for i in rng.permutation(len(LENGTHS))], dtype=np.int64)
    offs, total = layout(lens)
    words, in_stride, out_stride = C * per, (C + 2) * per, (C + 3) * per
    rows_in = rng.integers(0, 1 << 32, size=(total, in_stride), dtype=np.uint32)
    # NaNs with payloads, -0.0 and denormals among the bit patterns, as float32 and as the halves of a float64
    rows_in[::7, per] = 0x7FC12345
    rows_in[1::7, per] = 0xFFF00001
    rows_in[2::7, per] = 0x80000000
    rows_in[3::7, per : 2 * per] = 0
    rows_in[3::7, 2 * per - 1] = 0x80000000
    member = np.zeros(total, dtype=bool)
    for o, n in zip(offs, lens):
        member[o : o + n] = True
    d_in = torch.from_numpy(rows_in).cuda()
    d_meta = torch.from_numpy(np.stack([offs, lens])).cuda()
    for name, keep in masks(total, rng).items():
        counts = np.asarray([int((keep[o : o + n] != 0).sum()) for o, n in zip(offs, lens)], dtype=np.int64)
        # every utterance's rows at an offset of their own choosing: in reverse order of the utterances, a free row between
        sizes = counts + 1
        starts = np.cumsum(sizes[::-1])[::-1] - sizes + 1
        out_rows = int(sizes.sum()) + 2
        before = rng.integers(0, 1 << 32, size=(out_rows, out_stride), dtype=np.uint32)
        want = before.copy()
        for o, n, s in zip(offs, lens, starts):
            picked = rows_in[o : o + n][keep[o : o + n] != 0]
            want[s : s + len(picked), per : per + words] = picked[:, per : per + words]
        d_keep = torch.from_numpy(keep).cuda()
        d_out = torch.from_numpy(before).cuda()
        d_starts = torch.from_numpy(starts.astype(np.int64)).cuda()
        rc = lib.pds_select_rows_w32(d_in.data_ptr() + 4 * per, in_stride, words, d_meta[0].data_ptr(),
                                     d_meta[1].data_ptr(), len(lens), int(lens.max()), d_keep.data_ptr(),
                                     d_starts.data_ptr(), d_out.data_ptr() + 4 * per, out_stride,
                                     torch.cuda.current_stream().cuda_stream)
        _native.check_stages(rc, "pds_select_rows")
        got = d_out.cpu().numpy()
        assert got.tobytes() == want.tobytes(), (name, np.argwhere(got != want)[:5].tolist())
        if name == "all":
            assert counts.tolist() == lens.tolist()
        assert (keep[~member] != 0).any() or name == "none"  # (flags of rows of no utterance are set and ignored)
    assert d_in.cpu().numpy().tobytes() == rows_in.tobytes()


def test_rows_beyond_max_rows_are_not_looked_at():
    """``max_rows`` sizes the grid: an utterance's tiles past it are not launched, and neither call touches a pointer
    when it is 0"""
    import torch

    lib = _native.stages_lib()
    rng = np.random.default_rng(3)
    lens, offs = np.asarray([700], dtype=np.int64), np.asarray([0], dtype=np.int64)
    rows_in = rng.integers(0, 1 << 32, size=(700, 2), dtype=np.uint32)
    before = rng.integers(0, 1 << 32, size=(700, 2), dtype=np.uint32)
    d_in, d_out = torch.from_numpy(rows_in).cuda(), torch.from_numpy(before).cuda()
    d_meta = torch.from_numpy(np.stack([offs, lens, offs])).cuda()
    d_keep = torch.ones(700, dtype=torch.uint8, device="cuda")
    rc = lib.pds_select_rows_w32(d_in.data_ptr(), 2, 2, d_meta[0].data_ptr(), d_meta[1].data_ptr(), 1, 300,
                                 d_keep.data_ptr(), d_meta[2].data_ptr(), d_out.data_ptr(), 2, None)
    _native.check_stages(rc, "pds_select_rows")
    torch.cuda.synchronize()
    want = before.copy()
    want[:512] = rows_in[:512]  # two tiles of 256 rows
    assert d_out.cpu().numpy().tobytes() == want.tobytes()
    assert lib.pds_select_rows_w32(1, 2, 2, 1, 1, 1, 0, 1, 1, 1, 2, None) == 0
    assert lib.pds_vad_energy_rows_f32(1, 1, 1, 1, 1, 0, 5.0, 0.5, 0, 0.6, 1, 1, None) == 0
