"""The fused STFT kernel's filter-walk tail: where the coefficients go, the log floor, the linear form, float64 stores.

Every walk ends the same way: a coefficient is floored and logged (or not), then stored at a wave-uniform row base
plus the lane's column offset, with lanes without a filter and frames past the utterance's end masked off.  These
tests check the values against the pinned oracle at the suite's float32 tolerance (numpy.allclose(rtol=1e-4,
atol=1e-5), see test_gpu_stft.py) and check that nothing outside the utterances' rows and the bank's columns is
written: the output buffers are pre-filled with a sentinel and compared byte for byte where the kernel must not
write.
"""
import json

import numpy as np
import pytest

from oracle import stft_oracle as orc
from pydrobert_speech_amd import config
from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg
from pydrobert_speech_amd.compute import FrameComputer
from tests.conftest import assert_features_close

pytestmark = pytest.mark.gpu
F32 = dict(rtol=1e-4, atol=1e-5)
SENTINEL = -12345.6789

CONFIGS = {
    # the headline bank (row-segment walk, N = 512)
    "tri_mel40": {"name": "stft", "bank": {"name": "tri", "scaling_function": "mel", "num_filts": 40},
                  "frame_length_ms": 25, "frame_shift_ms": 10, "window_function": "hanning", "use_power": True},
    # energy in column 0: the filters' columns start at 1
    "fbank80_energy": {"name": "stft", "bank": {"name": "fbank", "num_filts": 80}, "frame_length_ms": 25,
                       "include_energy": True, "use_power": True},
    # linear features: the tail without the floor and the log
    "tri_mel40_linear": {"name": "stft", "bank": {"name": "tri", "scaling_function": "mel", "num_filts": 40},
                         "frame_length_ms": 25, "use_power": True, "use_log": False},
    # a dense complex bank (segmented walks)
    "gabor64": {"name": "stft", "bank": {"name": "gabor", "scaling_function": "mel", "num_filts": 64},
                "frame_length_ms": 25, "use_power": True},
}


def build(cfg):
    return alias_factory_subclass_from_arg(FrameComputer, json.loads(json.dumps(cfg)))


def params(comp):
    return orc.StftParams(
        frame_length=comp.frame_length, frame_shift=comp.frame_shift, dft_size=comp.dft_size,
        window=np.asarray(comp._window), starts=list(comp._filt_start_idxs),
        taps=[np.asarray(t) for t in comp._truncated_filts], is_real=comp.bank.is_real,
        centered=comp.frame_style == "centered", kaldi_shift=comp.kaldi_shift,
        include_energy=comp.includes_energy, use_power=bool(comp._power), use_log=bool(comp._log),
    )


def ragged_lengths(comp):
    """Utterance lengths whose frame counts are 0, 1, 2 and 3 (mod 4), several of each"""
    S = comp.frame_shift
    lens, want = [], [1, 2, 3, 0, 1, 2, 3, 0, 3, 2, 1]
    for i, r in enumerate(want):
        n = (13 + 7 * i) * S + (S // 3) * (i % 2)
        while comp.num_frames(n) % 4 != r:
            n += S
        lens.append(n)
    return lens


def launch_into_sentinel(comp, sigs, dtype, out_dtype, extra_rows, width):
    """One launch of the packed batch into a (rows + extra_rows, width) buffer filled with the sentinel"""
    import torch

    lens = [len(x) for x in sigs]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    packed = torch.from_numpy(np.concatenate(sigs).astype(dtype)).cuda()
    layout = comp.prepare_layout(offs, lens, device=packed.device)
    total = int(layout.row_offsets[-1])
    out = torch.full((total + extra_rows, width), SENTINEL, dtype=out_dtype, device="cuda")
    got = comp.launch(packed, layout, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    return out.cpu().numpy(), layout.row_offsets


def check_buffer(buf, rows, C, sigs, p, what):
    ubits = np.dtype(f"u{buf.dtype.itemsize}")
    sentinel = np.array(SENTINEL, dtype=buf.dtype).view(ubits)
    bits = buf.view(ubits)
    total = int(rows[-1])
    # no byte outside the utterances' rows and the bank's columns changes
    assert (bits[total:] == sentinel).all(), (what, "rows past the batch were written")
    assert (bits[:, C:] == sentinel).all(), (what, "columns past the coefficients were written")
    for b, x in enumerate(sigs):
        assert_features_close(buf[rows[b] : rows[b + 1], :C], orc.compute_full(x, p), what=(what, b, len(x)), **F32)


@pytest.mark.parametrize("ragged", [True, False])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_ragged_batch_into_a_wider_buffer(name, ragged, monkeypatch):
    """Frame counts 1, 2 and 3 (mod 4) and a row stride of three times the coefficients (the two-launch deltas
    layout): the partial last chunks store only their frames, columns >= C and rows past the batch keep the sentinel"""
    import torch

    monkeypatch.setattr(config, "RAGGED_SCHEDULING", ragged)
    comp = build(CONFIGS[name])
    assert comp.kernel_kind, "a fused kernel serves this configuration"
    p = params(comp)
    rng = np.random.default_rng(11)
    sigs = [(3000 * rng.standard_normal(n)).astype("f4") for n in ragged_lengths(comp)]
    C = comp.num_coeffs
    buf, rows = launch_into_sentinel(comp, sigs, "f4", torch.float32, extra_rows=9, width=3 * C)
    check_buffer(buf, rows, C, sigs, p, (name, ragged))


@pytest.mark.parametrize("name", ["tri_mel40", "fbank80_energy"])
def test_exact_silence_hits_the_log_floor(name):
    """Noise bursts between stretches of exact zeros: the frames inside the silence have zero power, every
    coefficient there is log(floor), and the frames at the edges of the bursts sit just above it"""
    import torch

    comp = build(CONFIGS[name])
    p = params(comp)
    rng = np.random.default_rng(12)
    parts = []
    for burst, gap in ((800, 4000), (3000, 2500), (50, 6000), (1600, 0)):
        parts += [(3000 * rng.standard_normal(burst)).astype("f4"), np.zeros(gap, "f4")]
    x = np.concatenate(parts)
    sigs = [x, x[1234:], np.zeros(2 * comp.frame_length, "f4")]
    want = [orc.compute_full(s, p) for s in sigs]
    floor = np.log(p.log_floor).astype(want[0].dtype)  # (the oracle keeps the samples' dtype)
    assert sum(int((w == floor).sum()) for w in want) > 100  # (the floor is reached)
    C = comp.num_coeffs
    buf, rows = launch_into_sentinel(comp, sigs, "f4", torch.float32, extra_rows=3, width=C + 5)
    check_buffer(buf, rows, C, sigs, p, name)
    # the floor itself, as float32 computes it
    for b, w in enumerate(want):
        got = buf[rows[b] : rows[b + 1], :C]
        assert np.allclose(got[w == floor], floor, **F32)


@pytest.mark.parametrize("name", ["tri_mel40", "fbank80_energy", "tri_mel40_linear"])
def test_float64_features(name, monkeypatch):
    """float64 samples into the fused kernel with float64 features (8-byte stores at 8-byte column offsets), into a
    wider buffer; the float32-feature launch of the same kernel gives the same values, rounded"""
    import torch

    monkeypatch.setattr(config, "FLOAT64_ARITHMETIC", "float32")
    comp = build(CONFIGS[name])
    assert comp._native_plan().has_f64in
    p = params(comp)
    rng = np.random.default_rng(13)
    sigs = [3000 * rng.standard_normal(n) for n in ragged_lengths(comp)[:7]]
    C = comp.num_coeffs
    buf64, rows = launch_into_sentinel(comp, sigs, "f8", torch.float64, extra_rows=5, width=2 * C + 1)
    assert buf64.dtype == np.float64
    check_buffer(buf64, rows, C, sigs, p, (name, "f64"))
    buf32, _ = launch_into_sentinel(comp, sigs, "f8", torch.float32, extra_rows=5, width=2 * C + 1)
    total = int(rows[-1])
    assert np.array_equal(buf64[:total, :C].astype(np.float32), buf32[:total, :C])
