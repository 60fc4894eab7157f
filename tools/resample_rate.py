#!/usr/bin/env python3
"""The rate-conversion kernels (``pds_resample_packed_*``, pre.Resample; ``pds_multistream_resample_*``,
multistream_resample.ResampleBatch) alone, against what a user would write without them: a torch float64 polyphase
``conv1d``.

    python tools/resample_rate.py [--utts 1024] [--seconds 10] [--reps 50] [--streams 1024] [--ticks 100]
                                  >> profiles/<tag>.txt

Offline: `utts` utterances of `seconds` each, packed on the GPU, at 8 -> 16 kHz and 44.1 -> 16 kHz, as int16 and as
float32.  Timed with HIP events around `reps` back-to-back launches after 10 untimed ones, each form twice (the run's
own spread):

    kernel   one ``pds_resample_packed_*`` launch into a preallocated output
    apply    ``Resample.apply_packed`` as a caller gets it (offsets up, the launch, the output's allocation)
    conv1d   the samples as float64 ``(utts, 1, n)``, zero-padded, through ``torch.nn.functional.conv1d`` with the
             weight table as a ``(out_unit, 1, taps)`` kernel (every phase's taps at its own offset) and stride
             ``in_unit``, transposed into sample order and cast back; fewer repetitions where it is slow

The kernel's samples equal the numpy model's bit for bit (tests/test_gpu_resample.py); the conv1d's agree with them to
rounding, which is checked here.  GB/s is over the algorithmic traffic, one read of the input and one write of the
output.  Streaming: `streams` streams with 10 ms chunks at 8 kHz, packed, host time per tick with and without a
``StreamBatch`` tick (40-mel filter bank) behind it.  Nothing is asserted on the times."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def offline(args, from_rate, to_rate, dtype):
    import torch

    from pydrobert_speech_amd import _native
    from pydrobert_speech_amd.pre import Resample

    rs = Resample(from_rate, to_rate)
    B, n = args.utts, from_rate * args.seconds
    m = rs.num_output_samples(n)
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = (3000 * torch.randn(B * n, generator=gen, device="cuda")).round()
    x = x.clamp(-32768, 32767).to(torch.int16) if dtype == "int16" else x
    offs, lens = np.arange(B, dtype=np.int64) * n, np.full(B, n, dtype=np.int64)
    out = torch.empty(B * m, dtype=torch.float32, device="cuda")
    table = torch.from_numpy(np.stack([offs, lens, np.arange(B, dtype=np.int64) * m])).cuda()
    first, ntaps, weights = rs._tables(x.device)
    lib = _native.stages_lib()
    fn = lib.pds_resample_packed_i16_f32 if dtype == "int16" else lib.pds_resample_packed_f32
    stream = torch.cuda.current_stream().cuda_stream

    def kernel():
        rc = fn(x.data_ptr(), table[0].data_ptr(), table[1].data_ptr(), table[2].data_ptr(), B, n, rs.in_unit,
                rs.out_unit, rs.max_taps, first.data_ptr(), ntaps.data_ptr(), weights.data_ptr(), out.data_ptr(), stream)
        _native.check_stages(rc, "pds_resample_packed")
        return out

    def apply():
        return rs.apply_packed(x, offs, lens)[0]

    # every phase's taps at its own offset in one kernel of `width` taps; output unit u of phase p reads from
    # u * in_unit + first[p], so the samples are padded by -min(first) in front
    lo = int(rs.first.min())
    width = int((rs.first + rs.ntaps).max()) - lo
    kern = np.zeros((rs.out_unit, 1, width))
    for p in range(rs.out_unit):
        kern[p, 0, rs.first[p] - lo : rs.first[p] - lo + rs.ntaps[p]] = rs.weights[p, : rs.ntaps[p]]
    d_kern = torch.from_numpy(kern).cuda()
    units = -(-m // rs.out_unit)
    back = max(0, (units - 1) * rs.in_unit + width - (n - lo))

    def conv1d():
        xd = torch.nn.functional.pad(x.view(B, 1, n).double(), (-lo, back))
        y = torch.nn.functional.conv1d(xd, d_kern, stride=rs.in_unit)  # (B, out_unit, units)
        return y.transpose(1, 2).reshape(B, -1)[:, :m].float().reshape(-1)

    want = kernel().clone()
    assert torch.equal(apply(), want)
    traffic = B * (n * x.element_size() + m * 4)
    rows = []
    forms = [("kernel", kernel, args.reps), ("apply", apply, args.reps)]
    try:
        got = conv1d()
        err, scale = (got - want).abs().max().item(), want.abs().max().item()
        assert err <= 1e-6 * scale, (err, scale)  # (float32 results of float64 sums in another order)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        conv1d()
        torch.cuda.synchronize()
        once = (time.perf_counter() - t0) * 1e3
        forms.append(("conv1d", conv1d, max(2, min(args.reps, int(3000 / max(once, 1e-3))))))
        note = f"conv1d within {err:.2e} of the kernel's samples (largest {scale:.0f})"
    except (RuntimeError, torch.OutOfMemoryError) as exc:
        note = f"conv1d unavailable: {str(exc).splitlines()[0][:120]}"
    print(f"# {from_rate} -> {to_rate} Hz, {dtype}: {B} x {n} samples -> {m}, in_unit {rs.in_unit}, out_unit "
          f"{rs.out_unit}, taps {int(rs.ntaps.min())}-{rs.max_taps}, {traffic / 1e6:.0f} MB of algorithmic traffic; {note}")
    for name, form, reps in forms * 2:
        for _ in range(10 if name != "conv1d" else 1):
            form()
        ms = timed(form, reps)
        rows.append((name, ms))
        print(f"{name:>7} {ms:>10.4f} ms/launch {traffic / ms / 1e6:>8.0f} GB/s {B * m / ms / 1e6:>8.2f} G outputs/s"
              f"  ({reps} launches)")
    return rows


def streaming(args):
    import json

    import torch

    from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg
    from pydrobert_speech_amd.compute import FrameComputer
    from pydrobert_speech_amd.multistream import StreamBatch
    from pydrobert_speech_amd.multistream_resample import ResampleBatch
    from pydrobert_speech_amd.pre import Resample

    S, c = args.streams, 80
    comp = alias_factory_subclass_from_arg(FrameComputer, json.loads(
        '{"name": "stft", "bank": {"name": "fbank", "num_filts": 40}, "frame_length_ms": 25, "use_power": true}'))
    ids, lens = np.arange(S), np.full(S, c, dtype=np.int64)
    gen = torch.Generator(device="cuda").manual_seed(1)
    print(f"# streaming: {S} streams, {c}-sample chunks (10 ms at 8 kHz) -> 16 kHz, packed, {args.ticks} ticks per "
          "measurement, host time per tick (synchronised at the end)")
    for dtype in (np.float32, np.int16):
        chunk = (3000 * torch.randn(S * c, generator=gen, device="cuda")).round().to(getattr(torch, np.dtype(dtype).name))
        for behind in (False, True) * 2:
            with ResampleBatch(Resample(8000, 16000), S, dtype) as rb, StreamBatch(comp, capacity=S) as sb:
                def tick():
                    d_out, out_lens = rb.resample_chunks_packed(ids, chunk, lens)
                    if behind:
                        sb.compute_chunks_packed(ids, d_out, out_lens)

                for _ in range(10):
                    tick()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.ticks):
                    tick()
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3 / args.ticks
            what = "resample + StreamBatch tick" if behind else "resample alone"
            print(f"{np.dtype(dtype).name:>8} {what:>28} {ms:>9.4f} ms/tick {S * c / ms / 1e3:>8.2f} M input samples/s"
                  f" ({S * 0.01 / (ms / 1e3):.0f} x real time)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=1024)
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--ticks", type=int, default=100)
    args = ap.parse_args()
    import torch

    print(f"# {torch.cuda.get_device_name(0)}, {args.reps} launches per measurement")
    for from_rate, to_rate in ((8000, 16000), (44100, 16000)):
        for dtype in ("int16", "float32"):
            offline(args, from_rate, to_rate, dtype)
            torch.cuda.empty_cache()
    streaming(args)


if __name__ == "__main__":
    main()
