#!/usr/bin/env python3
"""Rate of the headline configuration on SHORT utterances, where the items at a signal end are a large share.

    [PDS_AMD_LIB=variants/lib_x.so] python tools/edge_items_rate.py [--steps 200] [--seconds 1 2 5 10] [--dtype f32]

An item of the fused STFT kernel is four consecutive frames of one utterance; the first and the last item of every
utterance reach past a signal end and gather their rows with reflected indices (csrc/stft_wave_kernel.h).  At 10 s
that is 2 items of 250, at 1 s 2 of 25.  Batches of 1024 utterances of equal length through prepare_layout / launch,
clocks pre-rolled and steps timed with events as bench.py does; one JSON line per length.  Run it under two builds of
the library (tools/build_variant.sh, -DPDS_EDGE_STRAIGHT=0 for the rolled gather) to compare them.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CFG = {"name": "stft", "bank": {"name": "tri", "scaling_function": "mel", "num_filts": 40}, "frame_length_ms": 25,
       "frame_shift_ms": 10, "window_function": "hanning", "use_power": True}  # bench.py's default workload


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--seconds", type=float, nargs="+", default=[1.0, 2.0, 5.0])
    ap.add_argument("--dtype", default="f32", choices=["f32", "i16in", "f64in"])
    ap.add_argument("--preemph", type=float, default=0.0)
    args = ap.parse_args()

    import numpy as np
    import torch

    import pydrobert_speech_amd as ps
    from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg

    comp = alias_factory_subclass_from_arg(ps.compute.FrameComputer, json.loads(json.dumps(CFG)))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.dtype == "f64in":
        ps.config.FLOAT64_ARITHMETIC = "float32"
    for secs in args.seconds:
        n, B = int(round(secs * comp.sampling_rate)), args.batch
        g = torch.Generator(device=dev).manual_seed(1234)
        signal = torch.randn(B * n, generator=g, device=dev, dtype=torch.float32).mul_(3000.0)
        if args.dtype == "f64in":
            signal = signal.double()
        elif args.dtype == "i16in":
            signal = signal.clamp_(-32768, 32767).to(torch.int16)
        layout = comp.prepare_layout(np.arange(B, dtype=np.int64) * n, np.full(B, n, dtype=np.int64), device=dev)
        out = torch.empty((layout.total_rows, comp.num_coeffs), dtype=torch.float32, device=dev)

        def step():
            comp.launch(signal, layout, out=out, preemphasis=args.preemph)

        # pre-roll as bench.py: blocks of 20 steps until eight in a row have not beaten the fastest by 0.5 %, at most 2 s
        step()
        torch.cuda.synchronize(dev)
        t_start, best, settled = time.perf_counter(), float("inf"), 0
        while True:
            t_block = time.perf_counter()
            for _ in range(20):
                step()
            torch.cuda.synchronize(dev)
            now = time.perf_counter()
            settled = 0 if now - t_block < 0.995 * best else settled + 1
            best = min(best, now - t_block)
            if (now - t_start >= 0.06 and settled >= 8) or now - t_start > 2.0:
                break
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize(dev)
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        marks[0].record()
        for i in range(args.steps):
            step()
            marks[i + 1].record()
        torch.cuda.synchronize(dev)
        ms = np.array([marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps)])
        chunks = -(-comp.num_frames(n) // 4)
        print(json.dumps({
            "seconds": secs, "batch": B, "dtype": args.dtype, "preemph": args.preemph, "frames": int(layout.total_rows),
            "edge_item_share": round(min(2, chunks) / chunks, 4), "kernel_ms_avg": round(float(ms.mean()), 5),
            "kernel_ms_median": round(float(np.median(ms)), 5), "kernel_ms_min": round(float(ms.min()), 5),
            "frames_per_s": round(layout.total_rows / (1e-3 * float(ms.mean())), 1),
            "lib": os.path.basename(ps.LIB_PATH)}), flush=True)


if __name__ == "__main__":
    main()
