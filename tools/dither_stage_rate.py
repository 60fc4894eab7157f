#!/usr/bin/env python3
"""The dither stage of the command-line tool (command_line.py::FeatureDirWriter.process) alone: one
``Dither.apply_packed`` launch per batch against the per-utterance loop it replaced.

    python tools/dither_stage_rate.py [--utts 256] [--samples 16000] [--reps 30] >> profiles/<tag>.txt

A batch of `utts` utterances of `samples` 16-bit PCM samples each, packed on the GPU as ``process`` has it.  Timed, each
`reps` times after 5 untimed ones and ending in a synchronisation:

    loop      the packed int16 buffer widened to float32, then per utterance ``Dither(coeff, seed=s).apply(segment)``
              and a ``copy_`` back into the buffer -- what ``process`` did before
    packed    one ``apply_packed(float32 buffer, offsets, lengths, seeds)`` after the same widening (a batch of PCM and
              float files)
    packed16  one ``apply_packed(int16 buffer, ...)``: the widening rides along with the dither's load (a batch of PCM)

The three give the same samples (checked here).  Reports p50, minimum and maximum per form; nothing is asserted on the
times."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--samples", type=int, default=16000)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import torch

    from pydrobert_speech_amd.pre import Dither

    B, n = args.utts, args.samples
    pcm = torch.from_numpy(np.rint(3000 * np.random.default_rng(0).standard_normal(B * n)).astype(np.int16)).cuda()
    offsets = np.arange(B + 1, dtype=np.int64) * n
    lengths = np.full(B, n, dtype=np.int64)
    pre = Dither(1.0)
    seed = 11

    def loop():
        packed = pcm.to(torch.float32)
        for b in range(B):
            seg = packed[offsets[b] : offsets[b + 1]]
            seg.copy_(Dither(pre.coeff, seed=seed + b).apply(seg))
        return packed

    def packed():
        return pre.apply_packed(pcm.to(torch.float32), offsets[:-1], lengths, seeds=[seed + b for b in range(B)])

    def packed16():
        return pre.apply_packed(pcm, offsets[:-1], lengths, seeds=[seed + b for b in range(B)])

    want = loop()
    assert torch.equal(packed(), want) and torch.equal(packed16(), want)
    print(f"# {torch.cuda.get_device_name(0)}, dither stage of {B} utterances of {n} samples, {args.reps} repetitions")
    print(f"{'form':>9} {'p50 ms':>8} {'min ms':>8} {'max ms':>8}")
    for name, fn in (("loop", loop), ("packed", packed), ("packed16", packed16), ("loop", loop), ("packed", packed)):
        times = []
        for r in range(5 + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= 5:
                times.append(1e3 * (time.perf_counter() - t0))
        print(f"{name:>9} {np.median(times):>8.3f} {min(times):>8.3f} {max(times):>8.3f}")


if __name__ == "__main__":
    main()
