#!/usr/bin/env python3
"""The energy VAD (post.py EnergyVAD: ``pds_vad_energy_rows_f32`` and ``pds_select_rows_w32``) per call, against what a
user had before it: a torch formulation of the same rule over the packed batch.

    python tools/vad_rate.py [--utts 1024] [--frames 1000] [--coeffs 40] [--context 0] [--reps 50] >> profiles/<tag>.txt

`utts` utterances of `frames` float32 rows of `coeffs` values, packed on the GPU; column 0 is an energy that lies above
its utterance's threshold in stretches (about half the frames are voiced).  Timed with HIP events around `reps`
back-to-back calls after 10 untimed ones, the forms in turn and each twice (the run's own spread):

    decide_kernel  one ``pds_vad_energy_rows_f32`` launch into preallocated flags and counts (no synchronisation)
    decide_rows    ``EnergyVAD.decide_rows`` as a caller gets it: the launch, its two allocations and the fetch of the
                   counts, which synchronises
    select_kernel  one ``pds_select_rows_w32`` launch into a preallocated output, offsets on the device beforehand
    select_rows    ``EnergyVAD.select_rows`` with the mask of decide_rows: the counts derived from the mask (a cumsum and
                   a fetch), the offsets' upload, the output's allocation and the launch
    apply_rows     ``EnergyVAD.apply_rows``: decide_rows, then the selection with the counts it already has
    torch_decide   ``e.double().sum(1)`` per utterance, the threshold, ``e > thr``, a cumsum of the flags gathered at the
                   window's ends, the vote -- batched over all utterances at once, the window's ends on the device
                   beforehand
    torch_select   ``feats[voiced]``: boolean row indexing over the packed batch
    torch_apply    both

The torch sum is in another order than the rule's 64 partial sums, so a threshold may differ in its last bits and a
frame whose energy lies that close to it may be decided otherwise; the number of such frames is printed.  The kernels'
results equal the numpy model's bit for bit (tests/test_gpu_vad.py).  Reports the mean time per call, the rate over the
traffic the call must move (decide: the energy column and the flags, 5 bytes a row; select: the flags and the kept
rows once in and once out) and that rate's share of 8 TB/s; nothing is asserted on the times."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOFLINE = 8e12  # bytes per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--coeffs", type=int, default=40)
    ap.add_argument("--context", type=int, default=0)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    import torch

    from pydrobert_speech_amd import _native
    from pydrobert_speech_amd.post import EnergyVAD, _rows_meta

    B, T, C = args.utts, args.frames, args.coeffs
    vad = EnergyVAD(frames_context=args.context)
    gen = torch.Generator(device="cuda").manual_seed(0)
    feats = torch.randn((B * T, C), generator=gen, device="cuda", dtype=torch.float32)
    # energies in stretches of 50 frames, loud or quiet, with noise on top
    level = (torch.rand((B, -(-T // 50)), generator=gen, device="cuda") < 0.5).repeat_interleave(50, 1)[:, :T]
    feats[:, 0] = (8.0 + 10.0 * level + torch.randn((B, T), generator=gen, device="cuda")).reshape(-1)
    rows = np.arange(B + 1, dtype=np.int64) * T
    meta, _ = _rows_meta(rows, feats.device)
    lib = _native.stages_lib()
    stream = torch.cuda.current_stream().cuda_stream

    voiced, counts = vad.decide_rows(feats, rows)
    kept = int(counts.sum())
    out_off = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)).cuda()
    d_voiced, d_count = torch.zeros_like(voiced), torch.zeros(B, dtype=torch.int64, device="cuda")
    d_out = torch.empty((kept, C), dtype=torch.float32, device="cuda")

    def decide_kernel():
        rc = lib.pds_vad_energy_rows_f32(feats.data_ptr(), feats.stride(0), meta[0].data_ptr(), meta[1].data_ptr(), B, T,
                                         vad.energy_threshold, vad.energy_mean_scale, vad.frames_context,
                                         vad.proportion_threshold, d_voiced.data_ptr(), d_count.data_ptr(), stream)
        _native.check_stages(rc, "pds_vad_energy_rows")
        return d_voiced

    def select_kernel():
        rc = lib.pds_select_rows_w32(feats.data_ptr(), feats.stride(0), C, meta[0].data_ptr(), meta[1].data_ptr(), B, T,
                                     voiced.data_ptr(), out_off.data_ptr(), d_out.data_ptr(), C, stream)
        _native.check_stages(rc, "pds_select_rows")
        return d_out

    t = np.arange(T, dtype=np.int64)
    d_lo = torch.from_numpy(np.maximum(0, t - args.context)).cuda()
    d_hi1 = torch.from_numpy(np.minimum(T - 1, t + args.context) + 1).cuda()
    d_den = (d_hi1 - d_lo).double()[None, :] * vad.proportion_threshold
    zero = torch.zeros((B, 1), dtype=torch.int64, device="cuda")

    def torch_decide():
        e = feats.view(B, T, C)[:, :, 0].double()
        thr = vad.energy_threshold + (vad.energy_mean_scale * e.sum(1)) / T
        above = e > thr[:, None]
        c = torch.cat([zero, torch.cumsum(above, 1)], 1)
        return ((c[:, d_hi1] - c[:, d_lo]).double() >= d_den).reshape(-1)

    mask = voiced.bool()

    def torch_select():
        return feats[mask]

    def torch_apply():
        return feats[torch_decide()]

    forms = (
        ("decide_kernel", decide_kernel, 5 * B * T + 8 * B),
        ("decide_rows", lambda: vad.decide_rows(feats, rows), 5 * B * T + 8 * B),
        ("select_kernel", select_kernel, B * T + 8 * kept * C),
        ("select_rows", lambda: vad.select_rows(feats, rows, voiced), B * T + 8 * kept * C),
        ("apply_rows", lambda: vad.apply_rows(feats, rows), 6 * B * T + 8 * B + 8 * kept * C),
        ("torch_decide", torch_decide, 5 * B * T + 8 * B),
        ("torch_select", torch_select, B * T + 8 * kept * C),
        ("torch_apply", torch_apply, 6 * B * T + 8 * B + 8 * kept * C),
    )
    # what the forms give: the kernels' and the callers' results are the same; torch's differ only near a threshold
    assert torch.equal(decide_kernel(), voiced) and torch.equal(d_count.cpu(), torch.from_numpy(counts))
    want = feats[mask]
    assert torch.equal(select_kernel(), want) and torch.equal(vad.select_rows(feats, rows, voiced)[0], want)
    assert torch.equal(vad.apply_rows(feats, rows)[0], want)
    differ = int((torch_decide() != mask).sum().item())
    assert differ <= 1e-4 * B * T, differ
    print(f"# {torch.cuda.get_device_name(0)}, {B} utterances x {T} frames x {C} float32, energy_threshold "
          f"{vad.energy_threshold}, energy_mean_scale {vad.energy_mean_scale}, frames_context {vad.frames_context}, "
          f"proportion_threshold {vad.proportion_threshold}; {kept} of {B * T} frames voiced; {args.reps} calls per "
          f"measurement; torch decides {differ} frames otherwise (its sum is in another order)")
    print(f"{'form':>14} {'ms/call':>10} {'GB/s':>8} {'of 8 TB/s':>10}")
    for name, fn, traffic in forms * 2:
        for _ in range(10):
            fn()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.reps):
            fn()
        end.record()
        end.synchronize()
        ms = start.elapsed_time(end) / args.reps
        rate = traffic / (ms * 1e-3)
        print(f"{name:>14} {ms:>10.4f} {rate / 1e9:>8.0f} {100 * rate / ROOFLINE:>9.2f}%")


if __name__ == "__main__":
    main()
