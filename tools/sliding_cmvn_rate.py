#!/usr/bin/env python3
"""The sliding-window CMVN kernel (``pds_sliding_cmvn_rows_f32``, post.py SlidingCMVN) alone, against what a user had
before it: a torch float64 ``cumsum`` formulation of the same window.

    python tools/sliding_cmvn_rate.py [--utts 1024] [--frames 1000] [--coeffs 40] [--window 600] [--min-window 100]
                                      [--center] [--norm-vars] [--refresh R] [--reps 50] >> profiles/<tag>.txt

`utts` utterances of `frames` float32 rows of `coeffs` values, packed on the GPU.  Timed with HIP events around `reps`
back-to-back launches after 10 untimed ones, the forms in turn and each twice (the run's own spread):

    kernel   one ``pds_sliding_cmvn_rows_f32`` launch into a preallocated output
    apply    ``SlidingCMVN.apply_rows(feats, row_offsets)`` as a caller gets it (the launch and the output's allocation)
    cumsum   per utterance ``c = cumsum(x.double())`` (and of the squares with --norm-vars) with a zero row in front,
             ``s = c[we] - c[ws]`` gathered by the precomputed window ends, mean, variance and the normalisation in
             float64, cast back -- batched over all utterances at once, the window ends on the device beforehand

The kernel's rows equal the numpy model's bit for bit (tests/test_gpu_sliding.py); the cumsum's agree with them to
rounding, which is checked here.  Reports the mean time per launch and the rate over the algorithmic traffic, one read
and one write of every element; nothing is asserted on the times."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window_ends(T, W, min_window, center):
    """``(ws, we)`` int64 arrays of the `T` frames (the rule of post.SlidingCMVN, vectorised)"""
    t = np.arange(T, dtype=np.int64)
    if center:
        ws = t - W // 2
        we = ws + W
    else:
        ws = t - W
        we = t + 1
    neg = ws < 0
    we = np.where(neg, we - ws, we)
    ws = np.where(neg, 0, ws)
    if not center:
        we = np.where(we > t, np.maximum(t + 1, min_window), we)
    over = we > T
    ws = np.where(over, np.maximum(ws - (we - T), 0), ws)
    we = np.where(over, T, we)
    return ws, we


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--coeffs", type=int, default=40)
    ap.add_argument("--window", type=int, default=600)
    ap.add_argument("--min-window", type=int, default=100)
    ap.add_argument("--center", action="store_true")
    ap.add_argument("--norm-vars", action="store_true")
    ap.add_argument("--refresh", type=int, default=None)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    import torch

    from pydrobert_speech_amd import _native
    from pydrobert_speech_amd.post import SlidingCMVN, _rows_meta

    B, T, C = args.utts, args.frames, args.coeffs
    post = SlidingCMVN(args.window, args.min_window, args.center, args.norm_vars, args.refresh)
    gen = torch.Generator(device="cuda").manual_seed(0)
    feats = 5 * torch.randn((B * T, C), generator=gen, device="cuda", dtype=torch.float32) + 20
    out = torch.empty_like(feats)
    rows = np.arange(B + 1, dtype=np.int64) * T
    meta, _ = _rows_meta(rows, feats.device)
    lib = _native.stages_lib()
    stream = torch.cuda.current_stream().cuda_stream

    def kernel():
        rc = lib.pds_sliding_cmvn_rows_f32(feats.data_ptr(), feats.stride(0), meta[0].data_ptr(), meta[1].data_ptr(), B,
                                           T, C, post.cmn_window, post.min_window, int(post.center),
                                           int(post.norm_vars), post.refresh, out.data_ptr(), out.stride(0), stream)
        _native.check_stages(rc, "pds_sliding_cmvn_rows")
        return out

    def apply():
        return post.apply_rows(feats, rows)

    ws, we = window_ends(T, post.cmn_window, post.min_window, post.center)
    d_ws, d_we = torch.from_numpy(ws).cuda(), torch.from_numpy(we).cuda()
    d_n = (d_we - d_ws).double()[None, :, None]
    zero = torch.zeros((B, 1, C), dtype=torch.float64, device="cuda")

    def cumsum():
        x = feats.view(B, T, C).double()
        c = torch.cat([zero, torch.cumsum(x, 1)], 1)
        mean = (c[:, d_we] - c[:, d_ws]) / d_n
        y = x - mean
        if post.norm_vars:
            c2 = torch.cat([zero, torch.cumsum(x * x, 1)], 1)
            var = ((c2[:, d_we] - c2[:, d_ws]) / d_n - mean * mean).clamp_min(1e-10)
            y = torch.where(d_n == 1, torch.zeros_like(y), y / var.sqrt())
        return y.float().view(B * T, C)

    want = kernel().clone()
    assert torch.equal(apply(), want)
    err = (cumsum() - want).abs().max().item()
    scale = want.abs().max().item()
    # (the prefix sums carry T terms of magnitude ~20 where the kernel's carry a window's: rounding of 1e-16 * 20 T)
    assert err <= 1e-6 * max(scale, 1.0), (err, scale)
    traffic = 2 * B * T * C * 4
    print(f"# {torch.cuda.get_device_name(0)}, {B} utterances x {T} frames x {C} float32, cmn_window {post.cmn_window}, "
          f"min_window {post.min_window}, center {post.center}, norm_vars {post.norm_vars}, refresh {post.refresh}, "
          f"{args.reps} launches per measurement; cumsum within {err:.2e} of the kernel's rows (largest {scale:.1f})")
    print(f"{'form':>7} {'ms/launch':>10} {'GB/s':>8}")
    for name, fn in (("kernel", kernel), ("apply", apply), ("cumsum", cumsum)) * 2:
        for _ in range(10):
            fn()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.reps):
            fn()
        end.record()
        end.synchronize()
        ms = start.elapsed_time(end) / args.reps
        print(f"{name:>7} {ms:>10.4f} {traffic / ms / 1e6:>8.0f}")


if __name__ == "__main__":
    main()
