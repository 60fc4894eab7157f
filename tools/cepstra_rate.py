#!/usr/bin/env python3
"""The cepstra kernel (``pds_cepstra_rows_f32``, post.py Cepstra) alone, against what a user had before it: a torch
float64 matmul over the same rows.

    python tools/cepstra_rate.py [--rows 1024000] [--filters 40] [--ceps 13] [--reps 50] >> profiles/<tag>.txt

`rows` float32 rows of `filters` log filter-bank outputs on the GPU, `ceps` cepstral coefficients out.  Timed with HIP
events around `reps` back-to-back launches after 10 untimed ones, the forms in turn and each twice (the run's own
spread):

    kernel   one ``pds_cepstra_rows_f32`` launch into a preallocated output
    apply    ``Cepstra.apply(feats)`` as a caller gets it (the launch and the output's allocation)
    matmul   ``(feats.double() @ M.T).float()`` with the same float64 matrix M on the device

The kernel's rows equal numpy's separately rounded float64 sums byte for byte (tests/test_gpu_cepstra.py); the matmul's
agree with them to rounding, which is checked here.  Reports the mean time per launch and the rate over the
algorithmic traffic, rows x (filters + ceps) x 4 bytes; nothing is asserted on the times."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024000)
    ap.add_argument("--filters", type=int, default=40)
    ap.add_argument("--ceps", type=int, default=13)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    import torch

    from pydrobert_speech_amd import _native
    from pydrobert_speech_amd.post import Cepstra

    R, F, K = args.rows, args.filters, args.ceps
    post = Cepstra(K)
    M, copy_cols = post.matrix(F)
    gen = torch.Generator(device="cuda").manual_seed(0)
    feats = 5 * torch.randn((R, F), generator=gen, device="cuda", dtype=torch.float32) - 8
    d_M = torch.from_numpy(M).cuda()
    out = torch.empty((R, K), dtype=torch.float32, device="cuda")
    lib = _native.lib()
    stream = torch.cuda.current_stream().cuda_stream

    def kernel():
        rc = lib.pds_cepstra_rows_f32(feats.data_ptr(), feats.stride(0), R, F, d_M.data_ptr(), K, copy_cols,
                                      out.data_ptr(), out.stride(0), stream)
        _native.check(rc, "pds_cepstra_rows")
        return out

    def apply():
        return post.apply(feats)

    def matmul():
        return (feats.double() @ d_M.T).float()

    want = kernel().clone()
    assert torch.equal(apply(), want)
    err = (matmul() - want).abs().max().item()
    scale = want.abs().max().item()
    assert err <= 4 * np.finfo(np.float32).eps * scale, (err, scale)  # one float32 rounding each, of sums that agree
    traffic = R * (F + K) * 4
    print(f"# {torch.cuda.get_device_name(0)}, {R} x {F} float32 rows -> {K}, {args.reps} launches per measurement; "
          f"matmul within {err:.2e} of the kernel's rows (largest {scale:.1f})")
    print(f"{'form':>7} {'ms/launch':>10} {'GB/s':>8}")
    for name, fn in (("kernel", kernel), ("apply", apply), ("matmul", matmul)) * 2:
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
