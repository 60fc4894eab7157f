#!/usr/bin/env python3
"""PCEN (post.py PCEN: ``pds_pcen_smooth_rows_f32`` and ``pds_pcen_compress_rows_f32``) per call, against what a user
had before it: a torch formulation of the same definition.

    python tools/pcen_rate.py [--shapes 1024x1000x40,1x100000x40] [--reps 50] [--torch-reps 3] >> profiles/<tag>.txt

Per shape ``utterances x frames x columns`` of float32 linear energies, packed on the GPU.  Timed with HIP events around
`reps` back-to-back calls after 10 untimed ones, the forms in turn and each twice (the run's own spread):

    smooth_kernel    one ``pds_pcen_smooth_rows_f32`` launch into a preallocated float64 M (no synchronisation)
    compress_kernel  one ``pds_pcen_compress_rows_f32`` launch over the batch and that M into a preallocated output
    apply_rows       ``PCEN.apply_rows`` as a caller gets it: both launches and the allocations of M and the output
    torch            the formulation a user has today: M by a float64 loop over the frames (two multiplications and an
                     addition of ``(utterances, columns)`` tensors per frame), the rest with ``torch.pow`` over the
                     batch; `torch-reps` calls after one untimed one, because a loop over 100,000 frames takes seconds

Reports the mean time per call, the rate over the traffic the call must move (smooth: the rows in, 8 bytes of M out;
compress: the rows and M in, the rows out; apply_rows: both) and that rate's share of 8 TB/s; nothing is asserted on the
times.  torch's M is the same arithmetic and is checked to be the kernel's bit for bit; its y goes through torch's pow.

Then, for float32 and float64 rows of a smaller batch, the largest distance of the device's y from the numpy model of
the definition (tests/pcen_model.py), in units of the last place of the row type at the magnitude of the root
``y + bp`` (the subtraction of ``bp`` cancels where E is small, so the last place of y itself would say nothing about
``pow`` there), and the largest share of the standing
tolerance (``1e-5 + 1e-4 |ref|``, ``1e-9 + 1e-9 |ref|``) any element uses."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOFLINE = 8e12  # bytes per second


def timed(torch, fn, reps, warm):
    for _ in range(warm):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def rates(torch, post, B, T, C, reps, torch_reps):
    from pydrobert_speech_amd import _native
    from pydrobert_speech_amd.post import _rows_meta

    gen = torch.Generator(device="cuda").manual_seed(0)
    feats = torch.exp(torch.randn((B * T, C), generator=gen, device="cuda") * 4.6).float()
    feats[torch.rand((B * T, C), generator=gen, device="cuda") < 0.05] = 0.0
    rows = np.arange(B + 1, dtype=np.int64) * T
    meta, _ = _rows_meta(rows, feats.device)
    lib = _native.stages2_lib()
    stream = torch.cuda.current_stream().cuda_stream
    d_m = torch.empty((B * T, C), dtype=torch.float64, device="cuda")
    d_out = torch.empty_like(feats)

    def smooth_kernel():
        rc = lib.pds_pcen_smooth_rows_f32(feats.data_ptr(), C, meta[0].data_ptr(), meta[1].data_ptr(), B, C,
                                          post.smooth_coeff, post.oms, d_m.data_ptr(), C, stream)
        _native.check_stages2(rc, "pds_pcen_smooth_rows")
        return d_m

    def compress_kernel():
        rc = lib.pds_pcen_compress_rows_f32(feats.data_ptr(), C, d_m.data_ptr(), C, B * T, C, post.gain, post.bias,
                                            post.power, post.eps, post.bp, d_out.data_ptr(), C, stream)
        _native.check_stages2(rc, "pds_pcen_compress_rows")
        return d_out

    x3 = feats.view(B, T, C)

    def torch_form():
        x = x3.double()
        m = torch.empty_like(x)
        prev = m[:, 0] = x[:, 0]
        for t in range(1, T):
            prev = m[:, t] = post.oms * prev + post.smooth_coeff * x[:, t]
        y = torch.pow(x / torch.pow(post.eps + m, post.gain) + post.bias, post.power) - post.bp
        return y.float(), m

    n = B * T * C
    smooth_kernel()
    want = post.apply_rows(feats, rows)
    assert torch.equal(compress_kernel(), want)
    ty, tm = torch_form()
    assert torch.equal(tm.view(-1, C), d_m), "torch's M is not the kernel's"
    assert torch.allclose(ty.view(-1, C), want, rtol=1e-4, atol=1e-5)
    del ty, tm
    print(f"# {torch.cuda.get_device_name(0)}, {B} utterances x {T} frames x {C} float32; {reps} calls per measurement "
          f"({torch_reps} of the torch form)")
    print(f"{'form':>16} {'ms/call':>12} {'GB/s':>8} {'of 8 TB/s':>10}")
    forms = (("smooth_kernel", smooth_kernel, 12 * n, reps, 10), ("compress_kernel", compress_kernel, 16 * n, reps, 10),
             ("apply_rows", lambda: post.apply_rows(feats, rows), 28 * n, reps, 10),
             ("torch", torch_form, 28 * n, torch_reps, 1))
    for name, fn, traffic, r, warm in forms * 2:
        ms = timed(torch, fn, r, warm)
        rate = traffic / (ms * 1e-3)
        print(f"{name:>16} {ms:>12.4f} {rate / 1e9:>8.0f} {100 * rate / ROOFLINE:>9.2f}%")


def distances(torch, post):
    from tests.pcen_model import energies, pcen_model

    rng = np.random.default_rng(0)
    for dtype, atol, rtol in ((np.float32, 1e-5, 1e-4), (np.float64, 1e-9, 1e-9)):
        worst = share = 0.0
        count = 0
        for _ in range(16):
            E = energies(rng, (500, 40), dtype)
            ref, _ = pcen_model(post, E)
            got = post.apply(E, axis=0)
            assert (np.isfinite(got) == np.isfinite(ref)).all()
            err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
            # the last place of the root, |ref| + bp: y is that root minus bp, and where the two cancel (E = 0 gives
            # y = 0) the last place of y itself says nothing about pow
            ulp = np.spacing((np.abs(ref.astype(np.float64)) + post.bp).astype(dtype)).astype(np.float64)
            worst = max(worst, float((err / ulp).max()))
            share = max(share, float((err / (atol + rtol * np.abs(ref.astype(np.float64)))).max()))
            count += E.size
        print(f"# y against the numpy model, {np.dtype(dtype).name} rows, {count} elements: at most {worst:.2f} units of "
              f"the last place of y + bp apart; at most {100 * share:.2g} % of the tolerance {atol:g} + {rtol:g} |ref| used")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x1000x40,1x100000x40")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--torch-reps", type=int, default=3)
    args = ap.parse_args()
    import torch

    from pydrobert_speech_amd.post import PCEN

    post = PCEN()
    for shape in args.shapes.split(","):
        B, T, C = (int(v) for v in shape.split("x"))
        rates(torch, post, B, T, C, args.reps, args.torch_reps)
    distances(torch, post)


if __name__ == "__main__":
    main()
