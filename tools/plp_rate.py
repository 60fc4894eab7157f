#!/usr/bin/env python3
"""PLP (post.py PLP: ``pds_plp_rows_f32``) per call, against what a user had before it: a torch formulation of the
same definition.

    python tools/plp_rate.py [--shapes 1024x1000x23,1024x1000x40] [--reps 50] [--torch-reps 5] >> profiles/<tag>.txt

Per shape ``utterances x frames x filters`` of float32 linear energies, packed on the GPU, the default ``PLP`` (13
cepstra of order 12) with centre frequencies spread over 8 kHz.  Timed with HIP events around `reps` back-to-back
calls after 10 untimed ones, the forms in turn and each twice (the run's own spread):

    kernel        one ``pds_plp_rows_f32`` launch into a preallocated output (no synchronisation)
    apply_rows    ``PLP.apply_rows`` as a caller gets it: the launch and the allocation of the output
    with_aux      the same with the auxiliary output (d and E of every row, float64) into a preallocated buffer
    torch         the formulation a user has today: float64 ``torch.pow``, one matmul for r, a Python loop over the p
                  Durbin steps with the rows side by side, the cepstrum loop; `torch-reps` calls after one untimed one

Reports the mean time per call, rows per second and the rate over the bytes the call must move (the rows in, the
cepstra out; with_aux: 8 (F + 3) bytes a row more) as a share of 8 TB/s; nothing is asserted on the times.  The torch
form is another order of additions in r (a matmul): it is checked against the kernel within the float32 tolerance.

Then, for float32 and float64 rows, the largest share of the standing tolerance (``1e-5 + 1e-4 |ref|``, ``1e-9 + 1e-9
|ref|``) that any element of the device's output uses against the numpy model of the definition (tests/plp_model.py)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOFLINE = 8e12  # bytes per second


def centers(F):
    return [60.0 + 7900.0 * (f + 0.5) / F for f in range(F)]


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


def rates(torch, B, T, F, reps, torch_reps):
    from pydrobert_speech_amd import _native
    from pydrobert_speech_amd.post import PLP

    post = PLP(centers_hz=centers(F))
    p, K, D = post.lpc_order, post.num_ceps, F + 2
    gen = torch.Generator(device="cuda").manual_seed(0)
    R = B * T
    feats = torch.exp(torch.randn((R, F), generator=gen, device="cuda") * 2.0).float()
    feats[torch.rand((R, F), generator=gen, device="cuda") < 0.02] = 0.0
    lib = _native.stages4_lib()
    stream = torch.cuda.current_stream().cuda_stream
    d_w, d_B, d_L = post._tables_on(F, feats.device)
    d_out = torch.empty((R, K), dtype=torch.float32, device="cuda")
    d_aux = torch.empty((R, D + 1), dtype=torch.float64, device="cuda")

    def kernel():
        rc = lib.pds_plp_rows_f32(feats.data_ptr(), F, R, F, 0, d_w.data_ptr(), d_B.data_ptr(), d_L.data_ptr(), p, K,
                                  post.compress_factor, post.floor, d_out.data_ptr(), K, None, stream)
        _native.check_stages4(rc, "pds_plp_rows")
        return d_out

    def torch_form():
        e = feats.double()
        h = torch.pow(torch.clamp_min(e, post.floor) * d_w, post.compress_factor)
        d = torch.cat([h[:, :1], h, h[:, -1:]], dim=1)
        r = d @ d_B.T  # (R, p + 1)
        a = torch.zeros((R, p), dtype=torch.float64, device=e.device)
        E = r[:, 0].clone()
        for i in range(p):
            k = r[:, i + 1].clone()
            if i:
                k = k + (a[:, :i] * r[:, 1: i + 1].flip(1)).sum(1)
            k = k / E
            E = E * torch.clamp_min(1.0 - k * k, 1e-5)
            if i:
                a[:, :i] = a[:, :i] - k[:, None] * a[:, :i].flip(1)
            a[:, i] = -k
        q = torch.zeros((R, p), dtype=torch.float64, device=e.device)
        for i in range(p):
            s = 0.0
            if i:
                n = torch.arange(i, 0, -1, dtype=torch.float64, device=e.device)
                s = (n * a[:, :i] * q[:, :i].flip(1)).sum(1)
            q[:, i] = -a[:, i] - s / (i + 1)
        out = torch.cat([torch.log(E)[:, None], q[:, : K - 1]], dim=1) * d_L
        return out.float()

    want = post.apply_rows(feats)
    assert torch.equal(kernel(), want)
    assert torch.equal(post.apply_rows(feats, aux=d_aux), want)
    ty = torch_form()
    assert torch.allclose(ty, want, rtol=1e-4, atol=1e-5), float((ty - want).abs().max())
    del ty
    print(f"# {torch.cuda.get_device_name(0)}, {B} utterances x {T} frames x {F} float32, p = {p}, K = {K}; {reps} calls "
          f"per measurement ({torch_reps} of the torch form)")
    print(f"{'form':>12} {'ms/call':>10} {'M rows/s':>10} {'GB/s':>8} {'of 8 TB/s':>10}")
    moved = R * 4 * (F + K)
    forms = (("kernel", kernel, moved, reps, 10), ("apply_rows", lambda: post.apply_rows(feats), moved, reps, 10),
             ("with_aux", lambda: post.apply_rows(feats, aux=d_aux), moved + R * 8 * (D + 1), reps, 10),
             ("torch", torch_form, moved, torch_reps, 1))
    for name, fn, traffic, r, warm in forms * 2:
        ms = timed(torch, fn, r, warm)
        rate = traffic / (ms * 1e-3)
        print(f"{name:>12} {ms:>10.4f} {R / ms / 1e3:>10.1f} {rate / 1e9:>8.0f} {100 * rate / ROOFLINE:>9.2f}%")


def distances(torch):
    from pydrobert_speech_amd.post import PLP
    from tests.plp_model import energies, plp_model, tolerance_ratio

    rng = np.random.default_rng(0)
    for dtype, atol, rtol in ((np.float32, 1e-5, 1e-4), (np.float64, 1e-9, 1e-9)):
        share, count = 0.0, 0
        for F in (23, 40):
            post = PLP(centers_hz=centers(F))
            for _ in range(4):
                x = energies(rng, (2000, F), dtype)
                ref = plp_model(post, x)
                got = post.apply(x)
                assert np.isfinite(got).all() and np.isfinite(ref).all()
                share = max(share, tolerance_ratio(got, ref))
                count += ref.size
        print(f"# the output against the numpy model, {np.dtype(dtype).name} rows, {count} elements: at most "
              f"{100 * share:.2g} % of the tolerance {atol:g} + {rtol:g} |ref| used")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x1000x23,1024x1000x40")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--torch-reps", type=int, default=5)
    args = ap.parse_args()
    import torch

    for shape in args.shapes.split(","):
        B, T, F = (int(v) for v in shape.split("x"))
        rates(torch, B, T, F, args.reps, args.torch_reps)
    distances(torch)


if __name__ == "__main__":
    main()
