#!/usr/bin/env python3
"""SpecAugment (post.py SpecAugment: ``pds_specaug_plan``, ``pds_specaug_mean_rows_f32`` and
``pds_specaug_apply_rows_f32``) per call, against what a user had before it: a torch loop over the utterances.

    python tools/specaug_rate.py [--shapes 1024x1000x80,1x100000x80] [--reps 50] [--torch-reps 3] >> profiles/<tag>.txt

Per shape ``utterances x frames x columns`` of float32 features, packed on the GPU, and per form of the stage (the
defaults: masks only; ``warp=5``; ``fill="mean"``).  Timed with HIP events around `reps` back-to-back calls after 10
untimed ones, the forms in turn and each twice (the run's own spread):

    plan_kernel    one ``pds_specaug_plan`` launch over keys and counts already on the device
    mean_kernel    one ``pds_specaug_mean_rows_f32`` launch (only where the fill is the mean)
    apply_kernel   one ``pds_specaug_apply_rows_f32`` launch over the batch and that plan into a preallocated output
    apply_rows     ``SpecAugment.apply_rows`` as a caller gets it: the upload of offsets, counts and keys, the launches and
                   the allocations of the plan and the output, with one seed per utterance (each seed goes through
                   ``numpy.random.SeedSequence`` on the host, ``Dither``'s rule: measured at 3 us a seed)
    apply_rows_seq the same with ``seeds=None``: the keys are the next of the object's own sequence
    torch          the formulation a user has today: a loop over the utterances that draws widths and starts with
                   ``torch.randint`` from the global generator, assigns slices, and for the warp gathers two rows per
                   frame and interpolates (what ``torch.nn.functional.interpolate`` does along time); `torch-reps`
                   calls after one untimed one

Reports the mean time per call and, for apply_kernel and apply_rows, the rate over the bytes a copy of the batch moves
(every element read once and written once: a masked element is not read, a warped one reads a neighbour that the cache
mostly holds) and that rate's share of 8 TB/s; nothing is asserted on the times.  The kernels' output is checked to be
``apply_rows``'s; the torch form draws other masks and is not compared."""
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


def torch_form(torch, post, x3):
    """what a user writes without the stage: utterance by utterance"""
    B, T, C = x3.shape
    out = x3.clone()
    for b in range(B):
        u = out[b]
        if post.warp and T >= 2 * post.warp + 3:
            W = post.warp
            w0 = int(torch.randint(W + 1, T - 1 - W, ()))
            w1 = w0 - W + int(torch.randint(0, 2 * W + 1, ()))
            t = torch.arange(T, device=u.device, dtype=torch.float64)
            s = torch.where(t <= w1, t * w0 / w1, w0 + (t - w1) * (T - 1 - w0) / (T - 1 - w1))
            i = s.floor().long().clamp_(0, T - 1)
            a = (s - i).unsqueeze(1)
            lo, hi = u[i].double(), u[(i + 1).clamp_(max=T - 1)].double()
            u = out[b] = (lo + a * (hi - lo)).to(u.dtype)
        fill = u.double().mean().to(u.dtype) if post.fill == "mean" else post.fill
        for _ in range(post.freq_masks):
            f = int(torch.randint(0, min(post.freq_width, C) + 1, ()))
            f0 = int(torch.randint(0, C - f + 1, ()))
            u[:, f0:f0 + f] = fill
        for _ in range(post.time_masks):
            n = int(torch.randint(0, min(post.time_width, int(post.time_ratio * T)) + 1, ()))
            t0 = int(torch.randint(0, T - n + 1, ()))
            u[t0:t0 + n] = fill
    return out


def rates(torch, name, post, B, T, C, reps, torch_reps):
    from pydrobert_speech_amd import _native
    from pydrobert_speech_amd.pre import dither_keys

    gen = torch.Generator(device="cuda").manual_seed(0)
    feats = torch.randn((B * T, C), generator=gen, device="cuda")
    rows = np.arange(B + 1, dtype=np.int64) * T
    seeds = list(range(B))
    table = torch.from_numpy(np.stack([rows[:-1], np.diff(rows), dither_keys(seeds).view(np.int64)])).cuda()
    lib = _native.stages3_lib()
    stream = torch.cuda.current_stream().cuda_stream
    d_plan = torch.empty((B, post.plan_words), dtype=torch.int64, device="cuda")
    d_mean = torch.empty((B,), dtype=torch.float64, device="cuda")
    d_out = torch.empty_like(feats)
    use_mean = post.fill == "mean"

    def plan_kernel():
        rc = lib.pds_specaug_plan(table[1].data_ptr(), table[2].data_ptr(), B, C, post.freq_masks, post.freq_width,
                                  post.time_masks, post.time_width, post.time_ratio, post.warp, d_plan.data_ptr(), stream)
        _native.check_stages3(rc, "pds_specaug_plan")

    def mean_kernel():
        rc = lib.pds_specaug_mean_rows_f32(feats.data_ptr(), C, table[0].data_ptr(), table[1].data_ptr(), B, C,
                                           d_mean.data_ptr(), stream)
        _native.check_stages3(rc, "pds_specaug_mean_rows")

    def apply_kernel():
        rc = lib.pds_specaug_apply_rows_f32(feats.data_ptr(), C, table[0].data_ptr(), table[1].data_ptr(), B, C,
                                            d_plan.data_ptr(), post.freq_masks, post.time_masks,
                                            d_mean.data_ptr() if use_mean else None, 0.0 if use_mean else post.fill,
                                            d_out.data_ptr(), C, T, stream)
        _native.check_stages3(rc, "pds_specaug_apply_rows")

    plan_kernel()
    if use_mean:
        mean_kernel()
    apply_kernel()
    want = post.apply_rows(feats, rows, seeds=seeds)
    assert torch.equal(d_out.view(torch.int32), want.view(torch.int32)), "the kernels' rows are not apply_rows's"
    changed = float((want != feats).float().mean())
    x3 = feats.view(B, T, C)
    print(f"# {torch.cuda.get_device_name(0)}, {name}: {B} utterances x {T} frames x {C} float32; {reps} calls per "
          f"measurement ({torch_reps} of the torch form); {100 * changed:.1f} % of the elements changed")
    print(f"{'form':>16} {'ms/call':>12} {'GB/s':>8} {'of 8 TB/s':>10}")
    traffic = 8 * B * T * C
    forms = [("plan_kernel", plan_kernel, 0, reps, 10)]
    if use_mean:
        forms.append(("mean_kernel", mean_kernel, 0, reps, 10))
    forms += [("apply_kernel", apply_kernel, traffic, reps, 10),
              ("apply_rows", lambda: post.apply_rows(feats, rows, seeds=seeds), traffic, reps, 10),
              ("apply_rows_seq", lambda: post.apply_rows(feats, rows), traffic, reps, 10),
              ("torch", lambda: torch_form(torch, post, x3), 0, torch_reps, 1)]
    for form, fn, moved, r, warm in forms * 2:
        ms = timed(torch, fn, r, warm)
        if moved:
            rate = moved / (ms * 1e-3)
            print(f"{form:>16} {ms:>12.4f} {rate / 1e9:>8.0f} {100 * rate / ROOFLINE:>9.2f}%")
        else:
            print(f"{form:>16} {ms:>12.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x1000x80,1x100000x80")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--torch-reps", type=int, default=3)
    args = ap.parse_args()
    import torch

    from pydrobert_speech_amd.post import SpecAugment

    for shape in args.shapes.split(","):
        B, T, C = (int(v) for v in shape.split("x"))
        for name, post in (("masks only", SpecAugment(seed=0)), ("warp=5", SpecAugment(warp=5, seed=0)),
                           ('fill="mean"', SpecAugment(fill="mean", seed=0))):
            rates(torch, name, post, B, T, C, args.reps, args.torch_reps)


if __name__ == "__main__":
    main()
