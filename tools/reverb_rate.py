#!/usr/bin/env python3
"""Reverb (pre.py Reverb: ``pds_reverb_spectra_*``, ``pds_reverb_convolve``, ``pds_reverb_scale``) per call, against
what a user had before it: a torch formulation of the same reverberation.

    python tools/reverb_rate.py [--utts 1024] [--seconds 10] [--rirs 64] [--taps 400,4000,16000] [--reps 10] >> profiles/<tag>.txt

`utts` utterances of `seconds` at 16 kHz, packed on the GPU, against a bank of `rirs` responses of each tap count;
float32 and int16 samples.  Timed with HIP events around `reps` back-to-back calls after 3 untimed ones, the forms in
turn and each twice (the run's own spread):

    spectra       one ``pds_reverb_spectra`` launch into a preallocated workspace
    convolve      one ``pds_reverb_convolve`` launch over that workspace into a preallocated output
    scale         one ``pds_reverb_scale`` launch over the output
    apply_packed  ``Reverb.apply_packed`` with a plan drawn beforehand: one upload, the launches (the two energies and
                  the gain of the fifth library among them) and the allocations, the workspace included
    torch         the formulation a user would otherwise write: ``torch.fft.rfft`` of the batch padded to one length,
                  the product with the gathered response spectra, ``irfft``, the shift by a gather, then the power
                  ratio and the scale

A kernel's rate is given over its own least traffic as a share of 8 TB/s: spectra, the samples read once and 16 bytes a
sample written; convolve, the workspace read once and 4 bytes a sample written (what it re-reads P times is meant to
come from L2); scale, 8 bytes a sample.  Nothing is asserted on the times."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOFLINE = 8e12  # bytes per second
RATE = 16000


def timed(torch, fn, reps, warm=3):
    for _ in range(warm):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def response(L, rng):
    h = 0.3 * rng.standard_normal(L) * np.exp(-6.0 * np.arange(L) / L)
    h[min(L - 1, 40)] = 1.0
    return h.astype(np.float32)


def rates(torch, args, dtype, L):
    from pydrobert_speech_amd import _native
    from pydrobert_speech_amd.pre import Reverb

    B, n, K = args.utts, args.seconds * RATE, args.rirs
    name = {torch.float32: "f32", torch.int16: "i16"}[dtype]
    rng = np.random.default_rng(L)
    rev = Reverb([response(L, rng) for _ in range(K)], seed=1)
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((B * n,), generator=gen, device="cuda") * 3000.0
    if dtype == torch.int16:
        x = x.round().to(torch.int16)
    offs, lens = np.arange(B, dtype=np.int64) * n, np.full(B, n, dtype=np.int64)
    plan = rev.plan(B, seeds=list(range(B)))
    spec_base, spec_total, unit_base, unit_total = rev.layout(lens, plan)
    lib = _native.stages6_lib()
    stream = torch.cuda.current_stream().cuda_stream
    h, bank_table, tw, tap_gains = rev._bank_on(x.device)
    table = torch.as_tensor(np.stack([offs, lens, plan.rir, spec_base, unit_base])).cuda()
    ws = torch.empty((spec_total * 2048,), dtype=torch.float32, device="cuda")
    out = torch.empty((B * n,), dtype=torch.float32, device="cuda")
    gains = torch.full((B,), 0.5, dtype=torch.float64, device="cuda")
    spectra_fn = getattr(lib, "pds_reverb_spectra_" + name)
    xtype = {"f32": 0, "i16": 2}[name]

    def spectra():
        _native.check_stages6(spectra_fn(x.data_ptr(), table[0].data_ptr(), table[1].data_ptr(), table[2].data_ptr(),
                                         table[3].data_ptr(), B, spec_total, tw.data_ptr(), ws.data_ptr(), stream), "spectra")

    def convolve():
        _native.check_stages6(lib.pds_reverb_convolve(
            x.data_ptr(), xtype, table[0].data_ptr(), table[1].data_ptr(), table[2].data_ptr(), table[3].data_ptr(),
            table[4].data_ptr(), B, unit_total, ws.data_ptr(), h.data_ptr(), bank_table[0].data_ptr(),
            bank_table[1].data_ptr(), bank_table[2].data_ptr(), bank_table[3].data_ptr(), tap_gains.data_ptr(), K,
            tw.data_ptr(), out.data_ptr(), stream), "convolve")

    def scale():
        for lo in range(0, B, 65535):
            hi = min(B, lo + 65535)
            _native.check_stages6(lib.pds_reverb_scale(out.data_ptr(), table[0, lo:].data_ptr(), table[1, lo:].data_ptr(),
                                                       gains[lo:].data_ptr(), hi - lo, n, stream), "scale")

    def packed():
        return rev.apply_packed(x, offs, lens, plan=plan)

    # the torch formulation: one padded length for the batch, the response spectra gathered per utterance
    nfft = 1 << int(np.ceil(np.log2(n + L - 1)))
    taps = torch.zeros((K, L), dtype=torch.float32, device="cuda")
    for j, t in enumerate(rev._taps):
        taps[j] = torch.from_numpy(np.asarray(t, dtype=np.float32))
    Hs = torch.fft.rfft(taps, n=nfft)
    j_dev = torch.from_numpy(plan.rir).cuda()
    d_dev = torch.from_numpy(rev.rir_peaks[plan.rir]).cuda()
    steps = torch.arange(n, device="cuda")
    sub = min(B, args.torch_utts)

    def torch_form():
        xs = x.reshape(B, n)[:sub].to(torch.float32)
        full = torch.fft.irfft(torch.fft.rfft(xs, n=nfft) * Hs[j_dev[:sub]], n=nfft)
        wet = torch.gather(full, 1, d_dev[:sub, None] + steps[None, :])
        ps = xs.double().square().mean(dim=1)
        py = wet.double().square().mean(dim=1)
        return wet * torch.sqrt(ps / py).float()[:, None]

    samples = B * n
    in_bytes = x.element_size()
    traffic = {"spectra": samples * (in_bytes + 16), "convolve": samples * (16 + 4), "scale": samples * 8}
    print(f"-- {name} samples, L = {L} taps (P = {-(-L // 512)}), {B} x {args.seconds} s, {K} responses; workspace "
          f"{spec_total * 8192 / 2 ** 30:.2f} GiB, spectra bank {h.numel() * 4 / 2 ** 20:.1f} MiB")
    spectra()
    for label, fn in (("spectra", spectra), ("convolve", convolve), ("scale", scale)):
        ms = [timed(torch, fn, args.reps) for _ in range(2)]
        bw = traffic[label] / (min(ms) * 1e-3)
        print(f"{label:13s} {ms[0]:9.3f} {ms[1]:9.3f} ms   {bw / 1e12:5.2f} TB/s over its own traffic, "
              f"{100 * bw / ROOFLINE:4.1f} % of the roofline")
    ms = [timed(torch, packed, args.reps) for _ in range(2)]
    print(f"{'apply_packed':13s} {ms[0]:9.3f} {ms[1]:9.3f} ms   (with plan=)")
    del ws, out
    torch.cuda.empty_cache()
    mt = [timed(torch, torch_form, max(1, args.reps // 3), warm=1) * (B / sub) for _ in range(2)]
    print(f"{'torch':13s} {mt[0]:9.3f} {mt[1]:9.3f} ms   (rfft of {nfft} points; measured on {sub} utterances, scaled to "
          f"{B}) -- {min(mt) / min(ms):.1f} x apply_packed")
    # one utterance against the float64 convolution, for the record
    got = rev.apply_packed(x[:n].clone(), [0], [n], plan=type(plan)(plan.rir[:1], plan.applied[:1]), return_wet=True)[1]
    want = np.convolve(x[:n].cpu().numpy().astype(np.float64), rev._taps[int(plan.rir[0])])
    d = int(rev.rir_peaks[plan.rir[0]])
    err = np.abs(got.cpu().numpy() - want[d : d + n]).max() / np.abs(want).max()
    print(f"{'check':13s} largest error of the wet signal of utterance 0 against float64: {err:.2e} of its peak")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=1024)
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--rirs", type=int, default=64)
    ap.add_argument("--taps", default="400,4000,16000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-utts", type=int, default=256)
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "needs a HIP device"
    print(f"# tools/reverb_rate.py on {torch.cuda.get_device_name(0)}: ms per call, each form twice")
    for dtype in (torch.float32, torch.int16):
        for L in (int(v) for v in args.taps.split(",")):
            rates(torch, args, dtype, L)


if __name__ == "__main__":
    main()
