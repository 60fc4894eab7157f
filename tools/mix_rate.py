#!/usr/bin/env python3
"""AddNoise (pre.py AddNoise: ``pds_mix_chunk_energy_*``, ``pds_mix_gain``, ``pds_mix_apply_*``) per call, against what
a user had before it: a torch formulation of the same mixing.

    python tools/mix_rate.py [--utts 1024] [--seconds 10] [--clips 64] [--clip-seconds 30] [--reps 50] >> profiles/<tag>.txt

`utts` utterances of `seconds` at 16 kHz, packed on the GPU, against a bank of `clips` clips of `clip-seconds`; float32
on float32 and int16 on int16.  Timed with HIP events around `reps` back-to-back calls after 5 untimed ones, the forms
in turn and each twice (the run's own spread):

    energy        one ``pds_mix_chunk_energy`` launch over the utterances into a preallocated buffer
    gain          one ``pds_mix_gain`` launch (mode 2) over their chunk sums
    apply         one ``pds_mix_apply`` launch into a preallocated output
    apply_packed  ``AddNoise.apply_packed`` as a caller gets it: the plan on the host (one key per seed, as
                  ``Dither.apply_packed`` forms them), one upload, three launches and the allocations
    with plan=    the same with a plan drawn beforehand: no keys, no draws
    dither        ``Dither.apply_packed`` on the same buffer: the nearest existing kernel of the same shape
    torch loop    the formulation a user has today, utterance by utterance: an index tensor ``(s + arange(n)) % L``, a
                  gather, two float64 sums of squares, a scale and an add (on the first `torch-utts` utterances)
    torch batch   the same as one batched gather over all utterances

The apply kernel's rate is given over the 12 bytes a sample it must move (int16 on int16: 8) as a share of 8 TB/s.
Then the bank's one-time ``clip_power``, and ``clip_power`` of one ten-minute clip, which is what the chunking is for,
beside an estimate of the single wave it replaces.  Then the device against the numpy model of the definition
(tests/mix_model.py): elements compared, and those not bit-equal.  Nothing is asserted on the times."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOFLINE = 8e12  # bytes per second
RATE = 16000


def timed(torch, fn, reps, warm=5):
    for _ in range(warm):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def rates(torch, args, dtype):
    from pydrobert_speech_amd import _native
    from pydrobert_speech_amd.pre import AddNoise, Dither

    B, n, K, L = args.utts, args.seconds * RATE, args.clips, args.clip_seconds * RATE
    gen = torch.Generator(device="cuda").manual_seed(0)
    name = {torch.float32: "f32", torch.int16: "i16"}[dtype]

    def make(count, scale):
        x = torch.randn((count,), generator=gen, device="cuda") * scale
        return x.round().to(torch.int16) if dtype == torch.int16 else x

    bank = make(K * L, 500.0)
    an = AddNoise([c.cpu().numpy() for c in bank.reshape(K, L)], snr_db=(5.0, 20.0), seed=1)
    del bank
    x = make(B * n, 3000.0)
    offs, lens = np.arange(B, dtype=np.int64) * n, np.full(B, n, dtype=np.int64)
    lib = _native.stages5_lib()
    stream = torch.cuda.current_stream().cuda_stream
    d_bank, _, _ = an._bank_on(x.device)
    pn = an.clip_power(x.device)
    plan = an.plan(B, seeds=range(B))
    bases, total = an._chunk_bases(lens)
    table = torch.as_tensor(np.stack([offs, lens, bases, an.clip_offsets[plan.clip], an.clip_lengths[plan.clip], plan.start,
                                      plan.ratio.view(np.int64), plan.applied.astype(np.int64), plan.clip])).cuda()
    partials = torch.empty((total,), dtype=torch.float64, device="cuda")
    gains = torch.empty((B,), dtype=torch.float64, device="cuda")
    out = torch.empty((B * n,), dtype=torch.float32, device="cuda")
    energy_fn = getattr(lib, "pds_mix_chunk_energy_" + name)
    apply_fn = getattr(lib, f"pds_mix_apply_{name}_{name}")

    def energy():
        _native.check_stages5(energy_fn(x.data_ptr(), table[0].data_ptr(), table[1].data_ptr(), table[2].data_ptr(), B,
                                        total, partials.data_ptr(), stream), "energy")

    def gain():
        _native.check_stages5(lib.pds_mix_gain(partials.data_ptr(), table[2].data_ptr(), table[1].data_ptr(), B, 2,
                                               table[8].data_ptr(), table[6].data_ptr(), table[7].data_ptr(),
                                               pn.data_ptr(), K, gains.data_ptr(), stream), "gain")

    def apply():
        for lo in range(0, B, 65535):
            hi = min(B, lo + 65535)
            _native.check_stages5(apply_fn(x.data_ptr(), table[0, lo:].data_ptr(), table[1, lo:].data_ptr(),
                                           d_bank.data_ptr(), table[3, lo:].data_ptr(), table[4, lo:].data_ptr(),
                                           table[5, lo:].data_ptr(), gains[lo:].data_ptr(), hi - lo, n, out.data_ptr(),
                                           stream), "apply")

    seeds = list(range(B))
    dither = Dither(1.0)
    starts = torch.as_tensor(plan.start).cuda()
    clip_off = torch.as_tensor(an.clip_offsets[plan.clip]).cuda()
    clip_len = torch.as_tensor(an.clip_lengths[plan.clip]).cuda()
    ratio = torch.as_tensor(plan.ratio).cuda()
    steps = torch.arange(n, device="cuda")

    def torch_one(b):
        seg = x[b * n : (b + 1) * n].double()
        idx = clip_off[b] + (starts[b] + steps) % clip_len[b]
        z = d_bank[idx].double()
        whole = d_bank[clip_off[b] : clip_off[b] + clip_len[b]].double()
        g = torch.sqrt((seg * seg).sum() / n / ((whole * whole).sum() / clip_len[b] * ratio[b]))
        return (seg + g * z).float()

    def torch_loop():
        return [torch_one(b) for b in range(args.torch_utts)]

    def torch_batch():
        X = x.reshape(B, n).double()
        idx = clip_off[:, None] + (starts[:, None] + steps[None, :]) % clip_len[:, None]
        Z = d_bank[idx].double()
        ps = (X * X).sum(1) / n
        g = torch.sqrt(ps / (pn[torch.as_tensor(plan.clip).cuda()] * ratio))
        return (X + g[:, None] * Z).float()

    energy(), gain(), apply()
    want = an.apply_packed(x, offs, lens, plan=plan)
    assert torch.equal(out, want)
    ref = torch_one(3)
    got = want[3 * n : 4 * n]
    assert torch.allclose(got, ref, rtol=1e-5, atol=1e-2), float((got - ref).abs().max())
    del ref, got, want
    print(f"# {torch.cuda.get_device_name(0)}, {B} utterances x {n} samples {name} on a bank of {K} x {L} {name}; "
          f"{args.reps} calls per measurement ({args.torch_reps} of the torch forms, the loop over {args.torch_utts} utterances)")
    print(f"{'form':>14} {'ms/call':>10} {'G samples/s':>12} {'GB/s':>8} {'of 8 TB/s':>10}")
    width = 2 if dtype == torch.int16 else 4
    moved = B * n * (width + width + 4)
    forms = [("energy", energy, B * n * width, B * n, args.reps), ("gain", gain, total * 8, B * n, args.reps),
             ("apply", apply, moved, B * n, args.reps),
             ("apply_packed", lambda: an.apply_packed(x, offs, lens, seeds=seeds), moved + B * n * width, B * n, args.reps),
             ("with plan=", lambda: an.apply_packed(x, offs, lens, plan=plan), moved + B * n * width, B * n, args.reps),
             ("dither", lambda: dither.apply_packed(x, offs, lens, seeds=seeds), B * n * (width + 4), B * n, args.reps),
             ("torch loop", torch_loop, args.torch_utts * n * (width + width + 4), args.torch_utts * n, args.torch_reps)]
    if args.torch_batch:
        forms.append(("torch batch", torch_batch, moved, B * n, args.torch_reps))
    for label, fn, traffic, count, reps in forms * 2:
        ms = timed(torch, fn, reps, warm=1 if label.startswith("torch") else 5)
        rate = traffic / (ms * 1e-3)
        print(f"{label:>14} {ms:>10.4f} {count / ms / 1e6:>12.2f} {rate / 1e9:>8.0f} {100 * rate / ROOFLINE:>9.2f}%")
    # the bank's one-time clip powers (upload excluded: the bank is on the device)
    for _ in range(2):
        an._on_device[x.device.index][2] = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        an.clip_power(x.device)
        torch.cuda.synchronize()
        print(f"# clip_power of the bank ({K} x {L} {name}), two launches, wall clock: {1e3 * (time.perf_counter() - t0):.3f} ms")


def long_clip(torch, dtype_name):
    from pydrobert_speech_amd.pre import AddNoise

    n = 600 * RATE
    rng = np.random.default_rng(1)
    clip = (rng.standard_normal(n) * 500).astype(np.float32)
    if dtype_name == "i16":
        clip = np.rint(clip).astype(np.int16)
    an = AddNoise([clip])
    an._bank_on(None)
    times = []
    for _ in range(5):
        an._on_device[torch.cuda.current_device()][2] = None
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        an.clip_power()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    chunks = -(-n // 16384)
    # one wave alone: a lane's n / 64 float64 adds depend on one another; at about 8 cycles an add (the VALU's float64
    # issue rate on a quarter-rate path and the dependence) and 2.4 GHz that is n / 64 * 8 / 2.4e9 seconds -- an
    # estimate from the per-lane add chain, not a measurement
    estimate = n / 64 * 8 / 2.4e9 * 1e3
    print(f"# clip_power of one ten-minute clip ({n} samples {dtype_name}, {chunks} chunks = waves): "
          f"{min(times):.4f}-{max(times):.4f} ms over 5 calls; a single wave is estimated at {estimate:.2f} ms "
          f"(per-lane chain of {n // 64} dependent float64 adds; an estimate)")


def against_model(torch):
    from pydrobert_speech_amd.pre import AddNoise, dither_keys
    from tests import mix_model as mm

    rng = np.random.default_rng(2)
    for xt, zt in ((np.float32, np.float32), (np.int16, np.int16), (np.float64, np.float32), (np.float32, np.int16)):
        def make(count, scale, t):
            v = rng.standard_normal(count) * scale
            return np.rint(v).astype(np.int16) if t == np.int16 else v.astype(t)

        lengths = [int(v) for v in rng.integers(1, 40000, 48)]
        clip_lengths = [1, 50, 4000, 16385, 70000]
        clips = [make(L, 500.0, zt) for L in clip_lengths]
        an = AddNoise(clips, snr_db=(0.0, 20.0), prob=0.9)
        offs = np.cumsum([0] + lengths[:-1])
        x = make(sum(lengths), 3000.0, xt)
        seeds = list(range(len(lengths)))
        out, gains = an.apply_packed(torch.from_numpy(x).cuda(), offs, lengths, seeds=seeds, return_gains=True)
        plan = mm.plan(dither_keys(seeds), clip_lengths, (0.0, 20.0), 0.9)
        want, want_g = mm.apply_packed(x, offs, lengths, clips, plan)
        got, g = out.cpu().numpy(), gains.cpu().numpy()
        e = an.energy_packed(torch.from_numpy(x).cuda(), offs, lengths).cpu().numpy()
        want_e = np.asarray([mm.energy(x[o : o + n]) for o, n in zip(offs, lengths)])
        word = np.uint64 if got.dtype == np.float64 else np.uint32
        print(f"# device against the numpy model, {np.dtype(xt).name} on {np.dtype(zt).name}: {got.size} samples compared, "
              f"{int((got.view(word) != want.view(word)).sum())} not bit-equal; {len(g)} gains, "
              f"{int((g.view(np.uint64) != want_g.view(np.uint64)).sum())} not bit-equal; {len(e)} energies, "
              f"{int((e.view(np.uint64) != want_e.view(np.uint64)).sum())} not bit-equal")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=1024)
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--clip-seconds", type=int, default=30)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--torch-utts", type=int, default=64)
    ap.add_argument("--no-torch-batch", dest="torch_batch", action="store_false")
    args = ap.parse_args()
    import torch

    for dtype in (torch.float32, torch.int16):
        rates(torch, args, dtype)
        torch.cuda.empty_cache()
    for name in ("f32", "i16"):
        long_clip(torch, name)
    against_model(torch)


if __name__ == "__main__":
    main()
