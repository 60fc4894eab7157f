#!/usr/bin/env python3
"""Per-tick wall time of batched streaming (multistream.StreamBatch) against a loop of single-stream compute_chunk calls.

    python tools/stream_rate.py [--streams 64,1024,8192] [--ticks 200] [--loop 64,256] [--deltas] [--cmvn]
                                [--stack N] [--dither] [--cepstra N] [--sliding W] [--samples {f32,i16}] [--preemph C]
                                [--si] [--pcen] [--plp]
                                > profiles/<tag>_stream_rate.txt

Configuration c1_readme_fbank of tests/golden/configs.json (16 kHz, 25 ms frames, 10 ms shift), 160-sample (10 ms)
float32 chunks.  Per stream count S: `ticks` timed ticks after 20 untimed ones, each ending in a synchronisation --
compute_chunks (host arrays in, host arrays out) and compute_chunks_packed (samples already on the GPU, features left
there).  Real-time headroom = chunk duration / p50 tick.  The loop: compute_chunk of one chunk on each of S
single-stream computers per tick (the host feed path, as a caller gets it).  --deltas: the same ticks once more
through StreamBatch(deltas=Deltas(2)) (rows "host+d" / "packed+d": statics + delta + delta-delta, three times the
download), and no loop.  --cmvn: the same ticks once more through StreamBatch(cmvn=Standardize()), running mean and
variance normalisation per stream (rows "host+c" / "packed+c": one more launch per tick, the same download), and no
loop.  --stack N: the same ticks once more through StreamBatch(stack=Stack(N)), every N rows of a stream side by side
(rows "host+s" / "packed+s": one more launch per tick, the same download in a third of the rows for N = 3; a tick
returns a row every N-th time per stream, so "frames/tick" counts stacked rows), with --deltas also on top of the deltas
(rows "host+d+s" / "packed+d+s"), and no loop.  --dither: the same ticks once more through
StreamBatch(dither=Dither(1.0, seed=0)), every chunk sample dithered in the assemble launch (rows "host+n" / "packed+n":
no launch more, two more int64 words per stream in the upload, one Philox block, logarithm, square root and sincospi in
float64 per two samples), then the plain ticks a second time (rows "host again" / "packed again": the run's own
run-to-run spread, beside which the difference is reported), and no loop.  --cepstra N: the same ticks once more
through StreamBatch(cepstra=Cepstra(N, energy=<the configuration's include_energy>)), every static row turned into N
cepstral coefficients (rows "host+m" / "packed+m": one more launch per tick, a download of N columns instead of the
computer's), and no loop.  --sliding W: the same ticks once more through
StreamBatch(sliding_cmvn=SlidingCMVN(W, 1)), every static row normalised over the stream's last W + 1 rows (rows
"host+w" / "packed+w": one more launch per tick, the same download; the streams run W + 1 untimed ticks first, so that
the timed ones work on full windows, rebuilt every W frames), and no loop.  --pcen: the computer is built with
use_log=False for the whole run, and the same ticks go once more through StreamBatch(pcen=PCEN()), every static row
normalised by its stream's smoother and compressed (rows "host+e" / "packed+e": one more launch per tick, two words
and a byte more per stream in the upload, the same download), and no loop.  --plp: the computer is built with
use_log=False for the whole run too, and the same ticks go once more through StreamBatch(plp=PLP()), every static row
turned into its 13 PLP cepstra (rows "host+l" / "packed+l": one more launch per tick, no more upload, a download of 13
columns instead of the computer's), and no loop.  --samples i16: the chunks are 16-bit PCM, int16 arrays on the host (two bytes per sample over
the link) and an int16 tensor on the GPU; --preemph C: StreamBatch(preemphasis=C), the pre-emphasis carried across
ticks in the assemble launch.  Either leaves the loop out (a single-stream compute_chunk has no counterpart to them).

--si: the short-integration computer instead (multistream_si.SiStreamBatch, configuration s1_gabor_mel of
tests/golden/si_configs.json: 16 kHz, 10 ms shift), 1024 and 8192 streams by default, against the loop of
ShortIntegrationFrameComputer.compute_chunk calls over the same chunks at 1024 streams (extrapolated to the larger
counts by its cost per call); the ratios are reported, none is asserted.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pct(xs, q):
    return float(np.percentile(np.asarray(xs) * 1e3, q))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default=None, help="default: 64,1024,8192 (--si: 1024,8192)")
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--loop", default=None, help="default: 64,256 (--si: 1024)")
    ap.add_argument("--loop-ticks", type=int, default=20)
    ap.add_argument("--deltas", action="store_true", help="also time the ticks with deltas=Deltas(2); skips the loop")
    ap.add_argument("--cmvn", action="store_true", help="also time the ticks with cmvn=Standardize(); skips the loop")
    ap.add_argument("--stack", type=int, default=0, metavar="N",
                    help="also time the ticks with stack=Stack(N), alone and on top of --deltas; skips the loop")
    ap.add_argument("--dither", action="store_true",
                    help="also time the ticks with dither=Dither(1.0, seed=0), and the plain ticks twice; skips the loop")
    ap.add_argument("--cepstra", type=int, default=0, metavar="N",
                    help="also time the ticks with cepstra=Cepstra(N); skips the loop")
    ap.add_argument("--sliding", type=int, default=0, metavar="W",
                    help="also time the ticks with sliding_cmvn=SlidingCMVN(W, 1); skips the loop")
    ap.add_argument("--pcen", action="store_true",
                    help="linear energies (use_log=False) and also the ticks with pcen=PCEN(); skips the loop")
    ap.add_argument("--plp", action="store_true",
                    help="linear energies (use_log=False) and also the ticks with plp=PLP(); skips the loop")
    ap.add_argument("--samples", choices=("f32", "i16"), default="f32", help="sample type of the chunks")
    ap.add_argument("--preemph", type=float, default=0.0, metavar="C", help="pre-emphasis coefficient (0: none)")
    ap.add_argument("--si", action="store_true", help="short-integration streams (SiStreamBatch, s1_gabor_mel)")
    args = ap.parse_args()
    if args.streams is None:
        args.streams = "1024,8192" if args.si else "64,1024,8192"
    if args.loop is None:
        args.loop = "1024" if args.si else "64,256"
    import torch

    import pydrobert_speech_amd as ps
    from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg
    from pydrobert_speech_amd.multistream import StreamBatch
    from pydrobert_speech_amd.multistream_si import SiStreamBatch
    from pydrobert_speech_amd.post import PCEN, PLP, Cepstra, Deltas, SlidingCMVN, Stack, Standardize
    from pydrobert_speech_amd.pre import Dither

    name = "s1_gabor_mel" if args.si else "c1_readme_fbank"
    Batch = SiStreamBatch if args.si else StreamBatch
    with open(os.path.join(ROOT, "tests", "golden", "si_configs.json" if args.si else "configs.json")) as fh:
        cfg = json.load(fh)["configs"][name]
    if args.pcen or args.plp:
        cfg = dict(cfg, use_log=False)  # (PCEN and PLP take linear energies; the plain ticks of this run do too)

    def computer():
        return alias_factory_subclass_from_arg(ps.compute.FrameComputer, json.loads(json.dumps(cfg)))

    n = 160
    chunk_ms = 1e3 * n / 16000
    rng = np.random.default_rng(0)
    results = {"config": name, "chunk_samples": n, "device": torch.cuda.get_device_name(0)}
    warm = 20
    variant = ""
    extra = {}
    if args.samples != "f32" or args.preemph:
        results.update(samples=args.samples, preemph=args.preemph)
        variant = f", {args.samples} samples" + (f", preemphasis {args.preemph:g}" if args.preemph else "")
        extra = dict(preemphasis=args.preemph)
    print(f"# {results['device']}, {name}, {n}-sample chunks ({chunk_ms:.0f} ms), {args.ticks} ticks{variant}")
    print(f"{'streams':>8} {'api':>12} {'p50 ms':>8} {'p99 ms':>8} {'x real time':>12} {'frames/tick':>11}")
    for S in [int(s) for s in args.streams.split(",")]:
        comp = computer()
        block = (3000 * rng.standard_normal((S, n))).astype(np.float32)
        if args.samples == "i16":
            block = np.rint(block).astype(np.int16)
        chunks = list(block)
        ids = np.arange(S)
        d_block = torch.from_numpy(block.reshape(-1)).cuda()
        lens = np.full(S, n, dtype=np.int64)
        apis = ("host", "packed") + (("host+d", "packed+d") if args.deltas else ())
        apis += ("host+c", "packed+c") if args.cmvn else ()
        if args.stack > 1:
            apis += ("host+s", "packed+s") + (("host+d+s", "packed+d+s") if args.deltas else ())
        if args.dither:
            apis += ("host+n", "packed+n", "host again", "packed again")
        if args.cepstra > 0:
            apis += ("host+m", "packed+m")
        if args.sliding > 0:
            apis += ("host+w", "packed+w")
        if args.pcen:
            apis += ("host+e", "packed+e")
        if args.plp:
            apis += ("host+l", "packed+l")
        for api in apis:
            stages = api.split(" ")[0].split("+")[1:]
            post = dict(deltas=Deltas(2)) if "d" in stages else dict(cmvn=Standardize()) if "c" in stages else {}
            if "s" in stages:
                post["stack"] = Stack(args.stack)
            if "n" in stages:
                post["dither"] = Dither(1.0, seed=0)
            if "m" in stages:
                post["cepstra"] = Cepstra(args.cepstra, energy=bool(getattr(comp, "includes_energy", False)))
            warm = 20
            if "w" in stages:
                post["sliding_cmvn"] = SlidingCMVN(args.sliding, 1)
                warm = max(warm, args.sliding + 1)
            if "e" in stages:
                post["pcen"] = PCEN()
            if "l" in stages:
                post["plp"] = PLP()  # (centre frequencies and the energy column: the computer's)
            sb = Batch(comp, capacity=S, **post, **extra)
            times, frames = [], 0
            for t in range(warm + args.ticks):
                t0 = time.perf_counter()
                if api.startswith("host"):
                    outs = sb.compute_chunks(ids, chunks)
                    rows = sum(len(o) for o in outs)
                else:
                    feats, r = sb.compute_chunks_packed(ids, d_block, lens)
                    torch.cuda.current_stream().synchronize()
                    rows = int(r[-1])
                t1 = time.perf_counter()
                if t >= warm:
                    times.append(t1 - t0)
                    frames += rows
            sb.close()
            p50, p99 = pct(times, 50), pct(times, 99)
            results[f"{api}_{S}"] = dict(p50_ms=p50, p99_ms=p99, realtime_x=chunk_ms / p50, frames_per_tick=frames / args.ticks)
            print(f"{S:>8} {api:>12} {p50:>8.3f} {p99:>8.3f} {chunk_ms / p50:>12.1f} {frames / args.ticks:>11.1f}")
        if args.dither:
            for api in ("host", "packed"):
                a, b, d = (results[f"{k}_{S}"]["p50_ms"] for k in (api, api + " again", api + "+n"))
                print(f"# {S} streams, {api}: dither {d - min(a, b):+.3f} ms on the plain tick "
                      f"({min(a, b):.3f} -> {d:.3f}); the plain tick twice in this run: {a:.3f} / {b:.3f}")
    loops = [int(s) for s in args.loop.split(",") if s.strip() and int(s) > 0]  # (--loop 0: none)
    staged = args.deltas or args.cmvn or args.stack > 1 or args.dither or args.cepstra > 0 or args.sliding > 0 or args.pcen
    staged = staged or args.plp
    for S in [] if staged or variant else loops:
        comps = [computer() for _ in range(S)]
        block = (3000 * rng.standard_normal((S, n))).astype(np.float32)
        times = []
        for t in range(5 + args.loop_ticks):
            t0 = time.perf_counter()
            for c, x in zip(comps, block):
                c.compute_chunk(x)
            t1 = time.perf_counter()
            if t >= 5:
                times.append(t1 - t0)
        p50, p99 = pct(times, 50), pct(times, 99)
        results[f"loop_{S}"] = dict(p50_ms=p50, p99_ms=p99, realtime_x=chunk_ms / p50)
        print(f"{S:>8} {'loop':>12} {p50:>8.3f} {p99:>8.3f} {chunk_ms / p50:>12.1f}")
        if f"host_{S}" in results or S == 256:
            per_stream = p50 / S
            print(f"#   loop: {1e3 * per_stream:.1f} us per compute_chunk call")
            results[f"loop_{S}"]["us_per_call"] = 1e3 * per_stream
    if args.si:
        for L in loops:
            if f"loop_{L}" not in results:
                continue
            per_call = results[f"loop_{L}"]["p50_ms"] / L
            for S in (int(s) for s in args.streams.split(",")):
                if f"host_{S}" in results:
                    loop_S = per_call * S
                    results[f"speedup_{S}_host_vs_loop"] = loop_S / results[f"host_{S}"]["p50_ms"]
                    results[f"speedup_{S}_packed_vs_loop"] = loop_S / results[f"packed_{S}"]["p50_ms"]
                    how = "measured" if S == L else f"extrapolated from {L}"
                    print(f"# {S} streams: loop ({how}, {loop_S:.2f} ms) / tick: host "
                          f"{results[f'speedup_{S}_host_vs_loop']:.1f} x, packed {results[f'speedup_{S}_packed_vs_loop']:.1f} x")
            break
    elif "host_1024" in results and "loop_256" in results:
        loop_1024 = results["loop_256"]["us_per_call"] * 1024 / 1e3
        results["speedup_1024_host_vs_loop"] = loop_1024 / results["host_1024"]["p50_ms"]
        results["speedup_1024_packed_vs_loop"] = loop_1024 / results["packed_1024"]["p50_ms"]
        print(f"# 1024 streams: loop (extrapolated from 256, {loop_1024:.2f} ms) / tick: host "
              f"{results['speedup_1024_host_vs_loop']:.1f} x, packed {results['speedup_1024_packed_vs_loop']:.1f} x")
    print(json.dumps(results))


if __name__ == "__main__":
    main()
