#!/usr/bin/env python3
"""Fixture of the streaming frame stacking: the reference's Stack over its own streamed features (authoring container
only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stream_stack.py <checkout of the reference>

For the eight (length, chunking) cases of stream_random.npz (make_golden_stream.py) of c1_kaldi_fbank and
c2_tri_mel40: the signal is cut as recorded and streamed through the reference's compute_chunk / finalize again (the
features must be the recorded ones), and of the concatenated features `feats` the reference's

    <name>/<case>/deltas_stack3      Stack(3).apply(Deltas(2).apply(feats, axis=0))            rows // 3 x 9 F
    <name>/<case>/stack4_edge        Stack(4, pad_mode="edge").apply(feats)                     ceil(rows / 4) x 4 F
    <name>/<case>/stack2_constant    Stack(2, pad_mode="constant", constant_values=-1.0).apply(feats)

go to stream_stack.npz (float32).  Data only.
"""
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["c1_kaldi_fbank", "c2_tri_mel40"]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, os.path.join(sys.argv[1], "src"))
    from pydrobert.speech import compute as rcompute
    from pydrobert.speech import post as rpost
    from pydrobert.speech.alias import alias_factory_subclass_from_arg

    with open(os.path.join(HERE, "configs.json")) as fh:
        configs = json.load(fh)["configs"]
    master = np.load(os.path.join(HERE, "signals.npz"))["master"]
    with np.load(os.path.join(HERE, "stream_random.npz")) as z:
        recorded = {k: z[k] for k in z.files}
    deltas = rpost.Deltas(2)
    stacks = {
        "deltas_stack3": lambda feats: rpost.Stack(3).apply(deltas.apply(feats, axis=0)),
        "stack4_edge": rpost.Stack(4, pad_mode="edge").apply,
        "stack2_constant": rpost.Stack(2, pad_mode="constant", constant_values=-1.0).apply,
    }
    widths = {"deltas_stack3": (3, 3, False), "stack4_edge": (4, 1, True), "stack2_constant": (2, 1, True)}
    out = {}
    for name in NAMES:
        comp = alias_factory_subclass_from_arg(rcompute.FrameComputer, json.loads(json.dumps(configs[name])))
        for case in range(8):
            n = int(recorded[f"{name}/{case}/n"])
            pieces = np.split(master[50 : 50 + n].astype("f4"), recorded[f"{name}/{case}/cuts"])
            feats = np.concatenate([comp.compute_chunk(p) for p in pieces] + [comp.finalize()])
            assert np.array_equal(feats, recorded[f"{name}/{case}/feats"]), (name, case)
            T, F = feats.shape
            for tag, apply in stacks.items():
                nv, mult, pad = widths[tag]
                groups = -(-T // nv) if pad else T // nv
                full = apply(feats) if T else np.zeros((0, nv * mult * F), feats.dtype)
                assert full.dtype == np.float32 and full.shape == (groups, nv * mult * F), (name, case, tag, full.shape)
                out[f"{name}/{case}/{tag}"] = np.ascontiguousarray(full)
    path = os.path.join(HERE, "stream_stack.npz")
    np.savez_compressed(path, **out)
    print("stream_stack.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
