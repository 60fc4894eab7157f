#!/usr/bin/env python3
"""Fixture of the streaming deltas: the reference's Deltas(2) over its own streamed features (authoring container
only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stream_deltas.py <checkout of the reference>

For the eight (length, chunking) cases of stream_random.npz (make_golden_stream.py) of c1_kaldi_fbank and
c2_tri_mel40: the signal is cut as recorded and streamed through the reference's compute_chunk / finalize again (the
features must be the recorded ones), and the reference's ``Deltas(2).apply(feats, axis=0)`` of the concatenated
features goes to stream_deltas.npz as ``<name>/<case>/deltas`` (float32, rows x 3 F).  Data only.
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
    out = {}
    for name in NAMES:
        comp = alias_factory_subclass_from_arg(rcompute.FrameComputer, json.loads(json.dumps(configs[name])))
        for case in range(8):
            n = int(recorded[f"{name}/{case}/n"])
            pieces = np.split(master[50 : 50 + n].astype("f4"), recorded[f"{name}/{case}/cuts"])
            feats = np.concatenate([comp.compute_chunk(p) for p in pieces] + [comp.finalize()])
            assert np.array_equal(feats, recorded[f"{name}/{case}/feats"]), (name, case)
            full = deltas.apply(feats, axis=0) if len(feats) else np.zeros((0, 3 * feats.shape[1]), feats.dtype)
            assert full.dtype == np.float32 and full.shape == (len(feats), 3 * feats.shape[1])
            assert np.array_equal(full[:, : feats.shape[1]], feats)
            out[f"{name}/{case}/deltas"] = full
    path = os.path.join(HERE, "stream_deltas.npz")
    np.savez_compressed(path, **out)
    print("stream_deltas.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
