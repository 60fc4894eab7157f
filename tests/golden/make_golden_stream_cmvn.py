#!/usr/bin/env python3
"""Fixture of the streaming CMVN: the reference's Standardize applied frame by frame to its own features (authoring
container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stream_cmvn.py <checkout of the reference>

For c1_kaldi_fbank (40 coefficients) and c1_readme_fbank (41, the first the energy) of configs.json, two
configurations of stream.npz: the reference's ``compute_full`` of a stretch of the master signal of signals.npz, as
float32 and as float64 samples.  The first ROWS rows are the statics ``X``; the PRIOR_ROWS rows behind them go through
``Standardize().accumulate`` and leave the ``prior`` table.  Then, per sample type and case,

    running:  for every row in order  ``cmvn.accumulate(x); y = cmvn.apply(x)``   (and the final ``cmvn._stats``)
    global:   for every row           ``y = cmvn.apply(x)``                       (``cmvn._stats`` the prior)

with the cases ``run_noprior_nv``, ``run_noprior_nonv``, ``run_prior_nv``, ``glob_prior_nv``, ``glob_prior_nonv``
(``nv``: norm_var=True).  Goes to stream_cmvn.npz as ``<name>/X32``, ``<name>/X64``, ``<name>/prior32``,
``<name>/prior64``, ``<name>/<32|64>/<case>/Y`` and ``.../stats``.  Data only.
"""
import json
import os
import sys
import warnings

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["c1_kaldi_fbank", "c1_readme_fbank"]
ROWS, PRIOR_ROWS = 16, 10
# case -> (running, with the prior, norm_var)
CASES = {
    "run_noprior_nv": (True, False, True),
    "run_noprior_nonv": (True, False, False),
    "run_prior_nv": (True, True, True),
    "glob_prior_nv": (False, True, True),
    "glob_prior_nonv": (False, True, False),
}


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
    out = {}
    for name in NAMES:
        comp = alias_factory_subclass_from_arg(rcompute.FrameComputer, json.loads(json.dumps(configs[name])))
        n = (ROWS + PRIOR_ROWS + 2) * comp.frame_shift + comp.frame_length
        for tag, dtype in (("32", np.float32), ("64", np.float64)):
            feats = comp.compute_full(master[300 : 300 + n].astype(dtype))
            assert feats.dtype == dtype and len(feats) >= ROWS + PRIOR_ROWS, (feats.dtype, feats.shape)
            X, other = feats[:ROWS], feats[ROWS : ROWS + PRIOR_ROWS]
            acc = rpost.Standardize()
            acc.accumulate(other)
            prior = acc._stats.copy()
            assert prior.shape == (2, X.shape[1] + 1) and prior[0, -1] == PRIOR_ROWS
            out[f"{name}/X{tag}"] = X
            out[f"{name}/prior{tag}"] = prior
            for case, (running, with_prior, norm_var) in CASES.items():
                cmvn = rpost.Standardize(norm_var=norm_var)
                if with_prior:
                    cmvn._stats = prior.copy()
                Y = np.empty(X.shape, dtype=np.float64)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")  # ("0 variance encountered": a stream's first frame)
                    for t in range(ROWS):
                        if running:
                            cmvn.accumulate(X[t])
                        Y[t] = cmvn.apply(X[t])
                assert Y.dtype == np.float64 and np.isfinite(Y).all()
                out[f"{name}/{tag}/{case}/Y"] = Y
                out[f"{name}/{tag}/{case}/stats"] = cmvn._stats.copy()
    path = os.path.join(HERE, "stream_cmvn.npz")
    np.savez_compressed(path, **out)
    print("stream_cmvn.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
