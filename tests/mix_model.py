"""The definition of ``pre.AddNoise`` in numpy (its class docstring and include/pds_amd_stages5.h have the text): the
Philox block, the plan, the chunked segment energy with its tree, the gain and the mix for every pair of dtypes.  A
helper of the tests, not a test; it is written from the definition, not from the package's code, and shares with the
package only ``pre.dither_keys``, the one rule that turns a seed into a key."""
import math

import numpy as np

CHUNK, LANES = 16384, 64
COUNTER = (0, 0, 0, 0x4D495831)
MASK = (1 << 32) - 1


def philox4x32_10(counter, key):
    """the four output words (Python integers) of one Philox4x32-10 block; `key` is the 64-bit key"""
    c = [int(w) for w in counter]
    k0, k1 = int(key) & MASK, (int(key) >> 32) & MASK
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & MASK, (p0 >> 32) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + 0x9E3779B9) & MASK, (k1 + 0xBB67AE85) & MASK
    return c


def draw(x, K, lengths, lo, hi, prob, clip=None, snr=None):
    """(clip, start, snr, ratio, applied) of the output words `x` of an utterance's block"""
    j = (x[0] * K) >> 32 if clip is None else int(clip)
    s = (x[1] * int(lengths[j])) >> 32
    if snr is None:
        u = np.float64(x[2]) * np.float64(2.0 ** -32)
        snr = np.float64(lo) + (np.float64(hi) - np.float64(lo)) * u
    applied = bool(np.float64(x[3]) * np.float64(2.0 ** -32) < prob)
    return j, s, float(snr), math.pow(10.0, float(snr) / 10.0), applied


def plan(keys, lengths, snr_db, prob, clips=None, snrs=None):
    """the plan of the utterances with `keys` against clips of `lengths`: a dict of numpy arrays"""
    lo, hi = snr_db
    rows = [draw(philox4x32_10(COUNTER, key), len(lengths), lengths, lo, hi, prob,
                 None if clips is None else clips[b], None if snrs is None else snrs[b])
            for b, key in enumerate(keys)]
    cols = list(zip(*rows)) if rows else [[]] * 5
    return {"clip": np.asarray(cols[0], dtype=np.int64), "start": np.asarray(cols[1], dtype=np.int64),
            "snr_db": np.asarray(cols[2], dtype=np.float64), "ratio": np.asarray(cols[3], dtype=np.float64),
            "applied": np.asarray(cols[4], dtype=bool)}


def chunk_sum(x):
    """the sum of one chunk (at most 16384 samples): 64 lane sums in order, then the fixed tree"""
    v = np.asarray(x).astype(np.float64)
    p = np.zeros(LANES, dtype=np.float64)
    with np.errstate(all="ignore"):
        for r in range(0, len(v), LANES):
            row = v[r : r + LANES]
            p[: len(row)] = p[: len(row)] + row * row  # lane l takes sample r + l: product, then sum
        s = LANES // 2
        while s >= 1:
            p[:s] = p[:s] + p[s : 2 * s]
            s //= 2
    return p[0]


def energy(x):
    """E(x, n) as a numpy float64"""
    e = np.float64(0.0)
    with np.errstate(all="ignore"):
        for c in range(0, len(x), CHUNK):
            e = e + chunk_sum(x[c : c + CHUNK])
    return e


def energy_rows(X):
    """E of every row of the 2-D array `X` (utterances of one length), the same sums taken for all rows at once"""
    V = np.asarray(X).astype(np.float64)
    e = np.zeros(V.shape[0], dtype=np.float64)
    with np.errstate(all="ignore"):
        for c in range(0, V.shape[1], CHUNK):
            chunk = V[:, c : c + CHUNK]
            p = np.zeros((V.shape[0], LANES), dtype=np.float64)
            for r in range(0, chunk.shape[1], LANES):
                row = chunk[:, r : r + LANES]
                p[:, : row.shape[1]] = p[:, : row.shape[1]] + row * row
            s = LANES // 2
            while s >= 1:
                p[:, :s] = p[:, :s] + p[:, s : 2 * s]
                s //= 2
            e = e + p[:, 0]
    return e


def power(x):
    return energy(x) / np.float64(len(x)) if len(x) else np.float64(0.0)


def gain(ps, pn, ratio, applied):
    if not (applied and ps > 0.0 and pn > 0.0):  # (false for NaN)
        return np.float64(0.0)
    with np.errstate(all="ignore"):
        return np.sqrt(np.float64(ps) / (np.float64(pn) * np.float64(ratio)))


def out_dtype(x_dtype):
    return np.float64 if np.dtype(x_dtype) == np.float64 else np.float32


def mix(x, clip, start, g):
    """y of one utterance `x` with gain `g` against `clip` read from `start`"""
    T = out_dtype(x.dtype)
    if g == 0.0:
        return x.copy() if x.dtype == T else x.astype(T)
    idx = (int(start) + np.arange(len(x), dtype=np.int64)) % len(clip)
    with np.errstate(all="ignore"):
        prod = np.float64(g) * clip[idx].astype(np.float64)
        return (x.astype(np.float64) + prod).astype(T)


def apply_packed(signal, offsets, lengths, clips, the_plan, gains=None):
    """(out, gains): the packed result in numpy.  `clips`: the list of clips; `gains`: taken as given where not None
    (the device's own).  Float samples outside the utterances keep their values; for int16 they are zero here"""
    T = out_dtype(signal.dtype)
    out = signal.copy() if signal.dtype == T else np.zeros(len(signal), dtype=T)
    pn = [power(c) for c in clips]
    used = np.zeros(len(lengths), dtype=np.float64)
    for b, (o, n) in enumerate(zip(offsets, lengths)):
        x = signal[o : o + n]
        j = int(the_plan["clip"][b])
        g = gain(power(x), pn[j], the_plan["ratio"][b], bool(the_plan["applied"][b])) if gains is None else gains[b]
        used[b] = g
        out[o : o + n] = mix(x, clips[j], the_plan["start"][b], g)
    return out, used
