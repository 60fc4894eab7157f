"""A plain numpy restatement of the energy VAD as ``post.EnergyVAD`` and ``include/pds_amd_stages.h`` define it (test
infrastructure, CPU only): float64, the 64 interleaved partial sums by explicit ordered accumulation, every operation
rounded separately."""
import numpy as np

PARTIALS = 64


def energy_sum(e):
    """the sum of the float64 energies `e` as the definition orders it: 64 partial sums over ``t = j (mod 64)`` in
    ascending t, each from +0.0, then added in j order from +0.0.  `e` is ``(T,)``, or ``(T, N)`` for N utterances of
    one length side by side (the result is ``(N,)`` then)"""
    e = np.asarray(e, dtype=np.float64)
    partial = np.zeros((PARTIALS,) + e.shape[1:], dtype=np.float64)
    with np.errstate(all="ignore"):  # (NaN and infinite energies are part of the contract; the suite raises on warnings)
        for t in range(len(e)):
            partial[t % PARTIALS] = partial[t % PARTIALS] + e[t]
        s = np.zeros(e.shape[1:], dtype=np.float64)
        for j in range(PARTIALS):
            s = s + partial[j]
    return s


def threshold(e, energy_threshold=5.0, energy_mean_scale=0.5):
    """the float64 threshold of an utterance with the energies `e` (``len(e) >= 1``)"""
    if energy_mean_scale == 0:
        return np.float64(energy_threshold)
    with np.errstate(all="ignore"):
        scaled = np.float64(energy_mean_scale) * energy_sum(e)
        mean = scaled / np.float64(len(e))
        return np.float64(energy_threshold) + mean


def vad_decide(e, energy_threshold=5.0, energy_mean_scale=0.5, frames_context=0, proportion_threshold=0.6):
    """bool ``(T,)``: which frames of one utterance with the energies `e` (any float dtype, widened first) are voiced"""
    e = np.asarray(e).astype(np.float64)
    assert e.ndim == 1
    T = len(e)
    if T == 0:
        return np.zeros(0, dtype=bool)
    thr = threshold(e, energy_threshold, energy_mean_scale)
    with np.errstate(all="ignore"):
        above = e > thr  # (False for a NaN on either side)
    before = np.concatenate([[0], np.cumsum(above, dtype=np.int64)])  # (integers: exact in any order)
    voiced = np.zeros(T, dtype=bool)
    for t in range(T):
        lo, hi = max(0, t - frames_context), min(T - 1, t + frames_context)
        den, num = hi - lo + 1, int(before[hi + 1] - before[lo])
        voiced[t] = float(num) >= float(den) * float(proportion_threshold)
    return voiced


def vad_decide_rows(feats, row_offsets, energy_col=0, **kwargs):
    """``(voiced, counts)`` of a packed ragged batch: uint8 ``(R,)`` (0 in rows of no utterance), int64 ``(B,)``"""
    feats = np.asarray(feats)
    voiced = np.zeros(len(feats), dtype=np.uint8)
    counts = np.zeros(len(row_offsets) - 1, dtype=np.int64)
    for b in range(len(counts)):
        a, z = int(row_offsets[b]), int(row_offsets[b + 1])
        v = vad_decide(feats[a:z, energy_col], **kwargs)
        voiced[a:z] = v
        counts[b] = int(v.sum())
    return voiced, counts


def select_rows(feats, row_offsets, keep):
    """``(out, out_row_offsets)``: the rows of every utterance whose `keep` is not 0, in order"""
    feats, keep = np.asarray(feats), np.asarray(keep)
    pieces = [feats[int(a) : int(z)][keep[int(a) : int(z)] != 0] for a, z in zip(row_offsets[:-1], row_offsets[1:])]
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.int64)
    out = np.concatenate(pieces) if pieces else feats[:0]
    return np.ascontiguousarray(out), offsets
