"""A plain numpy restatement of sliding-window CMVN as ``post.SlidingCMVN`` and ``include/pds_amd_stages.h`` define it
(test infrastructure, CPU only): frame by frame, float64, every operation rounded separately."""
import numpy as np


def window(t, T, W, min_window, center):
    """``(ws, we)`` of frame `t` of an utterance of `T` frames"""
    if center:
        ws = t - W // 2
        we = ws + W
    else:
        ws = t - W
        we = t + 1
    if ws < 0:
        we -= ws
        ws = 0
    if not center and we > t:
        we = max(t + 1, min_window)
    if we > T:
        ws -= we - T
        we = T
        ws = max(ws, 0)
    return ws, we


def sliding_cmvn(x, cmn_window=600, min_window=100, center=False, norm_vars=False, refresh=None):
    """``(y, s1, s2)`` for the ``(T, C)`` float32 or float64 matrix `x` of one utterance: the normalised rows in x's
    dtype and the float64 ``(T, C)`` sums every frame was normalised with"""
    x = np.asarray(x)
    assert x.ndim == 2 and x.dtype in (np.float32, np.float64)
    refresh = cmn_window if refresh is None else refresh
    T, C = x.shape
    xd = x.astype(np.float64)
    y = np.zeros((T, C), dtype=np.float64)
    S1 = np.zeros((T, C), dtype=np.float64)
    S2 = np.zeros((T, C), dtype=np.float64)
    s1 = np.zeros(C, dtype=np.float64)
    s2 = np.zeros(C, dtype=np.float64)
    ws = we = 0
    with np.errstate(all="ignore"):  # (NaN and infinite frames are part of the contract; the suite raises on warnings)
        for t in range(T):
            nws, nwe = window(t, T, cmn_window, min_window, center)
            if t % refresh == 0:
                s1 = np.zeros(C, dtype=np.float64)
                s2 = np.zeros(C, dtype=np.float64)
                for u in range(nws, nwe):
                    s1 = s1 + xd[u]
                    s2 = s2 + xd[u] * xd[u]
            else:
                assert nws - ws in (0, 1) and nwe - we in (0, 1)
                if nws != ws:
                    s1 = s1 - xd[ws]
                    s2 = s2 - xd[ws] * xd[ws]
                if nwe != we:
                    s1 = s1 + xd[nwe - 1]
                    s2 = s2 + xd[nwe - 1] * xd[nwe - 1]
            ws, we = nws, nwe
            n = float(we - ws)
            mean = s1 / n
            row = xd[t] - mean
            if norm_vars:
                if we - ws == 1:
                    row = np.zeros(C, dtype=np.float64)
                else:
                    var = s2 / n - mean * mean
                    var = np.where(var > 1e-10, var, 1e-10)
                    row = row * (1.0 / np.sqrt(var))
            y[t], S1[t], S2[t] = row, s1, s2
        return y.astype(x.dtype), S1, S2


def same_bits(a, b):
    """equal shape and dtype, NaNs at the same positions and every other element equal bit for bit"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not (na == nb).all():
        return False
    ints = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool((a.view(ints)[~na] == b.view(ints)[~na]).all())
