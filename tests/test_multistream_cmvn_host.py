"""Running / global CMVN of batched streaming on the host, no device (multistream.CmvnState, multistream.streaming_cmvn):
the vectorised restatement of the reference's frame-by-frame ``accumulate(x); apply(x)`` against the reference's own
outputs (tests/golden/make_golden_stream_cmvn.py), the counts, fresh flags and metadata of random tick schedules -- with
pds_multistream_cmvn emulated in numpy from that metadata alone -- and the constructor contract."""
import ctypes
import os

import numpy as np
import pytest

from pydrobert_speech_amd import _native
from pydrobert_speech_amd.multistream import CmvnState, StreamBatch, streaming_cmvn
from pydrobert_speech_amd.multistream_si import SiStreamBatch
from pydrobert_speech_amd.post import CMVN, Deltas, Standardize
from tests.conftest import GOLDEN
from tests.test_multistream_host import build, golden_configs

NAMES = ["c1_kaldi_fbank", "c1_readme_fbank"]
# case of stream_cmvn.npz -> (running, with the prior, norm_var)
CASES = {
    "run_noprior_nv": (True, False, True),
    "run_noprior_nonv": (True, False, False),
    "run_prior_nv": (True, True, True),
    "glob_prior_nv": (False, True, True),
    "glob_prior_nonv": (False, True, False),
}
FLAG_FRESH = 1


def running_cmvn(X, prior=None, norm_var=True, running=True):
    """The reference's ``Standardize`` applied to the rows of `X` in order (post.py:160-173, 214-248), vectorised:
    `running`, ``accumulate(x); apply(x)`` row by row, else ``apply(x)`` with the fixed statistics `prior`
    (``[2, F + 1]``, None: zeros).  Returns ``(Y, stats)``: the float64 rows and the final table.

    ``np.cumsum`` along an axis adds in order, so s1_t = (..((P + x_1) + x_2)..) + x_t as the reference's ``+=``; the
    rest is element-wise and written as the reference writes it.  A NaN row makes every later row of that coefficient
    NaN, as there; what numpy would warn about (0 / 0 of a zero count, the root of a negative variance) is silenced
    here and gives the NaN the arithmetic gives."""
    X = np.asarray(X)
    x = X.astype(np.float64)
    T, F = x.shape
    P = np.zeros((2, F + 1)) if prior is None else np.array(prior, dtype=np.float64)
    assert P.shape == (2, F + 1)
    stats = P.copy()
    if T == 0:
        return x, stats
    if running:
        s1 = np.cumsum(np.concatenate([P[0:1, :F], x]), axis=0)[1:]
        s2 = np.cumsum(np.concatenate([P[1:2, :F], np.square(X, dtype=np.float64)]), axis=0)[1:]
        n = (P[0, F] + np.arange(1, T + 1, dtype=np.float64))[:, None]
        stats[0, :F], stats[1, :F], stats[0, F] = s1[-1], s2[-1], n[-1, 0]
    else:
        s1, s2, n = P[0:1, :F], P[1:2, :F], P[0, F]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = s1 / n
        if norm_var:
            var = s2 / n - mean ** 2
            var = np.where(np.isclose(var, 0), 1.0, var)
            scale = 1 / np.sqrt(var)
        else:
            scale = np.ones_like(mean)
        return x * scale - mean * scale, stats


def fixture():
    with np.load(os.path.join(GOLDEN, "stream_cmvn.npz")) as z:
        return {k: z[k] for k in z.files}


# ---- 1. the restatement against the reference ---------------------------------------------------------------------


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("tag", ["32", "64"])
@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference(name, tag, case):
    g = fixture()
    running, with_prior, norm_var = CASES[case]
    X = g[f"{name}/X{tag}"]
    assert X.dtype == (np.float32 if tag == "32" else np.float64) and 1 < len(X) <= 60
    prior = g[f"{name}/prior{tag}"] if with_prior else None
    Y, stats = running_cmvn(X, prior, norm_var, running)
    want = g[f"{name}/{tag}/{case}/Y"]
    assert Y.dtype == want.dtype == np.float64 and Y.shape == want.shape == X.shape
    assert np.array_equal(Y, want), float(np.abs(Y - want).max())
    assert np.array_equal(stats, g[f"{name}/{tag}/{case}/stats"])
    if not with_prior:
        assert not Y[0].any()  # (a stream's first frame without a prior: a row of zeros)
    if not running:
        from oracle.stft_oracle import cmvn_local

        assert np.array_equal(Y, cmvn_local(X, norm_var=norm_var, stats=prior))


def test_restatement_edge_cases():
    rng = np.random.default_rng(2)
    X = rng.standard_normal((9, 5)).astype(np.float32)
    X[:, 2] = 1.5  # a constant coefficient
    X[4] = X[3]  # a repeated frame
    for norm_var in (True, False):
        Y, stats = running_cmvn(X, None, norm_var)
        assert not Y[0].any() and not Y[:, 2].any() and np.isfinite(Y).all()
        assert stats[0, -1] == 9 and stats[1, -1] == 0
        # cut anywhere, the second part continued from the first part's table: the same rows, the same table
        for cut in (0, 1, 4, 9):
            Ya, sa = running_cmvn(X[:cut], None, norm_var)
            Yb, sb = running_cmvn(X[cut:], sa, norm_var)
            assert np.array_equal(np.concatenate([Ya, Yb]), Y) and np.array_equal(sb, stats)
    X[5, 1] = np.nan
    Y, stats = running_cmvn(X, None, True)
    assert np.isnan(Y[5:, 1]).all() and np.isfinite(Y[:5]).all() and np.isfinite(np.delete(Y, 1, axis=1)).all()
    assert np.isnan(stats[:, 1]).all()


# ---- 2. streaming_cmvn --------------------------------------------------------------------------------------------


def stats_file(tmp_path, table, name="stats.npy"):
    path = os.path.join(str(tmp_path), name)
    np.save(path, table)
    return path


def test_cmvn_settings_are_checked(tmp_path):
    g = fixture()
    comp = build(golden_configs()["c1_kaldi_fbank"])
    F = comp.num_coeffs
    prior = g["c1_kaldi_fbank/prior32"]
    assert prior.shape == (2, F + 1)
    path = stats_file(tmp_path, prior)
    for arg, norm_var in [(Standardize(), True), (CMVN(norm_var=False), False), ("cmvn", True), ("standardize", True),
                          ({"name": "cmvn", "norm_var": False}, False)]:
        for running in (True,):
            inst, table, nv = streaming_cmvn(arg, running, F)
            assert isinstance(inst, Standardize) and table is None and nv is norm_var
    for arg in (Standardize(path), {"name": "cmvn", "rfilename": path}):
        for running in (True, False):
            inst, table, nv = streaming_cmvn(arg, running, F)
            assert isinstance(inst, Standardize) and nv is True
            assert table.dtype == np.float64 and np.array_equal(table, prior) and table is not inst._stats
    assert streaming_cmvn(None, True, F) is None and streaming_cmvn(None, False, F) is None
    wide = stats_file(tmp_path, np.concatenate([prior, prior], axis=1), "wide.npy")
    fractional = prior.copy()
    fractional[0, -1] += 0.5
    empty = Standardize()
    empty._stats = np.zeros((2, F + 1))  # (statistics of no frame are none: Standardize.have_stats)
    assert streaming_cmvn(empty, True, F)[1] is None
    bad = [
        (Deltas(2), True), (3, True), ("deltas", True), ({"name": "stack", "num_vectors": 2}, True),
        ({"norm_var": True}, True), (Standardize(wide), True), (Standardize(wide), False),
        (Standardize(stats_file(tmp_path, fractional, "fractional.npy")), True),
    ]
    for arg, running in bad:
        with pytest.raises(ValueError):
            streaming_cmvn(arg, running, F)
        with pytest.raises(ValueError):  # (before anything touches a device)
            StreamBatch(comp, capacity=4, cmvn=arg, cmvn_running=running)
    for arg in (Standardize(), "cmvn", empty):
        with pytest.raises(ValueError, match="whole utterance"):
            streaming_cmvn(arg, False, F)
        with pytest.raises(ValueError, match="whole utterance"):
            StreamBatch(comp, capacity=4, cmvn=arg, cmvn_running=False)
    with pytest.raises(ValueError):  # statistics of 40 coefficients, a computer of 41
        StreamBatch(build(golden_configs()["c1_readme_fbank"]), capacity=4, cmvn=Standardize(path))
    si = build({"name": "si", "bank": {"name": "gabor", "scaling_function": "mel"}})
    with pytest.raises(ValueError):
        SiStreamBatch(si, capacity=4, cmvn=Deltas(2))
    with pytest.raises(ValueError, match="whole utterance"):
        SiStreamBatch(si, capacity=4, cmvn="cmvn", cmvn_running=False)
    with pytest.raises(ValueError):
        CmvnState(0)
    with pytest.raises(ValueError):
        CmvnState(4, prior_count=-1)
    with pytest.raises(ValueError):
        CmvnState(4, prior_count=0, running=False)


# ---- 3. CmvnState -------------------------------------------------------------------------------------------------


def emulate_tick(pool, prior, cstate, ids, fresh_rows, final, norm_var):
    """pds_multistream_cmvn of one tick in numpy, from the metadata CmvnState.fill_meta writes (include/pds_amd.h):
    `pool` is float64[capacity, 2, F], `prior` the [2, F + 1] table or None, `fresh_rows` the list of the streams' new
    static rows.  Returns each stream's normalised rows and advances `pool` and `cstate`."""
    F = pool.shape[-1]
    ids = np.asarray(ids, dtype=np.int64)
    k = np.asarray([len(x) for x in fresh_rows], dtype=np.int64)
    statics = np.concatenate(fresh_rows) if len(fresh_rows) else np.zeros((0, F))
    static_rows = np.concatenate([[0], np.cumsum(k)])
    step = cstate.step(ids, k, final=final)
    meta = np.full((len(ids), 8), -1, dtype=np.int64)
    cstate.fill_meta(meta, ids, step, static_rows[:-1])
    assert not meta[:, 5:].any()
    for s, flags, row, kk, count in meta[:, :5].tolist():
        assert flags in (0, FLAG_FRESH)
        table = np.zeros((2, F + 1))
        if cstate.running and not flags & FLAG_FRESH:
            table[:, :F] = pool[s]
        elif prior is not None:
            table[:, :F] = prior[:, :F]
        table[0, F] = count
        Y, table = running_cmvn(statics[row : row + kk], table, norm_var, cstate.running)
        statics[row : row + kk] = Y
        if cstate.running and kk:
            pool[s] = table[:, :F]
    cstate.commit(ids, step)
    return [statics[a:b] for a, b in zip(static_rows[:-1], static_rows[1:])]


@pytest.mark.parametrize("running,with_prior", [(True, False), (True, True), (False, True)])
def test_state_over_random_tick_schedules(running, with_prior):
    B, F, norm_var = 16, 5, True
    rng = np.random.default_rng(41 + 2 * running + with_prior)
    prior = None
    if with_prior:
        prior = running_cmvn(rng.standard_normal((7, F)))[1]
    count0 = 7 if with_prior else 0
    cstate = CmvnState(B, count0, running)
    assert cstate.fresh.all()
    pool = rng.standard_normal((B, 2, F))  # (stale sums must never be read)
    rows = [[] for _ in range(B)]  # the current life's statics and outputs
    outs = [[] for _ in range(B)]
    lives = empties = 0
    for _ in range(120):
        ids = np.flatnonzero(rng.random(B) < 0.5)
        rng.shuffle(ids)
        k = rng.integers(0, 6, size=len(ids))
        k[rng.random(len(ids)) < 0.4] = 0
        empties += int((k == 0).sum())
        new = [rng.standard_normal((kk, F)) for kk in k]
        seen = np.asarray([sum(len(r) for r in rows[i]) for i in ids], dtype=np.int64)
        step = cstate.step(ids, k)
        assert (step["fresh"] == (seen == 0)).all()
        assert (step["count"] == count0 + (seen if running else 0)).all()
        assert (cstate.seen[ids] == seen).all()  # (step changes nothing)
        for i, x, y in zip(ids.tolist(), new, emulate_tick(pool, prior, cstate, ids, new, False, norm_var)):
            rows[i].append(x)
            outs[i].append(y)
        assert (cstate.seen[ids] == seen + k).all() and (cstate.fresh[ids] == (seen + k == 0)).all()
        fin = np.flatnonzero(rng.random(B) < 0.1)  # (ids are reused afterwards)
        rng.shuffle(fin)
        last = [rng.standard_normal((int(kk), F)) for kk in rng.integers(0, 3, size=len(fin))]
        for i, x, y in zip(fin.tolist(), last, emulate_tick(pool, prior, cstate, fin, last, True, norm_var)):
            X = np.concatenate(rows[i] + [x])
            got = np.concatenate(outs[i] + [y])
            want, _ = running_cmvn(X, prior, norm_var, running)
            assert np.array_equal(got, want, equal_nan=True), (i, len(X))
            rows[i], outs[i] = [], []
            lives += 1
        assert cstate.fresh[fin].all() and (cstate.counts(fin) == count0).all()
    assert lives > 20 and empties > 50


def test_metadata_words():
    cstate = CmvnState(8, prior_count=3)
    ids = np.asarray([5, 2, 7])
    step = cstate.step(ids, [2, 0, 4])
    cstate.commit(ids, step)
    step = cstate.step(ids, [1, 3, 0])
    meta = np.full((3, 8), 99, dtype=np.int64)
    cstate.fill_meta(meta, ids, step, np.asarray([0, 1, 4]))
    assert meta.tolist() == [[5, 0, 0, 1, 5, 0, 0, 0], [2, FLAG_FRESH, 1, 3, 3, 0, 0, 0], [7, 0, 4, 0, 7, 0, 0, 0]]
    cstate.commit(ids, step)
    assert cstate.seen[[5, 2, 7]].tolist() == [3, 3, 4] and cstate.counts(ids).tolist() == [6, 6, 7]
    cstate.commit(ids[:1], cstate.step(ids[:1], [2], final=True))
    assert cstate.seen[[5, 2, 7]].tolist() == [0, 3, 4] and cstate.fresh[5]
    glob = CmvnState(8, prior_count=3, running=False)
    glob.commit(ids, glob.step(ids, [2, 0, 4]))
    assert glob.step(ids, [1, 1, 1])["count"].tolist() == [3, 3, 3]


# ---- 4. the binding -----------------------------------------------------------------------------------------------


def test_native_table_has_the_entry_points():
    want = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
            ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    for name in ("pds_multistream_cmvn_f32", "pds_multistream_cmvn_f64"):
        restype, argtypes = _native.SIGNATURES[name]
        assert restype is ctypes.c_int32 and argtypes == want
    with open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "pds_amd.h")) as fh:
        header = fh.read()
    assert "int32_t pds_multistream_cmvn_f32(float *d_statics, double *d_pool, int64_t capacity, int32_t coeffs," in header
    assert "int32_t pds_multistream_cmvn_f64(double *d_statics, double *d_pool, int64_t capacity, int32_t coeffs," in header
