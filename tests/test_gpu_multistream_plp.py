"""The PLP stage of batched streaming on the GPU (``StreamBatch(plp=...)``, ``SiStreamBatch(plp=...)``).

Five streams over seeded random cuts with empty chunks among them and ``finalize`` ticks of their own, float32 and
float64; two streams run a second utterance on their ids.  A stream's rows, concatenated over its ticks and its
``finalize``, are ``PLP.apply`` of its whole statics -- the rows of a batch built without any post stage and given the
same chunks -- bit for bit, whatever the cuts; with `cmvn`, ``Deltas(2)`` and ``Stack(3)`` behind the stage they are
the offline chain's.  The object's centre frequencies and energy column come from the batch's computer.  `plp` together
with `cepstra` or `pcen`, a computer that takes logs and a width the object refuses are ``ValueError`` s."""
import numpy as np
import pytest

from pydrobert_speech_amd.multistream import StreamBatch
from pydrobert_speech_amd.multistream_si import SiStreamBatch
from pydrobert_speech_amd.post import PCEN, PLP, Cepstra, Deltas, Stack, Standardize
from tests.plp_model import plp_model, same_bits, within_tolerance
from tests.test_gpu_multistream import build
from tests.test_gpu_multistream_pcen import CAPACITY, IDS, SI_CONFIG, computer, drive, statics
from tests.test_multistream_cmvn_host import running_cmvn
from tests.test_multistream_host import golden_configs

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


@pytest.mark.parametrize("spec", [PLP(), {"name": "plp", "num_ceps": 9, "lpc_order": 10, "compress_factor": 0.5,
                                          "lifter": 0, "scale": 0.1}], ids=["default", "config"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_are_the_offline_rows(dtype, spec):
    comp = computer("stft")
    post = PLP.for_computer(comp, **({} if isinstance(spec, PLP) else {k: v for k, v in spec.items() if k != "name"}))
    with StreamBatch(comp, capacity=CAPACITY, dtype=dtype, plp=spec) as sb:
        assert list(sb._stages) == ["plp"]
        assert sb.num_coeffs == post.num_ceps and sb.lookahead == 0 and sb.num_vectors == 1
        got, brought = drive(sb, dtype)
    assert 0 in brought and max(brought) >= 2  # empty ticks and ticks of several rows
    ref = statics("stft", dtype)
    assert got.keys() == ref.keys() and len(ref) == 7
    for key, x in ref.items():
        want = post.apply(x)
        assert want.dtype == dtype and want.shape == (len(x), post.num_ceps)
        assert same_bits(got[key], want), key  # whatever the cuts
        assert within_tolerance(want, plp_model(post, x)), key  # ... and they are the model's


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_whole_chain_is_the_offline_chain(dtype):
    comp = computer("stft")
    post, deltas, stack = PLP.for_computer(comp), Deltas(2), Stack(3)
    with StreamBatch(comp, capacity=CAPACITY, dtype=dtype, plp="plp", cmvn=Standardize(), deltas=Deltas(2),
                     stack=Stack(3)) as sb:
        assert list(sb._stages) == ["plp", "cmvn", "deltas", "stack"]
        assert sb.num_coeffs == 3 * 3 * 13 and sb.lookahead == 4 and sb.num_vectors == 3
        got, _ = drive(sb, dtype)
    for key, x in statics("stft", dtype).items():
        normed = running_cmvn(post.apply(x))[0].astype(dtype)  # Standardize frame by frame
        want = stack.apply(deltas.apply(normed, axis=0))
        assert want.shape == (len(x) // 3, 117)
        assert same_bits(got[key], want), key


@pytest.mark.parametrize("dtype", DTYPES)
def test_short_integration_streams(dtype):
    comp = computer("si")
    post = PLP.for_computer(comp, num_ceps=7)
    with SiStreamBatch(comp, capacity=CAPACITY, dtype=dtype, plp=PLP(num_ceps=7)) as sb:
        assert sb.num_coeffs == 7
        got, _ = drive(sb, dtype)
    rows = 0
    for key, x in statics("si", dtype).items():
        assert same_bits(got[key], post.apply(x)), key
        rows += len(x)
    assert rows > 60
    with SiStreamBatch(comp, capacity=CAPACITY, dtype=dtype, plp=PLP(num_ceps=7), cmvn=Standardize(), deltas=Deltas(2),
                       stack=Stack(3)) as sb:
        assert sb.num_coeffs == 3 * 3 * 7
        got, _ = drive(sb, dtype)
    for key, x in statics("si", dtype).items():
        normed = running_cmvn(post.apply(x))[0].astype(dtype)
        assert same_bits(got[key], Stack(3).apply(Deltas(2).apply(normed, axis=0))), key


def test_the_energy_column_is_the_computers():
    dtype = np.float32
    comp = build(dict(golden_configs()["c1_kaldi_fbank"], use_log=False, include_energy=True))
    assert comp.num_coeffs == 41 and comp.includes_energy
    x = np.clip(np.rint(3000 * np.random.default_rng(5).standard_normal(4000)), -32768, 32767).astype(dtype)
    with StreamBatch(comp, capacity=4, dtype=dtype, plp="plp") as sb, StreamBatch(comp, capacity=4, dtype=dtype) as plain:
        assert sb._stages["plp"].spec.energy is True and sb.num_coeffs == 13
        got = [sb.compute_chunks([2], [x[:1500]])[0], sb.compute_chunks([2], [x[1500:1500]])[0],
               sb.compute_chunks([2], [x[1500:]])[0], sb.finalize([2])[0]]
        ref = [plain.compute_chunks([2], [x[:1500]])[0], plain.compute_chunks([2], [x[1500:]])[0], plain.finalize([2])[0]]
    ref = np.concatenate(ref)
    post = PLP.for_computer(comp)
    want = post.apply(ref)
    assert len(got[1]) == 0 and same_bits(np.concatenate(got), want)
    floor = np.float64(post.floor)
    assert within_tolerance(want[:, 0], np.log(np.maximum(ref[:, 0].astype(np.float64), floor)).astype(dtype))


def test_the_three_value_errors():
    linear, logged = computer("stft"), build(golden_configs()["c1_kaldi_fbank"])
    for other in (dict(cepstra=Cepstra(13)), dict(pcen=PCEN()), dict(cepstra="mfcc", pcen="pcen")):
        with pytest.raises(ValueError, match="without cepstra and pcen"):
            StreamBatch(linear, capacity=CAPACITY, plp=PLP(), **other)
        with pytest.raises(ValueError, match="without cepstra and pcen"):
            SiStreamBatch(computer("si"), capacity=CAPACITY, plp="plp", **other)
    with pytest.raises(ValueError, match="PLP takes linear energies"):
        StreamBatch(logged, capacity=CAPACITY, plp=PLP())
    with pytest.raises(ValueError, match="PLP takes linear energies"):
        SiStreamBatch(build(dict(SI_CONFIG, use_log=True)), capacity=CAPACITY, plp="plp")
    # a width the object refuses: centres of another bank, more LPC coefficients than the bank supports
    with pytest.raises(ValueError, match="centre frequencies"):
        StreamBatch(linear, capacity=CAPACITY, plp=PLP(centers_hz=[100.0, 200.0, 300.0]))
    narrow = build({"name": "si", "bank": {"name": "fbank", "num_filts": 8}, "use_log": False})
    with pytest.raises(ValueError, match="lpc_order"):
        SiStreamBatch(narrow, capacity=CAPACITY, plp=PLP())
