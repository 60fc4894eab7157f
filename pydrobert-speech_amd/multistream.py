"""Batched streaming: ``compute_chunk`` / ``finalize`` of many streams per launch

:func:`ShortTimeFourierTransformFrameComputer.compute_chunk` serves one stream per call: one host concatenation, one
launch and one synchronisation for what is, for a 10 ms chunk, one frame.  :class:`StreamBatch` keeps the carried
samples of up to `capacity` streams in a device pool and takes every stream that has new audio in one *tick*:

    sb = StreamBatch(computer, capacity=4096)        # computer: an STFT frame computer
    outs = sb.compute_chunks(ids, chunks)             # ids: distinct ints; chunks: 1-D arrays -> list of (k_i, C)
    outs = sb.finalize(ids)                           # the last frames; the streams are reset and may be reused
    feats, rows = sb.compute_chunks_packed(ids, d_samples, lengths)   # GPU in, GPU out
    sb.close()

    sb = StreamBatch(computer, capacity=4096, deltas=Deltas(2))   # statics + delta + delta-delta, see below
    sb = StreamBatch(computer, capacity=4096, preemphasis=0.97)   # Preemphasize(0.97) over every stream's whole signal
    sb = StreamBatch(computer, capacity=4096, cmvn=Standardize())  # running CMVN per stream, see below
    sb = StreamBatch(computer, capacity=4096, stack=Stack(3))      # every 3 rows of a stream side by side, see below
    sb = StreamBatch(computer, capacity=4096, dither=Dither(1.0, seed=5))   # Dither over every stream's whole signal
    sb = StreamBatch(computer, capacity=4096, cepstra=Cepstra(13))  # cepstral coefficients of every row, see below
    sb = StreamBatch(computer, capacity=4096, sliding_cmvn=SlidingCMVN(600, 1))  # sliding-window CMVN, see below
    sb = StreamBatch(computer, capacity=4096, pcen=PCEN())         # per-channel energy normalisation, see below
    sb = StreamBatch(computer, capacity=4096, plp=PLP())           # PLP cepstra of every row, see below

Every stream gets, call by call, what a private copy of `computer` returns from ``compute_chunk`` / ``finalize`` for
the same chunks: the same row counts, dtype and -- for float32 and float64 samples -- the same values bit for bit as
the computer's plain path (``config.HOST_FEED = False``).  Which streams a tick names, and in which order, changes no
stream's result.  Chunks of 16-bit PCM (int16) give the values of the same chunks converted to `dtype` first; a tick
whose chunks are all int16 sends them to the GPU as they are, two bytes per sample, and converts them there.

A tick: the per-stream integer state (:class:`StreamState`: carry length, carry pad, pending skip, first-frame and
started flags) is advanced on the host with numpy, which fixes every output size without reading the device; samples
and metadata go up in one copy from pinned memory; ``pds_multistream_assemble_*`` (``csrc/multistream.hip``) writes
the tick's packed work buffer (carry + chunk of every stream) and the new carries in one launch; the STFT batch
kernels run over the work buffer with explicit per-stream frame counts, one launch per distinct carry pad (the left
reflection is launch-wide; in steady state every stream has pad 0); features come down in one copy.  ``finalize``
reads the carries where they lie in the pool.

Both kinds of tick, of this class and of :class:`multistream_si.SiStreamBatch`, are one pipeline,
:func:`_TickBatch._tick`: the streams' spans (where each one's samples lie in what the feature launch reads), the
upload -- laid out by :func:`_tick_layout` and addressed by section name through :class:`_Upload`, nowhere by hand --,
the assemble launch (``compute_chunks`` only), the feature launch, the commit or reset of the host state, then the
post stages.  A class adds what differs through four hooks: its host state, the order in which the emitting streams
launch, its extra rows of launch metadata, and the feature launch itself.

The post stages -- pcen, cepstra or plp, cmvn or sliding-window cmvn, deltas, stack, in that order -- are objects of one protocol,
:class:`_Stage`, which the constructor lists and the tick loops over twice.  A stage owns its parsed spec, its host
state (``DeltaState`` ...; none for cepstra), its device pools, its typed entry point -- looked up when the stage is
built, so a library without it is an ``AttributeError`` for the batch that asks for the stage and no other -- and the
names of its upload sections; it tells its output width from its input width.  ``plan`` is the host half, before the
upload: given every stream's first row in what enters the stage, it steps its state without changing it, fills its
sections and returns every stream's first row in what leaves it.  ``launch`` is the device half, after the feature
launch: its one launch and check, then the commit of its state.  ``release`` drops its pools.  A new stage is such a
class, its place in the constructor's list and -- if it has metadata -- its sections in :func:`_tick_layout`; the
dither and the pre-emphasis act inside the assemble launch and are no stages.

With `deltas` (a :class:`post.Deltas`: "edge" padding, concatenated along the coefficient axis) a stream's rows are
those of ``deltas.apply(X, axis=0)`` over the whole sequence X of its statics, bit for bit, delayed by the look-ahead
``H = num_deltas * context_window`` frames a delta row needs of the future: a ``compute_chunks`` call returns the rows
whose future has arrived, ``finalize`` the last ones with the right edge replicated.  :class:`DeltaState` counts
frames and rows per stream on the host; the device keeps every stream's last ``2 H`` static rows in a second
ping-pong pool, and one launch per tick (``pds_multistream_deltas_*``) reads "history, then the tick's new statics",
writes the rows due and the next history.  ``2 H`` rows suffice: after a tick the rows not yet returned are the last
H frames, the first of them reaches H further back, and while a stream has seen at most ``2 H`` frames its frame 0 is
still in the history, so the left edge replication never needs a row that is gone.

With `preemphasis` (a coefficient or a :class:`pre.Preemphasize`) a stream's rows are those of the same calls over
``Preemphasize(coeff).apply(x)`` of its whole raw signal x, cut where the chunks were cut, bit for bit: the assemble
launch pre-emphasises every chunk sample as it enters the work buffer, against the sample before it in the chunk or,
for a chunk's first sample, the stream's last raw sample, which a third ping-pong pool of one sample per stream keeps
across ticks (:attr:`StreamState.has_sample` says whether there is one).  A stream's first sample after its start or
``finalize`` passes unchanged.  The carries hold pre-emphasised samples, so ``finalize`` needs nothing more.

With `dither` (a :class:`pre.Dither`) a stream's rows are those of the same calls over ``Dither(coeff,
seed=s).apply(x)`` of its whole raw signal x converted to `dtype`, cut where the chunks were cut, bit for bit -- in
front of the pre-emphasis, if there is one, as in the reference's chain.  The generator is counter-based: the noise of
sample t depends on the utterance's key and t alone, so the assemble launch (``pds_multistream_assemble_dither``)
dithers every chunk sample as it enters the work buffer, given where the chunk starts in the stream's raw signal.
:class:`DitherState` keeps, per stream, the raw samples received this utterance (dropped ones too) and the utterance's
seed and key, and numbers the utterances the batch begins, from 0: streams begin in tick order and within a tick in the
order of `ids`, and the n-th utterance has seed ``dither_base + n`` (:attr:`StreamBatch.dither_base`: the ``Dither``'s
seed, or a 63-bit value drawn at construction).  ``finalize`` ends the utterance; the stream's next chunk begins a new
one with the next seed at position 0.  :func:`StreamBatch.dither_seeds` names the seeds of the current utterances.  The
carries and the previous-sample pool hold dithered samples, so ``finalize`` needs nothing more.

With `cepstra` (a :class:`post.Cepstra`) every static row becomes its `num_ceps` cepstral coefficients -- the first
post stage of a tick: one ``pds_cepstra_rows`` launch over the tick's static rows straight after the feature launch
(none in a tick without rows), before `cmvn`, `deltas` and `stack`, which all see rows of the cepstral width.  A row
depends on nothing but itself, so the stage has no state, no pool and no metadata, and the upload is laid out as without
it.  A stream's rows are those of the offline chain over its whole utterance, ``stack(deltas(cmvn(cepstra(statics))))``
with whichever stages are present, bit for bit.

With `cmvn` (a :class:`post.Standardize`) every static row is standardised as it is produced, in one of the two forms
of the reference's ``Standardize`` that do not need the whole utterance.  Per stream, with x_1, x_2, .. its static rows
since its start or last ``finalize`` and P the ``[2, F + 1]`` statistics of the ``Standardize`` passed in (sums | count,
sums of squares; zeros without any), in float64 and every operation rounded separately:

    s1_0 = P[0, :F];  s2_0 = P[1, :F];  n_0 = P[0, F]
    running (``cmvn_running=True``):  s1_t = s1_{t-1} + x_t;  s2_t = s2_{t-1} + x_t * x_t;  n_t = n_{t-1} + 1
    global (``cmvn_running=False``):  s1, s2 and n stay P's
    mean = s1_t / n_t;  var = s2_t / n_t - mean * mean
    norm_var:  var = 1 where |var| <= 1e-8;  scale = 1 / sqrt(var)        (else scale = 1)
    y_t = x_t * scale - mean * scale

-- the reference's ``cmvn.accumulate(x_t); cmvn.apply(x_t)`` frame by frame (running: cumulative mean and variance
normalisation, optionally seeded with prior statistics) or ``cmvn.apply(x_t)`` with fixed statistics (global), bit for
bit; y_t is rounded to `dtype` once.  As there, a stream's first frame without a prior comes out as zeros (its
variance is 0 and replaced by 1), a constant coefficient gives zeros, and a NaN static stays in its stream's sums until
the ``finalize``; the reference's "0 variance" warning is not raised.  ``Standardize`` without statistics over a whole
utterance cannot be streamed: ``cmvn_running=False`` without statistics is refused.  :class:`CmvnState` counts the
frames per stream on the host; the device keeps every stream's running sums in a pool of ``2 * capacity * F`` float64,
and one launch per tick (``pds_multistream_cmvn_*``), after the feature launches and before the deltas, adds the
tick's rows to the sums and normalises them in place.  ``finalize`` normalises the last frames like any others and
returns the stream to P.  With `deltas` the deltas are taken of the normalised statics (Kaldi's ``apply-cmvn |
add-deltas``), so the history pool holds normalised rows and a stream's rows are ``deltas.apply(Y, axis=0)``.
:func:`StreamBatch.cmvn_stats` returns the streams' current tables.

With `sliding_cmvn` (a :class:`post.SlidingCMVN` with ``center=False`` and ``min_window=1``) every static row is
normalised by the mean (and variance) of the stream's last ``W + 1 = cmn_window + 1`` static rows, itself included --
the stage runs where `cmvn` runs, after `cepstra` and before `deltas` and `stack`, and the two exclude each other.  A
stream's rows are ``sliding_cmvn.apply(X)`` of the whole sequence X of its statics since its start or last
``finalize``, bit for bit, whatever the cuts: the sums are rebuilt every `refresh` frames of the stream, as offline,
so rounding does not drift however long the stream runs, and a NaN or infinite row stops affecting the stream at the
first refresh after it has left the window.  A centred window needs ``W // 2`` frames of the future and
``min_window > 1`` makes the first rows wait for later ones: both are refused.  :class:`SlidingState` counts the frames
per stream on the host; the device keeps, per stream, a ring of its last ``W + 1`` static rows in `dtype` -- frame t in
slot ``t % (W + 1)``, so the slot a frame overwrites holds exactly the frame that leaves the window -- and its two sums
in float64, and one launch per tick (``pds_multistream_sliding_*`` of the stages library, ``csrc/sliding.hip``) takes
every stream's new rows in order, in place.  ``finalize`` normalises the last rows like any others and returns the
stream to fresh.

With `pcen` (a :class:`post.PCEN`, over a computer that does not take logs) every static row is normalised per column
by the stream's one-pole smoother and root-compressed -- the first post stage of a tick, before `cepstra`, `cmvn` /
`sliding_cmvn`, `deltas` and `stack`, which see its rows; widths and the look-ahead do not change.  A stream's rows are
those of the offline chain ``stack(deltas(cmvn(cepstra(pcen.apply(statics)))))`` over its whole utterance, bit for bit,
whatever the cuts: the smoother is a recurrence of one float64 per column, which a pool of ``capacity * F`` float64
keeps across ticks exactly, and the compression is the one function the offline kernels inline
(``csrc/pcen_rule.h``).  :class:`PcenState` knows per stream whether it is fresh -- its next row is the first of its
utterance, where ``M = E``; one launch per tick that has rows (``pds_multistream_pcen_*`` of the second stages library,
``csrc/pcen.hip``) takes every stream's new rows in order, in place, smoother and compression fused: a tick has one to
a few rows per stream.  The upload grows by the fresh flags, one byte per stream, and by what tells the kernel where a
stream's rows lie: its id and its first row, a word each (no section of a ``finalize`` tick carries them).
``finalize`` returns a stream to fresh.  :func:`StreamBatch.pcen_smooth` reads the streams' current M.

With `plp` (a :class:`post.PLP`, over a computer that does not take logs) every static row becomes its `num_ceps`
perceptual linear prediction cepstra -- the stage stands in `cepstra`'s place as the first post stage (it excludes
`cepstra` and `pcen`): one ``pds_plp_rows`` launch of the fourth stages library (``csrc/plp.hip``) over the tick's
static rows, none in a tick without rows, before `cmvn` / `sliding_cmvn`, `deltas` and `stack`, which see rows of
width `num_ceps`.  A row depends on nothing but itself, so the stage has no state, no pool and no upload section, and
the kernel is the one the offline calls launch: a stream's rows are ``stack(deltas(cmvn(plp.apply(statics))))`` of the
offline objects over its whole utterance, bit for bit, whatever the cuts.  The centre frequencies and the energy column
are the computer's where the object leaves them open (:func:`post.PLP.bound_to`).

With `stack` (a :class:`post.Stack`: frames along the row axis, ``pad_mode`` None, "edge" or "constant") every
``nv = num_vectors`` consecutive rows of a stream become one row of ``nv`` times the width -- the last stage, after
`cmvn` and `deltas`: a stream's rows, concatenated over its ``compute_chunks`` calls and its ``finalize``, are
``stack.apply(X, axis=-1)`` of the sequence X of rows the same object returns without `stack`, bit for bit (the stage
moves values and computes nothing, so NaN payloads and signed zeros pass).  Groups run on across ticks: a stream holds
``r < nv`` pending rows, those not yet returned; a tick that brings it m rows returns ``(r + m) // nv`` stacked rows
and keeps the other ``(r + m) % nv``; ``finalize`` returns the groups of what is left and drops the remainder
(``pad_mode=None``, as the reference does) or fills the last group with the stream's last row ("edge") or a constant
("constant", ``constant_values`` rounded to `dtype`), and nothing where nothing is left.  The other numpy pad modes look
at the whole utterance and are refused.  :class:`StackState` counts the pending rows per stream on the host; the device
keeps them in a ping-pong pool of ``2 * capacity * (nv - 1)`` rows, and one launch per tick
(``pds_multistream_stack_*``), the last, reads "pending rows, then the tick's new rows", writes the groups and the next
pending rows.  The row offsets of the packed calls count stacked rows; :attr:`StreamBatch.lookahead` stays the delay of
the deltas, in frames.

Not thread-safe; works on the current torch stream of the device that was current at construction.
"""
import functools
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native, config
from .alias import alias_factory_subclass_from_arg
from .compute import PackedLayout, ShortTimeFourierTransformFrameComputer
from .post import PCEN, PLP, Cepstra, Deltas, PostProcessor, SlidingCMVN, Stack, Standardize, refuse_log_computer
from .pre import Dither, Preemphasize, PreProcessor, dither_keys

__all__ = ["CmvnState", "DeltaState", "DitherState", "PcenState", "SlidingState", "StackState", "StreamBatch",
           "StreamState", "streaming_cepstra", "streaming_cmvn", "streaming_deltas", "streaming_dither", "streaming_pcen", "streaming_plp",
           "streaming_preemphasis", "streaming_sliding_cmvn", "streaming_stack"]

_FIELDS = 8  # int64 per entry of pds_multistream_assemble's metadata (include/pds_amd.h)
_DFIELDS = 8  # ... and of pds_multistream_deltas'
_CFIELDS = 8  # ... and of pds_multistream_cmvn's
_KFIELDS = 8  # ... and of pds_multistream_stack's
_WFIELDS = 8  # ... and of pds_multistream_sliding's (include/pds_amd_stages.h)
_PAD_NONE, _PAD_CONSTANT, _PAD_EDGE = 0, 1, 2  # the `pad` of pds_multistream_stack
_FLAG_FRESH = 1  # of the flags word of the cmvn metadata: the stream starts from the prior statistics
_FLAG_FINAL = 2  # (bit 0 of the flags word is the pool half)
_HAS_SAMPLE = 2  # of word 7 of the assemble metadata, beside the pool half in bit 0: the stream has a previous sample
_SAMPLES_F32, _SAMPLES_F64, _SAMPLES_I16 = 0, 1, 2  # PDS_SAMPLES_* (include/pds_amd.h)
_I16 = np.dtype(np.int16)


def _exclusive_cumsum(x: np.ndarray) -> np.ndarray:
    out = np.zeros(len(x) + 1, dtype=np.int64)
    np.cumsum(x, out=out[1:])
    return out


def _post_processor(name: str, arg, kind):
    """the shared opening of the ``streaming_*`` readers of the post stages: `arg`, keyword `name` of
    :class:`StreamBatch`, as ``alias_factory_subclass_from_arg(PostProcessor, ...)`` makes it, which must be a `kind`"""
    try:
        arg = alias_factory_subclass_from_arg(PostProcessor, arg)
    except (KeyError, TypeError) as e:
        raise ValueError(f"StreamBatch: {name} is no post-processor ({e!r})") from None
    if not isinstance(arg, kind):
        raise ValueError(f"StreamBatch: {name} must be a post.{kind.__name__}")
    return arg


def _typed(lib, name: str, dtype):
    """the entry point ``<name>_f32`` or ``<name>_f64`` of `lib` for samples of `dtype`; ``AttributeError`` from a
    library that does not have it"""
    return getattr(lib, name + ("_f32" if dtype == np.float32 else "_f64"))


class _StreamWords:
    """What the host states of both stream batches keep alike, per stream: ``started`` between the first chunk and
    ``finalize``, and one ``word`` as the assemble metadata takes it -- bit 0 the pool ``half`` holding the carry and
    the stream's previous sample (every tick that names the stream writes the other half), bit 1 ``has_sample``: given
    at least one sample since its start or last reset (a pre-emphasis has a previous sample to use) -- so a tick
    gathers and scatters the two once."""

    def __init__(self, capacity: int):
        capacity = int(capacity)
        if capacity <= 0:
            raise ValueError("capacity must be positive")
        self.capacity = capacity
        self.started = np.zeros(capacity, dtype=bool)
        self.word = np.zeros(capacity, dtype=np.int64)

    @property
    def half(self) -> np.ndarray:
        return self.word & 1

    @property
    def has_sample(self) -> np.ndarray:
        return (self.word & _HAS_SAMPLE) != 0

    @staticmethod
    def next_word(word: np.ndarray, lengths: np.ndarray) -> np.ndarray:
        """the words after a tick that brought the streams chunks of `lengths`"""
        return (word ^ 1) | (lengths > 0) * _HAS_SAMPLE

    def check_ids(self, ids) -> np.ndarray:
        """`ids` as int64, or ``ValueError`` if any is unknown, negative or repeated"""
        arr = np.asarray(ids)
        if arr.ndim != 1:
            raise ValueError("ids must be a 1-D sequence of stream indices")
        if arr.size == 0:
            return np.zeros(0, dtype=np.int64)
        if not np.issubdtype(arr.dtype, np.integer):
            raise ValueError("stream ids must be integers")
        arr = arr.astype(np.int64, copy=False)
        if arr.min() < 0 or arr.max() >= self.capacity:
            raise ValueError(f"stream ids must lie in [0, {self.capacity})")
        if np.unique(arr).size != arr.size:
            raise ValueError("a tick names each stream at most once")
        return arr


class StreamState(_StreamWords):
    """Host bookkeeping of many streams: the state machine of ``compute_chunk`` / ``finalize`` (compute.py) applied to
    arrays of streams.  Needs no device.

    Per stream: ``carry_len`` samples carried (always < `frame_length`), ``carry_pad`` left reflection the carry's
    first frame still needs, ``skip`` samples still to drop (`frame_shift` > `frame_length`), ``first`` no frame
    emitted yet, and ``started``, ``has_sample`` and ``half`` as :class:`_StreamWords` keeps them.
    """

    def __init__(self, capacity: int, frame_length: int, frame_shift: int, pad_left: int):
        super().__init__(capacity)
        capacity = self.capacity
        self.L, self.S, self.pad_left = int(frame_length), int(frame_shift), int(pad_left)
        self.carry_len = np.zeros(capacity, dtype=np.int64)
        self.carry_pad = np.full(capacity, self.pad_left, dtype=np.int64)
        self.skip = np.zeros(capacity, dtype=np.int64)
        self.first = np.ones(capacity, dtype=bool)

    def chunk_step(self, ids: np.ndarray, lengths: np.ndarray) -> dict:
        """What ``compute_chunk`` of chunks of `lengths` does to streams `ids` (compute.py ``compute_chunk``), without
        changing the state: per stream the samples `drop`ped from the chunk's start, the carry (`carry_len`, `cp`),
        the work span `avail` = carry + kept chunk, its frame count `k`, where the new carry starts in the span
        (`new_carry`) and the new state (``commit_chunks`` applies it)"""
        L, S = self.L, self.S
        lengths = np.asarray(lengths, dtype=np.int64)
        skip = self.skip[ids]
        drop = np.minimum(skip, lengths)
        skip = skip - drop
        c, cp, word = self.carry_len[ids], self.carry_pad[ids], self.word[ids]
        avail = c + lengths - drop
        k = np.maximum(0, (avail + cp - L) // S + 1)
        nxt = k * S - cp  # start of the next frame inside the span
        emit = k > 0
        fwd = emit & (nxt >= 0)
        new_carry = np.where(fwd, np.minimum(nxt, avail), 0)
        step = dict(
            drop=drop, carry_len=c, cp=cp, avail=avail, k=k, new_carry=new_carry,
            next_skip=np.where(fwd, np.maximum(0, nxt - avail), skip),
            next_cp=np.where(fwd, 0, np.where(emit, -nxt, cp)),
            next_first=self.first[ids] & ~emit,
            next_carry_len=avail - new_carry,
            word=word, next_word=self.next_word(word, lengths),
        )
        assert (step["next_carry_len"] < L).all()
        return step

    def commit_chunks(self, ids: np.ndarray, step: dict) -> None:
        self.skip[ids] = step["next_skip"]
        self.carry_pad[ids] = step["next_cp"]
        self.first[ids] = step["next_first"]
        self.carry_len[ids] = step["next_carry_len"]
        self.started[ids] = True
        # (the assemble kernel wrote the new carries and previous samples to the other half)
        self.word[ids] = step["next_word"]

    def finalize_step(self, ids: np.ndarray) -> dict:
        """What ``finalize`` does (compute.py ``finalize``): frames `k` from the carry (`carry_len`, left pad `cp`)"""
        S = self.S
        c, cp = self.carry_len[ids], self.carry_pad[ids]
        # (a stream that has not emitted a frame still has carry_pad == pad_left)
        num = np.where(self.first[ids], (c + S // 2) // S, (c + cp + S // 2 - self.pad_left) // S)
        k = np.where((num >= 1) & (c > 0), num, 0).astype(np.int64)
        return dict(carry_len=c, cp=cp, k=k, half=self.word[ids] & 1)

    def reset(self, ids: np.ndarray) -> None:
        self.carry_len[ids] = 0
        self.carry_pad[ids] = self.pad_left
        self.skip[ids] = 0
        self.first[ids] = True
        self.started[ids] = False
        self.word[ids] &= 1


def _no_streaming_reverb(pre) -> None:
    """``TypeError`` for a :class:`pre.Reverb`: its scale needs the whole utterance, so it has no per-stream form"""
    from .pre import Reverb

    if isinstance(pre, Reverb):
        raise TypeError("StreamBatch: pre.Reverb has no streaming form (its scale needs the whole utterance); "
                        "reverberate the utterances offline with Reverb.apply_packed")


def streaming_preemphasis(preemphasis) -> float:
    """`preemphasis` as :class:`StreamBatch` takes it -- a coefficient, a :class:`pre.Preemphasize` or what
    ``alias_factory_subclass_from_arg(PreProcessor, ...)`` makes one -> the coefficient, 0.0 for none (``None`` or a
    coefficient of 0); ``ValueError`` for anything else"""
    if preemphasis is None:
        return 0.0
    _no_streaming_reverb(preemphasis)
    if isinstance(preemphasis, (bool, np.bool_)):
        raise ValueError("StreamBatch: preemphasis must be a coefficient or a pre.Preemphasize")
    if not isinstance(preemphasis, (int, float, np.integer, np.floating)):
        try:
            pre = alias_factory_subclass_from_arg(PreProcessor, preemphasis)
        except (KeyError, TypeError, ValueError) as e:
            raise ValueError(f"StreamBatch: preemphasis is no coefficient and no pre-processor ({e!r})") from None
        if not isinstance(pre, Preemphasize):
            raise ValueError("StreamBatch: preemphasis must be a coefficient or a pre.Preemphasize")
        preemphasis = pre.coeff
        if isinstance(preemphasis, (bool, np.bool_)) or not isinstance(
                preemphasis, (int, float, np.integer, np.floating)):
            raise ValueError("StreamBatch: the pre-emphasis coefficient must be a number")
    coeff = float(preemphasis)
    if not np.isfinite(coeff):
        raise ValueError("StreamBatch: the pre-emphasis coefficient must be finite")
    return coeff


def streaming_dither(dither) -> Optional[Tuple[float, Optional[int]]]:
    """`dither` as :class:`StreamBatch` takes it -- a :class:`pre.Dither` or what
    ``alias_factory_subclass_from_arg(PreProcessor, ...)`` makes one -> ``(coeff, seed)`` with `seed` the ``Dither``'s
    own (None without one), or None for no dither (``None`` or a coefficient of 0); ``ValueError`` for anything else"""
    if dither is None:
        return None
    _no_streaming_reverb(dither)
    if isinstance(dither, (bool, np.bool_, int, float, np.integer, np.floating)):
        raise ValueError("StreamBatch: dither must be a pre.Dither (a bare number says nothing about the seed)")
    try:
        pre = alias_factory_subclass_from_arg(PreProcessor, dither)
    except (KeyError, TypeError, ValueError) as e:
        raise ValueError(f"StreamBatch: dither is no pre-processor ({e!r})") from None
    if not isinstance(pre, Dither):
        raise ValueError("StreamBatch: dither must be a pre.Dither")
    coeff, seed = pre.coeff, pre.seed
    if isinstance(coeff, (bool, np.bool_)) or not isinstance(coeff, (int, float, np.integer, np.floating)):
        raise ValueError("StreamBatch: the dither coefficient must be a number")
    coeff = float(coeff)
    if not np.isfinite(coeff):
        raise ValueError("StreamBatch: the dither coefficient must be finite")
    if seed is not None:
        if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 1 << 63:
            raise ValueError("StreamBatch: the dither seed must be an integer in [0, 2**63): the utterances' seeds "
                             "count up from it")
        seed = int(seed)
    if coeff == 0.0:
        return None
    return coeff, seed


class DitherState:
    """Host bookkeeping of the dither of many streams.  Needs no device.

    `base`: the seed of the first utterance the batch begins; ``count`` utterances begun so far, the next one has seed
    ``base + count``.  Per stream: ``seed`` of its current utterance (-1: none begun), ``key`` its generator key
    (:func:`pre.dither_keys`, the uint64's bits as int64) and ``pos`` raw samples received this utterance, dropped ones
    included: the position of its next chunk's first sample.
    """

    def __init__(self, capacity: int, base: int):
        capacity, base = int(capacity), int(base)
        if capacity <= 0 or not 0 <= base < 1 << 63:
            raise ValueError("capacity must be positive and the base seed lie in [0, 2**63)")
        self.capacity, self.base, self.count = capacity, base, 0
        self.seed = np.full(capacity, -1, dtype=np.int64)
        self.key = np.zeros(capacity, dtype=np.int64)
        self.pos = np.zeros(capacity, dtype=np.int64)

    def step(self, ids: np.ndarray, lengths: np.ndarray) -> dict:
        """What a tick that brings streams `ids` chunks of `lengths` does, without changing the state: the streams
        without an utterance begin one, in the order of `ids`, with the next seeds; per stream the `seed` and `key` of
        its utterance, the position `pos` of the chunk's first sample, and the state after the tick"""
        lengths = np.asarray(lengths, dtype=np.int64)
        seed, key = self.seed[ids], self.key[ids]  # (copies)
        fresh = np.flatnonzero(seed < 0)
        if len(fresh):
            first = self.base + self.count
            if first + len(fresh) > 1 << 63:
                raise OverflowError("the dither seeds have run past 2**63")
            seed[fresh] = first + np.arange(len(fresh), dtype=np.int64)
            key[fresh] = dither_keys(seed[fresh].tolist()).view(np.int64)
        pos = self.pos[ids]
        return dict(seed=seed, key=key, pos=pos, next_pos=pos + lengths, next_count=self.count + len(fresh))

    def commit(self, ids: np.ndarray, step: dict) -> None:
        self.seed[ids] = step["seed"]
        self.key[ids] = step["key"]
        self.pos[ids] = step["next_pos"]
        self.count = step["next_count"]

    def reset(self, ids: np.ndarray) -> None:
        """the streams' utterances are over (``finalize``): their next chunks begin new ones"""
        self.seed[ids] = -1
        self.key[ids] = 0
        self.pos[ids] = 0

    def fill_meta(self, meta: np.ndarray, step: dict) -> None:
        """pds_multistream_assemble_dither's second metadata section of a tick into `meta` (int64[n, 2])"""
        meta[:, 0] = step["pos"]
        meta[:, 1] = step["key"]


def streaming_deltas(deltas) -> Optional[Tuple[Deltas, int, int]]:
    """`deltas` as :class:`StreamBatch` takes it -> ``(Deltas, num_deltas, context_window)``, or None for no deltas
    (``deltas=None`` or ``num_deltas == 0``); ``ValueError`` for settings batched streaming does not serve"""
    if deltas is None:
        return None
    deltas = _post_processor("deltas", deltas, Deltas)
    K = int(deltas.num_deltas)
    if K < 0:
        raise ValueError("StreamBatch: num_deltas must not be negative")
    if deltas._pad_mode != "edge" or deltas._pad_kwargs:
        raise ValueError("StreamBatch: deltas must use pad_mode='edge' without pad arguments")
    if not deltas.concatenate:
        raise ValueError("StreamBatch: deltas must be concatenated (concatenate=True)")
    if deltas._target_axis not in (-1, 1):
        raise ValueError("StreamBatch: the deltas' target axis must be the coefficient axis of (rows, coeffs): -1 or 1")
    if K == 0:
        return None
    W = (len(deltas._filts[1]) - 1) // 2
    if W < 1:
        raise ValueError("StreamBatch: context_window must be positive")
    return deltas, K, W


class DeltaState:
    """Host bookkeeping of the delayed delta rows of many streams.  Needs no device.

    Per stream: ``seen`` static frames produced since its start, ``emitted`` rows returned, ``valid`` rows of its
    device history (``min(seen, 2 * lookahead)``: the frames ``seen - valid .. seen - 1``, oldest first), ``half`` the
    pool half holding it.
    """

    def __init__(self, capacity: int, lookahead: int):
        capacity, lookahead = int(capacity), int(lookahead)
        if capacity <= 0 or lookahead <= 0:
            raise ValueError("capacity and lookahead must be positive")
        self.capacity, self.H = capacity, lookahead
        self.hist_rows = 2 * lookahead
        self.seen = np.zeros(capacity, dtype=np.int64)
        self.emitted = np.zeros(capacity, dtype=np.int64)
        self.valid = np.zeros(capacity, dtype=np.int64)
        self.half = np.zeros(capacity, dtype=np.int64)

    def step(self, ids: np.ndarray, k: np.ndarray, final: bool = False) -> dict:
        """What a tick that brings streams `ids` `k` new static frames does, without changing the state.  Per stream,
        over the virtual sequence "`valid` history rows, then `k` new rows": `rows` output rows starting at row `first`
        of the sequence (all the stream's remaining ones if `final`, else those whose `H` frames of future are there),
        `keep` rows of next history (the sequence's last ones; none if `final`) and the `half` the history is read
        from"""
        H = self.H
        k = np.asarray(k, dtype=np.int64)
        seen, emitted, valid = self.seen[ids], self.emitted[ids], self.valid[ids]
        n, V = seen + k, valid + k
        rows = n - emitted if final else np.maximum(0, n - H) - emitted
        first = emitted - (seen - valid)
        keep = np.zeros_like(V) if final else np.minimum(V, self.hist_rows)
        # the kernel's clamp of a row index to the sequence is "edge" padding and nothing else: every row a tap reads
        # is in the sequence, unless it lies before the stream's frame 0 (row 0 of the sequence is then frame 0) or,
        # in a finalize, after its last frame
        assert (rows >= 0).all() and (first >= 0).all() and (first + rows <= V).all()
        assert ((first - H >= 0) | (seen == valid) | (rows == 0)).all()
        assert final or (first + rows - 1 + H <= V - 1)[rows > 0].all()
        return dict(valid=valid, k=k, first=first, rows=rows, keep=keep, half=self.half[ids], final=bool(final),
                    next_seen=n, next_emitted=emitted + rows)

    def commit(self, ids: np.ndarray, step: dict) -> None:
        if step["final"]:
            self.reset(ids)
            return
        self.seen[ids] = step["next_seen"]
        self.emitted[ids] = step["next_emitted"]
        self.valid[ids] = step["keep"]
        self.half[ids] ^= 1  # (the deltas kernel wrote the next histories to the other half)

    def reset(self, ids: np.ndarray) -> None:
        self.seen[ids] = 0
        self.emitted[ids] = 0
        self.valid[ids] = 0

    def fill_meta(self, meta: np.ndarray, prefix: np.ndarray, ids: np.ndarray, step: dict, static_rows: np.ndarray,
                  out_rows: np.ndarray, coeffs: int) -> int:
        """pds_multistream_deltas' metadata of a tick into `meta` (int64[n, 8]) and `prefix` (int64[n + 1], elements
        per entry as an exclusive prefix sum); `static_rows` / `out_rows`: each stream's first row in the tick's
        statics and in its output.  Returns the number of elements"""
        meta[:, 0] = ids
        meta[:, 1] = step["half"] | (_FLAG_FINAL if step["final"] else 0)
        meta[:, 2] = step["valid"]
        meta[:, 3] = step["k"]
        meta[:, 4] = static_rows
        meta[:, 5] = step["first"]
        meta[:, 6] = step["rows"]
        meta[:, 7] = out_rows
        prefix[0] = 0
        np.cumsum((step["rows"] + step["keep"]) * int(coeffs), out=prefix[1:])
        return int(prefix[-1])


def streaming_cepstra(cepstra) -> Optional[Cepstra]:
    """`cepstra` as :class:`StreamBatch` takes it -- a :class:`post.Cepstra` or what
    ``alias_factory_subclass_from_arg(PostProcessor, ...)`` makes one (``"mfcc"``, ``{"name": "mfcc", "num_ceps": 13}``)
    -> the ``Cepstra``, or None for ``cepstra=None``; ``ValueError`` for anything else"""
    if cepstra is None:
        return None
    cepstra = _post_processor("cepstra", cepstra, Cepstra)
    return cepstra


def streaming_cmvn(cmvn, running: bool, num_coeffs: int) -> Optional[Tuple[Standardize, Optional[np.ndarray], bool]]:
    """`cmvn` as :class:`StreamBatch` takes it -- a :class:`post.Standardize` or what
    ``alias_factory_subclass_from_arg(PostProcessor, ...)`` makes one -> ``(Standardize, prior, norm_var)`` with `prior`
    a float64 copy of its ``[2, num_coeffs + 1]`` statistics (None without any), or None for ``cmvn=None``;
    ``ValueError`` for anything that is no ``Standardize``, for statistics of another width, for a count that is not a
    whole number, and for ``running=False`` without statistics: per-utterance statistics need the whole utterance,
    which a stream does not have"""
    if cmvn is None:
        return None
    cmvn = _post_processor("cmvn", cmvn, Standardize)
    prior = None
    if cmvn._stats is not None:
        prior = np.array(cmvn._stats, dtype=np.float64)
        if prior.ndim != 2 or prior.shape != (2, int(num_coeffs) + 1):
            raise ValueError(f"StreamBatch: the cmvn statistics have shape {prior.shape}, the computer's "
                             f"{num_coeffs} coefficients need (2, {int(num_coeffs) + 1})")
        count = prior[0, -1]
        if not (0 <= count < 2.0 ** 52 and count == np.floor(count)):
            raise ValueError("StreamBatch: the count of the cmvn statistics must be a whole number")
        if not count:
            prior = None  # (Standardize.have_stats: statistics of no frame are none)
    if prior is None and not running:
        raise ValueError("StreamBatch: cmvn_running=False needs accumulated statistics (Standardize(rfilename=...) or "
                         "accumulate()): per-utterance statistics need the whole utterance, which a stream does not "
                         "have -- standardise after finalize, or use running statistics")
    return cmvn, prior, bool(cmvn._norm_var)


class CmvnState:
    """Host bookkeeping of the running statistics of many streams.  Needs no device.

    Per stream: ``seen`` static frames accumulated since its start or last ``finalize``; a stream that has none is
    ``fresh``: its sums are the prior's, and its slot of the device pool is not read.  `prior_count`: the count of the
    prior statistics (0 without any); `running`: whether frames are accumulated at all (global statistics: the count a
    tick is given is the prior's, always).
    """

    def __init__(self, capacity: int, prior_count: int = 0, running: bool = True):
        capacity, prior_count = int(capacity), int(prior_count)
        if capacity <= 0 or prior_count < 0:
            raise ValueError("capacity must be positive and the prior count not negative")
        if not running and not prior_count:
            raise ValueError("global statistics need a prior")
        self.capacity, self.prior_count, self.running = capacity, prior_count, bool(running)
        self.seen = np.zeros(capacity, dtype=np.int64)

    @property
    def fresh(self) -> np.ndarray:
        return self.seen == 0

    def counts(self, ids: np.ndarray) -> np.ndarray:
        """the count of the streams' current statistics"""
        seen = self.seen[ids]
        return self.prior_count + (seen if self.running else np.zeros_like(seen))

    def step(self, ids: np.ndarray, k: np.ndarray, final: bool = False) -> dict:
        """What a tick that brings streams `ids` `k` new static frames does, without changing the state: per stream
        the `count` before the tick, whether it is `fresh`, and the frames seen after it"""
        k = np.asarray(k, dtype=np.int64)
        seen = self.seen[ids]
        return dict(k=k, count=self.counts(ids), fresh=seen == 0, next_seen=seen + k, final=bool(final))

    def commit(self, ids: np.ndarray, step: dict) -> None:
        if step["final"]:
            self.reset(ids)  # (the next utterance on the id starts from the prior again)
        else:
            self.seen[ids] = step["next_seen"]

    def reset(self, ids: np.ndarray) -> None:
        self.seen[ids] = 0

    def fill_meta(self, meta: np.ndarray, ids: np.ndarray, step: dict, static_rows: np.ndarray) -> None:
        """pds_multistream_cmvn's metadata of a tick into `meta` (int64[n, 8]); `static_rows`: each stream's first row
        in the tick's statics"""
        meta[:, 0] = ids
        meta[:, 1] = step["fresh"] * _FLAG_FRESH
        meta[:, 2] = static_rows
        meta[:, 3] = step["k"]
        meta[:, 4] = step["count"]
        meta[:, 5:] = 0


def streaming_sliding_cmvn(sliding_cmvn) -> Optional[SlidingCMVN]:
    """`sliding_cmvn` as :class:`StreamBatch` takes it -- a :class:`post.SlidingCMVN` or what
    ``alias_factory_subclass_from_arg(PostProcessor, ...)`` makes one (``{"name": "sliding_cmvn", "cmn_window": 600,
    "min_window": 1}``) -> the ``SlidingCMVN``, or None for ``sliding_cmvn=None``; ``ValueError`` for anything else, for
    a centred window and for ``min_window != 1``, which a stream cannot serve"""
    if sliding_cmvn is None:
        return None
    sliding_cmvn = _post_processor("sliding_cmvn", sliding_cmvn, SlidingCMVN)
    if sliding_cmvn.center:
        raise ValueError("StreamBatch: sliding_cmvn must use center=False: a centred window needs cmn_window // 2 "
                         "frames of the future, which a stream does not have")
    if sliding_cmvn.min_window != 1:
        raise ValueError("StreamBatch: sliding_cmvn must use min_window=1: with a larger one a stream's first rows "
                         "would have to wait for later ones (holding rows back is not served)")
    return sliding_cmvn


class SlidingState:
    """Host bookkeeping of the sliding-window CMVN of many streams.  Needs no device.

    `window`: ``cmn_window``; the device ring holds ``window + 1`` rows per stream.  Per stream: ``seen`` static frames
    normalised since its start or last ``finalize`` -- its next row is frame ``seen`` of its utterance, which goes to
    slot ``seen % (window + 1)`` of its ring; a stream that has none is ``fresh``: its ring and sums are not read.
    """

    def __init__(self, capacity: int, window: int, refresh: Optional[int] = None):
        capacity, window = int(capacity), int(window)
        refresh = window if refresh is None else int(refresh)
        if capacity <= 0 or window <= 0 or refresh <= 0:
            raise ValueError("capacity, window and refresh must be positive")
        self.capacity, self.window, self.refresh = capacity, window, refresh
        self.ring_rows = window + 1
        self.seen = np.zeros(capacity, dtype=np.int64)

    @property
    def fresh(self) -> np.ndarray:
        return self.seen == 0

    def step(self, ids: np.ndarray, k: np.ndarray, final: bool = False) -> dict:
        """What a tick that brings streams `ids` `k` new static frames does, without changing the state: per stream
        the frames `seen` before the tick, whether it is `fresh`, and the frames seen after it"""
        k = np.asarray(k, dtype=np.int64)
        seen = self.seen[ids]
        return dict(k=k, seen=seen, fresh=seen == 0, next_seen=seen + k, final=bool(final))

    def commit(self, ids: np.ndarray, step: dict) -> None:
        if step["final"]:
            self.reset(ids)  # (the next utterance on the id starts with an empty window)
        else:
            self.seen[ids] = step["next_seen"]

    def reset(self, ids: np.ndarray) -> None:
        self.seen[ids] = 0

    def fill_meta(self, meta: np.ndarray, ids: np.ndarray, step: dict, static_rows: np.ndarray) -> None:
        """pds_multistream_sliding's metadata of a tick into `meta` (int64[n, 8]); `static_rows`: each stream's first
        row in the tick's statics"""
        meta[:, 0] = ids
        meta[:, 1] = step["fresh"] * _FLAG_FRESH
        meta[:, 2] = static_rows
        meta[:, 3] = step["k"]
        meta[:, 4] = step["seen"]
        meta[:, 5:] = 0


def streaming_plp(plp, computer=None) -> Optional[PLP]:
    """`plp` as :class:`StreamBatch` takes it -- a :class:`post.PLP` or what
    ``alias_factory_subclass_from_arg(PostProcessor, ...)`` makes one (``"plp"``, ``{"name": "plp", "num_ceps": 13}``)
    -> the ``PLP``, or None for ``plp=None``; ``ValueError`` for anything else.  Given the `computer`, the ``PLP`` bound
    to it (:func:`post.PLP.bound_to`: centre frequencies and `energy` from the computer where the object leaves them
    open), a ``ValueError`` for a computer that takes logs and for a width the object refuses"""
    if plp is None:
        return None
    plp = _post_processor("plp", plp, PLP)
    if computer is not None:
        plp = plp.bound_to(computer)
        plp._split(computer.num_coeffs)
    return plp


def streaming_pcen(pcen, computer=None) -> Optional[PCEN]:
    """`pcen` as :class:`StreamBatch` takes it -- a :class:`post.PCEN` or what
    ``alias_factory_subclass_from_arg(PostProcessor, ...)`` makes one (``"pcen"``, ``{"name": "pcen", "smooth": 0.025}``)
    -> the ``PCEN``, or None for ``pcen=None``; ``ValueError`` for anything else and, given the `computer`, for one that
    takes logs"""
    if pcen is None:
        return None
    pcen = _post_processor("pcen", pcen, PCEN)
    if computer is not None:
        refuse_log_computer(computer)
    return pcen


class PcenState:
    """Host bookkeeping of the PCEN smoother of many streams.  Needs no device.

    Per stream: whether it is ``live`` -- it has had a static row since its start or last ``finalize``, so its slot of
    the device pool holds its last M; a stream that is not is ``fresh``: its next row is the first of its utterance
    (``M = E``), and its slot is not read.
    """

    def __init__(self, capacity: int):
        capacity = int(capacity)
        if capacity <= 0:
            raise ValueError("capacity must be positive")
        self.capacity = capacity
        self.live = np.zeros(capacity, dtype=bool)

    @property
    def fresh(self) -> np.ndarray:
        return ~self.live

    def step(self, ids: np.ndarray, k: np.ndarray, final: bool = False) -> dict:
        """What a tick that brings streams `ids` `k` new static frames does, without changing the state: per stream
        whether it is `fresh` before the tick and whether it is live after it"""
        k = np.asarray(k, dtype=np.int64)
        live = self.live[ids]
        return dict(k=k, fresh=~live, next_live=live | (k > 0), final=bool(final))

    def commit(self, ids: np.ndarray, step: dict) -> None:
        if step["final"]:
            self.reset(ids)  # (the next utterance on the id starts its smoother anew)
        else:
            self.live[ids] = step["next_live"]

    def reset(self, ids: np.ndarray) -> None:
        self.live[ids] = False

    def fill_meta(self, d_ids: np.ndarray, d_rows: np.ndarray, d_fresh: np.ndarray, ids: np.ndarray, step: dict,
                  rows: np.ndarray) -> None:
        """pds_multistream_pcen's three arrays of a tick: the stream ids into `d_ids` (int64[n]), every stream's first
        row in the tick's statics and the end of the last one's, `rows`, into `d_rows` (int64[n + 1]), and the fresh
        flags, one byte per stream, into the front of the words `d_fresh` (int64[ceil(n / 8)])"""
        d_ids[:] = ids
        d_rows[:] = rows
        d_fresh[:] = 0
        d_fresh.view(np.uint8)[: len(ids)] = step["fresh"]


def streaming_stack(stack) -> Optional[Tuple[Stack, int, int, float]]:
    """`stack` as :class:`StreamBatch` takes it -- a :class:`post.Stack` or what
    ``alias_factory_subclass_from_arg(PostProcessor, ...)`` makes one -> ``(Stack, num_vectors, pad, fill)`` with `pad`
    as pds_multistream_stack takes it (0 none, 1 constant, 2 edge) and `fill` the constant (0.0 unless given), or None
    for no stacking (``stack=None`` or ``num_vectors == 1``); ``ValueError`` for settings batched streaming does not
    serve"""
    if stack is None:
        return None
    stack = _post_processor("stack", stack, Stack)
    nv = stack.num_vectors
    if isinstance(nv, (bool, np.bool_)) or not isinstance(nv, (int, np.integer)) or nv < 1:
        raise ValueError("StreamBatch: num_vectors must be a positive integer")
    if isinstance(stack.time_axis, (bool, np.bool_)) or stack.time_axis not in (0, -2):
        raise ValueError("StreamBatch: the stack's time axis must be the row axis of (rows, coeffs): 0 or -2")
    mode, kwargs = stack._pad_mode, stack._pad_kwargs
    fill = 0.0
    if mode is None:
        pad = _PAD_NONE
    elif isinstance(mode, str) and mode == "edge":
        pad = _PAD_EDGE
    elif isinstance(mode, str) and mode == "constant":
        pad = _PAD_CONSTANT
    else:
        raise ValueError(f"StreamBatch: stack must use pad_mode None, 'edge' or 'constant', not {mode!r}: the other "
                         "numpy pad modes need the whole utterance, which a stream does not have -- stack after "
                         "finalize")
    if kwargs and (pad != _PAD_CONSTANT or set(kwargs) != {"constant_values"}):
        raise ValueError("StreamBatch: the only pad argument of stack is a scalar constant_values with "
                         "pad_mode='constant'")
    if kwargs:
        value = kwargs["constant_values"]
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
            raise ValueError("StreamBatch: the stack's constant_values must be a scalar number")
        fill = float(value)
    if nv == 1:
        return None
    return stack, int(nv), pad, fill


class StackState:
    """Host bookkeeping of the frame stacking of many streams.  Needs no device.

    `num_vectors` rows make a group; `pad`: a ``finalize`` fills a last, partial group instead of dropping it.  Per
    stream: ``pending`` rows given to the stage but not returned yet (always < `num_vectors`; they lie in the device
    pool, oldest first) and ``half`` the pool half holding them.
    """

    def __init__(self, capacity: int, num_vectors: int, pad: bool = False):
        capacity, num_vectors = int(capacity), int(num_vectors)
        if capacity <= 0 or num_vectors <= 0:
            raise ValueError("capacity and num_vectors must be positive")
        self.capacity, self.nv, self.pad = capacity, num_vectors, bool(pad)
        self.pool_rows = num_vectors - 1
        self.pending = np.zeros(capacity, dtype=np.int64)
        self.half = np.zeros(capacity, dtype=np.int64)

    def step(self, ids: np.ndarray, m: np.ndarray, final: bool = False) -> dict:
        """What a tick that brings streams `ids` `m` new rows does, without changing the state.  Per stream, over the
        virtual sequence "`pending` rows, then `m` new rows": `groups` stacked rows (the whole groups of the sequence;
        if `final` under a padding a last partial one too), `keep` rows of next pending ones (the sequence's rows behind
        the groups; none if `final`) and the `half` the pending rows are read from"""
        nv = self.nv
        m = np.asarray(m, dtype=np.int64)
        pending, half = self.pending[ids], self.half[ids]
        V = pending + m
        padded = final and self.pad
        groups = (V + (nv - 1)) // nv if padded else V // nv
        rest = V - groups * nv  # rows of the sequence behind the groups; negative: rows the last group lacks
        keep = np.zeros_like(V) if final else rest
        # the kernel reads row q of the sequence for every q < groups * nv + keep.  All of them are in the sequence --
        # and what is kept fits the pool -- unless a finalize pads: then fewer than a group's are not, and the
        # sequence has a last row to repeat (no rows give no group)
        assert len(m) == 0 or m.min() >= 0
        if padded:
            assert ((rest <= 0) & (rest > -nv) & ((V > 0) | (groups == 0))).all()
        else:
            assert ((rest >= 0) & (rest <= self.pool_rows)).all()
        return dict(pending=pending, m=m, groups=groups, keep=keep, half=half, final=bool(final))

    def commit(self, ids: np.ndarray, step: dict) -> None:
        if step["final"]:
            self.reset(ids)
            return
        self.pending[ids] = step["keep"]
        self.half[ids] = step["half"] ^ 1  # (the stack kernel wrote the next pending rows to the other half)

    def reset(self, ids: np.ndarray) -> None:
        self.pending[ids] = 0

    def fill_meta(self, meta: np.ndarray, prefix: np.ndarray, ids: np.ndarray, step: dict, new_rows: np.ndarray,
                  out_rows: np.ndarray, coeffs: int) -> int:
        """pds_multistream_stack's metadata of a tick into `meta` (int64[n, 8]) and `prefix` (int64[n + 1], elements
        per entry as an exclusive prefix sum); `new_rows` / `out_rows`: each stream's first row in the tick's rows and
        in its output.  Returns the number of elements"""
        meta[:, 0] = ids
        meta[:, 1] = step["half"] | (_FLAG_FINAL if step["final"] else 0)
        meta[:, 2] = step["pending"]
        meta[:, 3] = step["m"]
        meta[:, 4] = new_rows
        meta[:, 5] = step["groups"]
        meta[:, 6] = out_rows
        meta[:, 7] = 0
        prefix[0] = 0
        np.cumsum((step["groups"] * self.nv + step["keep"]) * int(coeffs), out=prefix[1:])
        return int(prefix[-1])


class _Upload:
    """A tick's one upload, in int64 words: `sample_words` of samples, then the sections of `layout`
    (:func:`_place`) back to back.  `words` is the sum: what the tick asks of the staging and what it sends.  The
    sections are placed relative to the end of the samples, so `sample_words` may still be lowered after the staging
    was asked (a tick that travels as int16 takes fewer words than its size in `dtype`).  ``host(name)`` / ``dev(name)``
    are the views of a section (or of ``"samples"``), in its shape, of `pinned` (the staging buffer's words, a numpy
    array) and of `device` (the tensor :func:`_TickBatch._send` returns); an empty section has valid empty views."""

    def __init__(self, sample_words, layout):
        self.sample_words = sample_words
        self.at, self.section_words = layout
        self.pinned = self.device = None

    @property
    def words(self):
        return self.sample_words + self.section_words

    def host(self, name):
        if name == "samples":
            return self.pinned[: self.sample_words]
        lo, size, shape, _ = self.at[name]
        lo += self.sample_words
        return self.pinned[lo : lo + size].reshape(shape)

    def dev(self, name):
        if name == "samples":
            return self.device[: self.sample_words]
        lo, _, shape, strides = self.at[name]
        # (`device` is a whole tensor: its storage starts at its word 0)
        return self.device.as_strided(shape, strides, self.sample_words + lo)


def _place(sections):
    """`sections` -- ``(name, shape)`` with one- or two-dimensional shapes, in int64 words -- back to back in the order
    given -> ``({name: (first word, words, shape, strides)}, words of all)``.  A section that a tick does not have has a
    zero in its shape and takes no words"""
    at = {}
    off = 0
    for name, shape in sections:
        if len(shape) == 2:
            size, strides = shape[0] * shape[1], (shape[1], 1)
        else:
            size, strides = shape[0], (1,)
        at[name] = (off, size, shape, strides)
        off += size
    return at, off


@functools.lru_cache(maxsize=256)  # (a batch's ticks repeat a few sizes: each is placed once)
def _tick_layout(n, E, launch_rows, chunks, deltas, cmvn, stack=False, dither=False, sliding=False, pcen=False):
    """The sections behind the samples in the upload of a tick over `n` streams of which `E` emit frames, placed: the
    assemble metadata and the tile prefix (`chunks`: a ``compute_chunks`` tick; ``finalize`` has neither, and no
    samples), the launch metadata -- `launch_rows` rows, one column per emitting stream --, the deltas metadata and
    the element prefix (`deltas`), the cmvn metadata (`cmvn`), the stack metadata and its element prefix (`stack`), the
    positions and keys of the dither (`dither`, in a ``compute_chunks`` tick), the sliding-window cmvn metadata
    (`sliding`), the ids, row prefix and fresh bytes of the PCEN (`pcen`)"""
    # (a batch without `stack` / `dither` / `sliding` / `pcen` has the layout it had before there was one: their
    # sections are not placed at all)
    return _place((("assemble", (n if chunks else 0, _FIELDS)),
                   ("tiles", (n + 1 if chunks else 0,)),
                   ("launch", (launch_rows, E)),
                   ("deltas", (n if deltas else 0, _DFIELDS)),
                   ("elems", (n + 1 if deltas else 0,)),
                   ("cmvn", (n if cmvn else 0, _CFIELDS)))
                  + ((("stack", (n, _KFIELDS)), ("stack_elems", (n + 1,))) if stack else ())
                  + ((("dither", (n if chunks else 0, 2)),) if dither else ())
                  + ((("sliding", (n, _WFIELDS)),) if sliding else ())
                  + ((("pcen_ids", (n,)), ("pcen_rows", (n + 1,)), ("pcen_fresh", ((n + 7) // 8,))) if pcen else ()))


class _Stage:
    """One post stage of a batch `b`, as :func:`_TickBatch._tick` drives it (the protocol is in the module docstring).

    `spec`: the parsed keyword.  `state`: the host state.  `width_in` / `width`: a row's coefficients entering and
    leaving the stage.  `pools`: the device memory it keeps across ticks, by name.  `sections`: its sections of the
    upload, the metadata first; :func:`_tick_layout` places them under the flag of the stage.  `counts`: for a stage
    that makes rows of its own out of "what the stream keeps on the device, then the tick's new rows", the key of the
    step's rows per stream; its second section is then the elements per entry as a prefix sum, and it launches in
    every tick (a ``finalize`` returns rows without bringing any).  A stage without `counts` works on the rows where
    they lie, and its launch is left out in a tick without rows: none of its pools changes then.  A subclass builds
    the state and the pools, looks its typed entry point up -- there and nowhere else -- and has :func:`_run`, the
    launch and its check, given the rows, the output (the rows themselves without `counts`), the device pointers of
    the sections, the number of streams, the step and the stream's handle."""

    sections = ()
    state = counts = None

    def __init__(self, batch, spec, width):
        self.b, self.spec, self.width_in, self.width, self.pools = batch, spec, width, width, {}

    def plan(self, up, ids, rows, final):
        """the host half of a tick, before the upload: changes no state, fills the stage's sections of `up` and keeps
        the step; `rows`: every stream's first row in what enters the stage (an exclusive prefix).  Returns the same of
        what leaves it"""
        step = self._step = self.state.step(ids, rows[1:] - rows[:-1], final=final)
        out, extra = rows, ()
        if self.counts:
            out = step["out"] = _exclusive_cumsum(step[self.counts])
            extra = (out[:-1], self.width_in)
        step["elems"] = self.state.fill_meta(*map(up.host, self.sections), ids, step, rows[:-1], *extra)
        return out

    def launch(self, up, rows, ids, stream):
        """the device half, after the feature launch: the stage's one launch over the `rows` that enter it, then the
        commit of its host state.  Returns the rows that leave it"""
        step, b, out = self._step, self.b, rows
        if self.counts:
            out = b._torch.empty((int(step["out"][-1]), self.width), dtype=b._tdtype, device=b.device)
        if self.counts or rows.shape[0]:
            self._run(rows, out, [up.dev(name).data_ptr() for name in self.sections], len(ids), step,
                      stream.cuda_stream)
        self.state.commit(ids, step)
        return out

    def release(self):
        self.pools = {}


class _PcenStage(_Stage):
    """`pcen`, a kernel of the second stages library: the first post stage, in place.  Pool: ``smooth``, every
    stream's last M, float64 ``(capacity, F)`` (a fresh stream's is not read: no fill)"""

    sections = ("pcen_ids", "pcen_rows", "pcen_fresh")

    def __init__(self, batch, spec, width):
        super().__init__(batch, spec, width)
        self.state = PcenState(batch.capacity)
        self._fn = _typed(_native.stages2_lib(), "pds_multistream_pcen", batch.dtype)
        self.pools["smooth"] = batch._torch.empty((batch.capacity, width), dtype=batch._torch.float64,
                                                  device=batch.device)

    def plan(self, up, ids, rows, final):
        step = self._step = self.state.step(ids, rows[1:] - rows[:-1], final=final)
        self.state.fill_meta(*map(up.host, self.sections), ids, step, rows)
        return rows

    def _run(self, statics, out, sections, n, step, stream):
        spec = self.spec
        rc = self._fn(statics.data_ptr(), self.pools["smooth"].data_ptr(), self.b.capacity, self.width, spec.smooth_coeff,
                      spec.oms, spec.gain, spec.bias, spec.power, spec.eps, spec.bp, *sections, n, stream)
        _native.check_stages2(rc, "pds_multistream_pcen")

    def smooth(self, ids: np.ndarray) -> np.ndarray:
        """:func:`StreamBatch.pcen_smooth` of the checked `ids`"""
        out = np.full((len(ids), self.width), np.nan, dtype=np.float64)
        live = np.flatnonzero(self.state.live[ids])
        if len(live):
            at = self.b._torch.from_numpy(ids[live]).to(self.b.device)
            out[live] = self.pools["smooth"][at].cpu().numpy()
        return out


class _CepstraStage(_Stage):
    """`cepstra`: a row depends on nothing but itself -- no state, no pool, no section"""

    def __init__(self, batch, spec, width):
        super().__init__(batch, spec, width)
        self.width = spec.num_ceps

    def plan(self, up, ids, rows, final):
        return rows

    def launch(self, up, rows, ids, stream):
        return self.spec.apply(rows)  # one launch on `stream`, none without rows


class _PlpStage(_Stage):
    """`plp`, a kernel of the fourth stages library, in `cepstra`'s place: a row depends on nothing but itself -- no
    state, no pool, no section"""

    def __init__(self, batch, spec, width):
        super().__init__(batch, spec, width)
        self.width = spec.num_ceps
        _native.stages4_lib()  # (a missing or stale library is an error here, not in the first tick)

    def plan(self, up, ids, rows, final):
        return rows

    def launch(self, up, rows, ids, stream):
        return self.spec.apply_rows(rows)  # one launch on `stream`, none without rows


class _CmvnStage(_Stage):
    """`cmvn`: `spec` is :func:`streaming_cmvn`'s ``(Standardize, prior, norm_var)`` and whether the statistics run.
    Pools: ``sums``, float64 ``(capacity, 2, F)`` (running statistics only; a fresh stream's slot is never read: no
    fill), and ``prior``, the statistics passed in without their count (if any)"""

    sections = ("cmvn",)

    def __init__(self, batch, spec, width):
        super().__init__(batch, spec, width)
        _, self.prior, self._norm_var, running = spec
        torch = batch._torch
        self.state = CmvnState(batch.capacity, int(self.prior[0, -1]) if self.prior is not None else 0, running)
        if self.prior is not None:
            self.pools["prior"] = torch.from_numpy(np.ascontiguousarray(self.prior[:, :-1])).to(batch.device)
        if running:
            self.pools["sums"] = torch.empty((batch.capacity, 2, width), dtype=torch.float64, device=batch.device)
        self._fn = _typed(batch._lib, "pds_multistream_cmvn", batch.dtype)

    def _run(self, statics, out, sections, n, step, stream):
        sums, prior = self.pools.get("sums"), self.pools.get("prior")
        rc = self._fn(statics.data_ptr(), sums.data_ptr() if sums is not None else None, self.b.capacity, self.width,
                      prior.data_ptr() if prior is not None else None, int(self._norm_var), int(self.state.running),
                      *sections, n, stream)
        _native.check(rc, "pds_multistream_cmvn")

    def stats(self, ids: np.ndarray) -> np.ndarray:
        """:func:`StreamBatch.cmvn_stats` of the checked `ids`"""
        F = self.width
        out = np.zeros((len(ids), 2, F + 1), dtype=np.float64)
        if self.prior is not None:
            out[:] = self.prior
        live = np.flatnonzero(~self.state.fresh[ids]) if self.state.running else np.zeros(0, dtype=np.int64)
        if len(live):
            at = self.b._torch.from_numpy(ids[live]).to(self.b.device)
            out[live, :, :F] = self.pools["sums"][at].cpu().numpy()
            out[live, 0, F] = self.state.counts(ids[live])
        return out


class _SlidingStage(_Stage):
    """`sliding_cmvn`, a kernel of the stages library.  Pools: ``ring``, every stream's last ``cmn_window + 1`` static
    rows, ``(capacity, cmn_window + 1, F)`` of `dtype`, and ``sums``, float64 ``(capacity, 2, F)`` (a fresh stream's
    are not read: no fill)"""

    sections = ("sliding",)

    def __init__(self, batch, spec, width):
        super().__init__(batch, spec, width)
        torch, dev = batch._torch, batch.device
        self.state = SlidingState(batch.capacity, spec.cmn_window, spec.refresh)
        self._fn = _typed(_native.stages_lib(), "pds_multistream_sliding", batch.dtype)
        self.pools["ring"] = torch.empty((batch.capacity, self.state.ring_rows, width), dtype=batch._tdtype, device=dev)
        self.pools["sums"] = torch.empty((batch.capacity, 2, width), dtype=torch.float64, device=dev)

    def _run(self, statics, out, sections, n, step, stream):
        spec = self.spec
        rc = self._fn(statics.data_ptr(), self.pools["ring"].data_ptr(), self.pools["sums"].data_ptr(),
                      self.b.capacity, self.width, spec.cmn_window, int(spec.norm_vars), spec.refresh, *sections, n,
                      stream)
        _native.check_stages(rc, "pds_multistream_sliding")


class _DeltasStage(_Stage):
    """`deltas`: `spec` is :func:`streaming_deltas`'s ``(Deltas, num_deltas, context_window)``.  Pool: ``hist``, two
    halves of every stream's last ``2 H`` static rows, ``(2, capacity, 2 H, F)`` of `dtype`"""

    sections = ("deltas", "elems")
    counts = "rows"

    def __init__(self, batch, spec, width):
        super().__init__(batch, spec, width)
        deltas, self._K, W = spec
        self.state = DeltaState(batch.capacity, self._K * W)
        self.width = (self._K + 1) * width
        self.pools["hist"] = batch._torch.zeros((2, batch.capacity, self.state.hist_rows, width), dtype=batch._tdtype,
                                                device=batch.device)
        self._filts, self._filt_off = deltas._filters_on(batch.device)
        self._fn = _typed(batch._lib, "pds_multistream_deltas", batch.dtype)

    def _run(self, statics, out, sections, n, step, stream):
        rc = self._fn(statics.data_ptr() if statics.shape[0] else None, self.pools["hist"].data_ptr(),
                      self.b.capacity, self.state.hist_rows, self.width_in, self._filts.data_ptr(),
                      self._filt_off.data_ptr(), self._K, *sections, n, step["elems"], out.data_ptr(), stream)
        _native.check(rc, "pds_multistream_deltas")


class _StackStage(_Stage):
    """`stack`: `spec` is :func:`streaming_stack`'s ``(Stack, num_vectors, pad, fill)``; `fill` is the constant
    rounded to `dtype`, as ``numpy.pad`` rounds it.  Pool: ``pending``, two halves of every stream's rows not yet
    returned, ``(2, capacity, num_vectors - 1, C)`` of `dtype` (a stream without any has nothing read from its slot: no
    fill)"""

    sections = ("stack", "stack_elems")
    counts = "groups"

    def __init__(self, batch, spec, width):
        super().__init__(batch, spec, width)
        _, nv, self._pad, fill = spec
        self.fill = float(batch.dtype.type(fill))
        self.state = StackState(batch.capacity, nv, self._pad != _PAD_NONE)
        self.width = nv * width
        self.pools["pending"] = batch._torch.empty((2, batch.capacity, nv - 1, width), dtype=batch._tdtype,
                                                   device=batch.device)
        self._fn = _typed(batch._lib, "pds_multistream_stack", batch.dtype)

    def _run(self, new, out, sections, n, step, stream):
        rc = self._fn(new.data_ptr() if new.shape[0] else None, self.pools["pending"].data_ptr(), self.b.capacity,
                      self.state.nv, self.width_in, *sections, n, step["elems"], self._pad, self.fill,
                      out.data_ptr() if out.shape[0] else None, stream)
        _native.check(rc, "pds_multistream_stack")


class _TickBatch:
    """What :class:`StreamBatch` and :class:`multistream_si.SiStreamBatch` share: the constructor, the public calls, the
    pools, the pinned staging and -- :func:`_tick` -- the one pipeline of a tick, ``compute_chunks`` and ``finalize``
    alike.  A subclass states what differs: `_computer_type` (and the ``TypeError`` message for another,
    `_wrong_computer`), :func:`_new_state` (its host state machine -- ``chunk_step``, ``commit_chunks``,
    ``finalize_step``, ``reset`` over a :class:`_StreamWords` -- and the row length of the carry pool),
    :func:`_emit_order` (which order the emitting streams launch in), `_launch_extra` (the keys of a step that follow
    offset, length, frame count and first row in the launch metadata, a row each) and :func:`_feature_launch`.  The
    post stages are `_stages`, :class:`_Stage` objects by name, built by the constructor in the order they run;
    `_tick` and `close` loop over it, and `dstate`, `cstate`, `wstate`, `kstate` and `estate` are the states of its
    members."""

    _computer_type = _wrong_computer = None
    _launch_extra = ()

    def __init__(self, computer, capacity: int = 4096, dtype=np.float32, deltas=None, preemphasis=None, cmvn=None,
                 cmvn_running=True, stack=None, dither=None, cepstra=None, sliding_cmvn=None, pcen=None, plp=None):
        # every argument is read before a device is touched
        if not isinstance(computer, self._computer_type):
            raise TypeError(self._wrong_computer)
        dtype = np.dtype(dtype)
        if dtype not in (np.float32, np.float64):
            raise TypeError("StreamBatch: samples must be float32 or float64")
        dspec, coeff = streaming_deltas(deltas), streaming_preemphasis(preemphasis)
        espec = streaming_pcen(pcen, computer)
        # the width the cmvn sees is the cepstral one with `cepstra` (whose bounds on the computer's width are checked
        # here, where it is known)
        pspec = streaming_cepstra(cepstra)
        if plp is not None and (pspec is not None or espec is not None):
            raise ValueError("StreamBatch: plp stands in cepstra's place and takes the linear energies themselves: "
                             "give it without cepstra and pcen")
        # ... and PLP's (its centre frequencies and its energy column are the computer's where it leaves them open)
        lspec = streaming_plp(plp, computer)
        width = computer.num_coeffs
        if pspec is not None:
            pspec._split(width)
            width = pspec.num_ceps
        if lspec is not None:
            width = lspec.num_ceps
        cspec = streaming_cmvn(cmvn, bool(cmvn_running), width)
        wspec = streaming_sliding_cmvn(sliding_cmvn)
        if cspec is not None and wspec is not None:
            raise ValueError("StreamBatch: cmvn and sliding_cmvn both normalise the statics: give one of them")
        kspec = streaming_stack(stack)
        nspec = streaming_dither(dither)
        self.state, row_length = self._new_state(computer, capacity)
        # the device side: `computer`'s plan, the carry pool of ``2 * capacity * row_length`` samples, the
        # previous-sample pool (with a pre-emphasis), the staging buffers and what the post stages keep
        torch = _native.require_device()
        self._torch = torch
        self._lib = _native.lib()
        self.dtype = dtype
        self.capacity = self.state.capacity
        self.device = torch.device("cuda", torch.cuda.current_device())
        self._comp = computer
        self._plan = computer._native_plan(self.device)
        self._tdtype = torch.float32 if dtype == np.float32 else torch.float64
        self._assemble = _typed(self._lib, "pds_multistream_assemble", dtype)
        self._tile = int(self._lib.pds_multistream_tile())
        self._row_length = int(row_length)
        self._pool = torch.zeros((2, self.capacity, self._row_length), dtype=self._tdtype, device=self.device)
        # every stream's previous raw sample, read from / written to the halves the carries are (none: no pool)
        self.preemphasis = coeff
        self._prev = torch.zeros((2, self.capacity), dtype=self._tdtype, device=self.device) if coeff else None
        self._format = _SAMPLES_F32 if dtype == np.float32 else _SAMPLES_F64
        # the dither: host state only (the noise is a function of position and key; the device keeps nothing for it)
        self.nstate = None
        self.dither = 0.0
        if nspec is not None:
            self.dither, base = nspec
            if base is None:
                base = int(np.random.SeedSequence().generate_state(1, np.uint64)[0] >> 1)
            self.nstate = DitherState(self.capacity, base)
        # pinned upload buffers (int64 words: samples, then metadata), used in turn; the event of a buffer's last
        # copy is waited for before it is written again
        self._up = [None, None]
        self._up_events = [None, None]
        self._up_next = 0
        self._down = None  # pinned features of the host-array calls
        # the post stages by name, in the order they run.  `_F0` is the computer's own width, which the feature launch
        # writes, `_F` the statics' as the post stages see them and `_C` the one before stacking
        self._F0, self._F = computer.num_coeffs, width
        self._stages = {}
        width = self._F0
        if cspec is not None:
            cspec += (bool(cmvn_running),)
        for name, kind, spec in (("pcen", _PcenStage, espec), ("cepstra", _CepstraStage, pspec),
                                 ("plp", _PlpStage, lspec), ("cmvn", _CmvnStage, cspec),
                                 ("sliding", _SlidingStage, wspec), ("deltas", _DeltasStage, dspec),
                                 ("stack", _StackStage, kspec)):
            if spec is not None:
                stage = self._stages[name] = kind(self, spec, width)
                width = stage.width
        self.num_coeffs = width
        self._C = self._stages["stack"].width_in if "stack" in self._stages else width
        states = {name: stage.state for name, stage in self._stages.items()}
        self.cstate, self.wstate, self.dstate, self.kstate = map(states.get, ("cmvn", "sliding", "deltas", "stack"))
        # what a tick asks of _tick_layout: a stage's sections are placed if it is there
        self._layout_flags = (*(flag in states for flag in ("deltas", "cmvn", "stack")), self.nstate is not None,
                              "sliding" in states)
        self.estate = states.get("pcen")
        if self.estate is not None:  # (a batch without the stage asks for the layout as it did before there was one)
            self._layout_flags += (True,)

    # ---- public interface -----------------------------------------------------------

    @property
    def lookahead(self) -> int:
        """frames of delay of the rows: ``num_deltas * context_window`` (0 without deltas)"""
        return self.dstate.H if self.dstate is not None else 0

    @property
    def num_vectors(self) -> int:
        """rows of a stream side by side in a returned row (1 without `stack`)"""
        return self.kstate.nv if self.kstate is not None else 1

    @property
    def dither_base(self) -> Optional[int]:
        """the seed of the first utterance this object began or will begin (None without `dither`): the ``Dither``'s
        seed, or the 63-bit value drawn at construction when it had none"""
        return self.nstate.base if self.nstate is not None else None

    def dither_seeds(self, ids) -> np.ndarray:
        """int64 per stream of `ids`: the seed of its current utterance -- ``Dither(coeff, seed=that).apply`` over the
        utterance's whole raw signal gives the samples its features are made of --, -1 for a stream that has not
        started"""
        self._check_open()
        if self.nstate is None:
            raise ValueError(f"{type(self).__name__} was built without dither")
        return self.nstate.seed[self.state.check_ids(ids)].copy()

    def started(self, ids) -> np.ndarray:
        """bool per stream of `ids`: between its first chunk and its ``finalize``"""
        self._check_open()
        return self.state.started[self.state.check_ids(ids)].copy()

    def cmvn_stats(self, ids) -> np.ndarray:
        """the current statistics of streams `ids` (with `cmvn`): host float64 ``[len(ids), 2, F + 1]``, each stream's
        table as ``Standardize`` keeps it (sums | count, sums of squares | unused) -- the prior, or zeros, for a stream
        at its start or after its ``finalize``, and for every stream under ``cmvn_running=False``.  Reads the device
        (one synchronisation) unless every stream is fresh"""
        self._check_open()
        if self.cstate is None:
            raise ValueError(f"{type(self).__name__} was built without cmvn")
        return self._stages["cmvn"].stats(self.state.check_ids(ids))

    def pcen_smooth(self, ids) -> np.ndarray:
        """the current smoother output M of streams `ids` (with `pcen`): host float64 ``[len(ids), F]``, the M of each
        stream's last static row; NaN rows for a stream that is fresh (at its start or after its ``finalize``).  Reads
        the device (one synchronisation) unless every stream is fresh"""
        self._check_open()
        if self.estate is None:
            raise ValueError(f"{type(self).__name__} was built without pcen")
        return self._stages["pcen"].smooth(self.state.check_ids(ids))

    def compute_chunks(self, ids, chunks: Sequence) -> List[np.ndarray]:
        """``compute_chunk`` of ``chunks[i]`` (1-D host array) for stream ``ids[i]``; returns the list of feature
        matrices in the order of `ids`"""
        self._check_open()
        ids = self.state.check_ids(ids)
        if len(chunks) != len(ids):
            raise ValueError("one chunk per stream id")
        arrs = [np.asarray(c) for c in chunks]
        if any(a.ndim != 1 for a in arrs):
            raise ValueError("chunks must be 1-dimensional")
        lengths = np.fromiter(map(len, arrs), dtype=np.int64, count=len(arrs))
        feats, rows = self._tick(ids, lengths, host_chunks=arrs)
        return self._to_host(feats, rows, np.ones(len(ids), dtype=bool))

    def compute_chunks_packed(self, ids, d_samples, lengths) -> Tuple[object, np.ndarray]:
        """``compute_chunk`` of chunks already on the GPU: `d_samples` holds them back to back (1-D contiguous tensor of
        this object's dtype, or of int16, on its device), ``lengths[i]`` samples for stream ``ids[i]``.  Returns
        ``(feats, rows)``: the ``(R, num_coeffs)`` GPU tensor and the host int64 ``len(ids) + 1`` row offsets of the
        streams in it"""
        self._check_open()
        torch = self._torch
        ids = self.state.check_ids(ids)
        lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        if len(lengths) != len(ids):
            raise ValueError("one length per stream id")
        if len(lengths) and lengths.min() < 0:
            raise ValueError("negative chunk length")
        if (not isinstance(d_samples, torch.Tensor) or d_samples.device != self.device or d_samples.dim() != 1
                or not d_samples.is_contiguous() or d_samples.dtype not in (self._tdtype, torch.int16)):
            raise ValueError(f"d_samples must be a contiguous 1-D {self.dtype} or int16 tensor on {self.device}")
        if int(lengths.sum()) > d_samples.numel():
            raise ValueError("the chunks lie outside d_samples")
        return self._tick(ids, lengths, d_samples=d_samples, i16=d_samples.dtype == torch.int16)

    def finalize(self, ids) -> List[np.ndarray]:
        """``finalize`` of streams `ids`: their last frames; the streams are reset and may be used again.  A stream
        that was not started gives ``(0, num_coeffs)`` float64 rows, as ``computer.finalize()`` does"""
        self._check_open()
        ids = self.state.check_ids(ids)
        started = self.state.started[ids].copy()
        feats, rows = self._tick(ids)
        return self._to_host(feats, rows, started)

    def finalize_packed(self, ids) -> Tuple[object, np.ndarray]:
        """:func:`finalize` with the features left on the GPU: ``(feats, rows)`` as :func:`compute_chunks_packed`"""
        self._check_open()
        return self._tick(self.state.check_ids(ids))

    def close(self) -> None:
        """Release the pools and the pinned buffers; the object cannot be used afterwards"""
        for stage in self._stages.values():
            stage.release()
        self._pool = self._prev = None
        self._up = [None, None]
        self._up_events = [None, None]
        self._down = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- a tick ---------------------------------------------------------------------

    def _check_open(self):
        if self._pool is None:
            raise ValueError(f"{type(self).__name__} is closed")

    def _staging(self, words: int):
        """the next pinned upload buffer (int64 numpy view of at least `words`), free to write"""
        torch = self._torch
        slot = self._up_next
        self._up_next ^= 1
        if self._up_events[slot] is not None:
            self._up_events[slot].synchronize()
        buf = self._up[slot]
        if buf is None or buf.numel() < words:
            size = 1 << 12
            while size < words:
                size <<= 1
            buf = self._up[slot] = torch.empty(size, dtype=torch.int64, pin_memory=True)
        return slot, buf

    def _send(self, slot: int, words: int, stream):
        """one copy of the first `words` of upload buffer `slot` to the device, on `stream`"""
        torch = self._torch
        dev = torch.empty(max(words, 1), dtype=torch.int64, device=self.device)
        if words:
            dev.copy_(self._up[slot][:words], non_blocking=True)
            ev = self._up_events[slot] = torch.cuda.Event()
            ev.record(stream)
        return dev

    def _pack_chunks(self, host, host_chunks, lengths, total):
        """the samples of a tick's host chunks (`total` > 0 of them) into the front of the pinned words `host`; returns
        the words they take and whether they went as 16-bit PCM"""
        # 16-bit PCM travels as it is, two bytes per sample, when the tick's non-empty chunks are all int16; else
        # the chunks are converted on their way into the buffer.  numpy checks the dtypes as it copies (no loop here)
        i16 = False
        ns = (total * self.dtype.itemsize + 7) // 8
        first = host_chunks[0] if len(host_chunks[0]) else host_chunks[int(np.argmax(lengths > 0))]
        if first.dtype == _I16:
            ns = (total * 2 + 7) // 8
            try:
                np.concatenate(host_chunks, out=host[:ns].view(_I16)[:total], casting="no")
                i16 = True
            except TypeError:  # another dtype: of empty chunks only?
                i16 = all(a.dtype == _I16 for a in host_chunks if len(a))
                if i16:
                    np.concatenate(host_chunks, out=host[:ns].view(_I16)[:total], casting="unsafe")
                else:
                    ns = (total * self.dtype.itemsize + 7) // 8
        if not i16:
            np.concatenate(host_chunks, out=host[:ns].view(self.dtype)[:total], casting="unsafe")
        return ns, i16

    def _tick(self, ids, lengths=None, host_chunks=None, d_samples=None, i16=False):
        """One tick over streams `ids`: ``compute_chunks`` of chunks of `lengths` -- `host_chunks`, or back to back in
        `d_samples` on the device, of int16 if `i16` --, over the work buffer an assemble launch packs of every
        stream's carry and chunk; without `lengths` ``finalize``, over the carries where they lie in the pool.  Returns
        ``(feats, rows)``: the tick's rows on the device and every stream's first row in them"""
        st = self.state
        final = lengths is None
        n = len(ids)
        # every stream's span of samples: `span` of them from `off` of what the feature launch reads
        if final:
            step = st.finalize_step(ids)
            span = step["carry_len"]
            off = (step["half"] * self.capacity + ids) * self._row_length
            total = ns = 0
        else:
            step = st.chunk_step(ids, lengths)
            span = step["avail"]
            work_off = _exclusive_cumsum(span)
            off = work_off[:-1]
            tile_prefix = _exclusive_cumsum((span + self._tile - 1) // self._tile)
            total = int(lengths.sum())
            ns = (total * self.dtype.itemsize + 7) // 8 if host_chunks is not None else 0
        k = step["k"]
        rows = _exclusive_cumsum(k)
        row0 = rows[:-1]
        order = self._emit_order(step, np.flatnonzero(k > 0))
        up = _Upload(ns, _tick_layout(n, len(order), 4 + len(self._launch_extra), not final, *self._layout_flags))
        slot, buf = self._staging(up.words)
        up.pinned = buf.numpy()
        if ns:
            # (the staging was sized for samples of `dtype`; a tick that travels as int16 takes fewer words)
            up.sample_words, i16 = self._pack_chunks(up.host("samples"), host_chunks, lengths, total)
        if not final:
            am = up.host("assemble")
            am[:, 0] = ids
            am[:, 1] = _exclusive_cumsum(lengths)[:-1]
            am[:, 2] = lengths
            am[:, 3] = step["carry_len"]
            am[:, 4] = step.get("drop", 0)  # (a short-integration stream drops nothing of a chunk)
            am[:, 5] = step["new_carry"]
            am[:, 6] = off
            am[:, 7] = step["word"]
            up.host("tiles")[:] = tile_prefix
            if self.nstate is not None:
                nstep = self.nstate.step(ids, lengths)
                self.nstate.fill_meta(up.host("dither"), nstep)
        lm = up.host("launch")
        lm[0], lm[1], lm[2], lm[3] = off[order], span[order], k[order], row0[order]
        for r, key in enumerate(self._launch_extra, 4):
            lm[r] = step[key][order]
        out_rows = rows  # every stream's first row in what the tick returns: the statics', through the stages
        for stage in self._stages.values():
            out_rows = stage.plan(up, ids, out_rows, final)
        stream = self._torch.cuda.current_stream(self.device)
        up.device = self._send(slot, up.words, stream)
        if final:
            signal = self._pool.view(-1)
        else:
            samples = up.dev("samples") if host_chunks is not None else d_samples
            signal = self._assemble_launch(samples if total else None, i16, up.dev("assemble"), up.dev("tiles"), n,
                                           int(tile_prefix[-1]), int(work_off[-1]), stream,
                                           up.dev("dither") if self.nstate is not None else None)
        feats = self._feature_launch(signal, up.dev("launch"), order, step, off, span, rows, stream)
        if final:
            st.reset(ids)
        else:
            st.commit_chunks(ids, step)
        if self.nstate is not None:
            if final:
                self.nstate.reset(ids)
            else:
                self.nstate.commit(ids, nstep)
        for stage in self._stages.values():
            feats = stage.launch(up, feats, ids, stream)
        return feats, out_rows

    def _assemble_launch(self, samples, i16, d_meta, d_tile_prefix, n, tiles, work_len, stream, d_dither=None):
        """one pds_multistream_assemble launch: the tick's work buffer (returned) and the new carries, in the other
        pool half; `samples`: the device tensor the chunks start in (only its address is used; None: no samples);
        `d_dither`: the positions and keys of a batch with `dither`"""
        torch = self._torch
        work = torch.empty(max(work_len, 1), dtype=self._tdtype, device=self.device)
        chunks = samples.data_ptr() if samples is not None else None
        if d_dither is not None:
            rc = self._lib.pds_multistream_assemble_dither(
                _SAMPLES_I16 if i16 else self._format, self._format, chunks, self._pool.data_ptr(), self.capacity,
                self._row_length, d_meta.data_ptr(), d_tile_prefix.data_ptr(), n, tiles, work.data_ptr(),
                self.preemphasis, self._prev.data_ptr() if self._prev is not None else None, d_dither.data_ptr(),
                self.dither, stream.cuda_stream)
        elif i16 or self._prev is not None:
            rc = self._lib.pds_multistream_assemble_pcm(
                _SAMPLES_I16 if i16 else self._format, self._format, chunks, self._pool.data_ptr(), self.capacity,
                self._row_length, d_meta.data_ptr(), d_tile_prefix.data_ptr(), n, tiles, work.data_ptr(),
                self.preemphasis, self._prev.data_ptr() if self._prev is not None else None, stream.cuda_stream)
        else:
            rc = self._assemble(chunks, self._pool.data_ptr(), self.capacity, self._row_length, d_meta.data_ptr(),
                                d_tile_prefix.data_ptr(), n, tiles, work.data_ptr(), stream.cuda_stream)
        _native.check(rc, "pds_multistream_assemble")
        return work

    def _to_host(self, feats, rows, started) -> List[np.ndarray]:
        """one download into pinned memory, one synchronisation, views per stream"""
        torch = self._torch
        R, C = feats.shape
        if R:
            if self._down is None or self._down.numel() < R * C:
                size = 1 << 16
                while size < R * C:
                    size <<= 1
                self._down = torch.empty(size, dtype=self._tdtype, pin_memory=True)
            pinned = self._down[: R * C].view(R, C)
            pinned.copy_(feats, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
            host = pinned.numpy().copy()
        else:
            host = np.empty((0, C), dtype=self.dtype)
        idle = np.empty((0, C), dtype=np.float64)
        return [host[a:b] if s else idle.copy() for a, b, s in zip(rows[:-1].tolist(), rows[1:].tolist(), started)]


class StreamBatch(_TickBatch):
    """``compute_chunk`` / ``finalize`` of many streams of one STFT computer, one tick per call

    `computer`: a :class:`ShortTimeFourierTransformFrameComputer` (its plan and configuration are used; its own
    streaming state is not touched).  `capacity`: number of streams, ids ``0 .. capacity - 1``.  `dtype`: sample type,
    float32 or float64, fixed here: the working and feature type.  Chunks of another dtype are converted with numpy's
    rules (int16 chunks on the GPU when a tick has no others).  Device memory: the carry pool,
    ``2 * capacity * frame_length`` samples.

    `preemphasis`: a coefficient, a :class:`pre.Preemphasize` (or what
    ``alias_factory_subclass_from_arg(PreProcessor, ...)`` makes one); ``None`` or ``0``: none.  Every stream's raw
    signal is pre-emphasised as ``Preemphasize.apply`` does it over the whole signal (float64 arithmetic, rounded to
    `dtype`; the first sample after a start or ``finalize`` unchanged), whatever the cuts.  Additional device memory:
    the previous-sample pool, ``2 * capacity`` elements of `dtype`.

    `deltas`: a :class:`post.Deltas` (or what ``alias_factory_subclass_from_arg(PostProcessor, ...)`` makes one) with
    ``pad_mode="edge"``, ``concatenate=True`` and the coefficient axis as target; ``None`` or ``num_deltas == 0``: no
    deltas.  With ``F = computer.num_coeffs``, ``K = num_deltas`` and ``H = K * context_window`` (:attr:`lookahead`)
    every stream's rows become ``[static, d_1 .. d_K]`` (``num_coeffs == (K + 1) * F``), equal bit for bit to
    ``deltas.apply(X, axis=0)`` of its concatenated statics X and delayed by H frames: when a stream has produced n
    static frames and been given e rows, a ``compute_chunks`` call returns ``max(0, n - H) - e`` rows and ``finalize``
    the last ``n - e``.  Additional device memory: the history pool, exactly ``2 * capacity * 2 * H * F`` elements of
    `dtype` (two halves of ``2 H`` static rows per stream), and per tick the ``(new rows, F)`` statics.

    `cmvn`: a :class:`post.Standardize` (or what ``alias_factory_subclass_from_arg(PostProcessor, ...)`` makes one:
    ``"cmvn"``, ``{"name": "cmvn", "rfilename": ...}``); ``None``: none.  With ``cmvn_running=True`` every stream's
    static rows are standardised by the statistics of the rows so far, this one included, on top of the statistics the
    ``Standardize`` holds, if any -- the reference's ``cmvn.accumulate(x); cmvn.apply(x)`` frame by frame, in float64,
    rounded to `dtype` once; with ``cmvn_running=False`` by the fixed statistics it holds, which it then must
    (``cmvn.apply(x)``).  The arithmetic, the first frame of zeros, NaN and the order with `deltas` (the deltas are
    those of the normalised statics) are in the module docstring; the reference's "0 variance" warning is not raised.
    The statistics' count must be a whole number.  ``finalize`` returns a stream to the statistics passed in;
    :func:`cmvn_stats` reads a stream's current ones.  The ``Standardize`` itself is not changed.  Additional device
    memory: the running sums, ``2 * capacity * F`` float64 (none with ``cmvn_running=False``).

    `stack`: a :class:`post.Stack` (or what ``alias_factory_subclass_from_arg(PostProcessor, ...)`` makes one:
    ``{"name": "stack", "num_vectors": 3}``) with the row axis as time axis (0 or -2) and ``pad_mode`` None, "edge" or
    "constant" (with at most a scalar ``constant_values``); ``None`` or ``num_vectors == 1``: no stacking.  The last
    stage: with C the row width after `cmvn` and `deltas` and ``nv = num_vectors`` (:attr:`num_vectors`) every stream's
    rows become those of ``stack.apply(X, axis=-1)`` over the sequence X of its rows without `stack`
    (``num_coeffs == nv * C``), bit for bit, groups running on across calls: when a stream holds r rows not yet
    returned and a call brings it m, ``compute_chunks`` returns ``(r + m) // nv`` rows and keeps ``(r + m) % nv``;
    ``finalize`` returns ``(r + m) // nv`` and drops the rest, or under a padding ``ceil((r + m) / nv)`` with the last
    group filled up.  The row offsets of the packed calls count stacked rows.  Additional device memory: the pool of
    pending rows, ``2 * capacity * (nv - 1) * C`` elements of `dtype`, and per tick the ``(new rows, C)`` rows before
    stacking.

    `cepstra`: a :class:`post.Cepstra` (or what ``alias_factory_subclass_from_arg(PostProcessor, ...)`` makes one:
    ``"mfcc"``, ``{"name": "mfcc", "num_ceps": 13}``); ``None``: none.  The first post stage: every static row becomes
    ``cepstra.apply(row)``, `num_ceps` wide, and `cmvn`, `deltas` and `stack` work on those rows (``F`` above is then
    `num_ceps`: the width of the cmvn statistics and of :func:`cmvn_stats`, of the deltas' history and of
    ``num_coeffs``), so a stream's rows are ``stack(deltas(cmvn(cepstra(statics))))`` of the offline objects over its
    whole utterance, bit for bit.  ``ValueError`` here if the computer's width does not admit `num_ceps`.  No state,
    no additional device memory, no change of a tick's upload; one more launch per tick that has rows.

    `sliding_cmvn`: a :class:`post.SlidingCMVN` (or what ``alias_factory_subclass_from_arg(PostProcessor, ...)`` makes
    one: ``{"name": "sliding_cmvn", "cmn_window": 600, "min_window": 1}``) with ``center=False`` and ``min_window=1``;
    ``None``: none.  It stands where `cmvn` stands (after `cepstra`, before `deltas` and `stack`; giving both is
    refused): every static row is normalised over the stream's last ``cmn_window + 1`` static rows, and a stream's rows
    are ``sliding_cmvn.apply(X)`` of its whole sequence of statics X, bit for bit (the module docstring has the
    arithmetic and why a centred window and ``min_window > 1`` are refused).  ``finalize`` returns a stream to fresh.
    Additional device memory: per stream a ring of ``cmn_window + 1`` rows of F elements of `dtype` and ``2 * F``
    float64 sums -- 96 KB per stream at ``cmn_window = 600``, ``F = 40`` and float32 (601 * 40 * 4 + 640 bytes), 394 MB
    at the default capacity of 4096: size `capacity` to the streams that are live.  A tick's upload grows by eight
    words per stream.

    `pcen`: a :class:`post.PCEN` (or what ``alias_factory_subclass_from_arg(PostProcessor, ...)`` makes one:
    ``"pcen"``, ``{"name": "pcen", "smooth": 0.025}``); ``None``: none.  The first post stage, before `cepstra`: every
    static row is normalised by the stream's per-column smoother and compressed, and a stream's rows are
    ``stack(deltas(cmvn(cepstra(pcen.apply(statics, axis=0)))))`` of the offline objects over its whole utterance, bit
    for bit.  PCEN takes linear energies: a computer built with ``use_log=True`` is a ``ValueError``.  Widths and
    :attr:`lookahead` do not change; ``finalize`` returns a stream to fresh; :func:`pcen_smooth` reads a stream's
    current M.  Additional device memory: ``capacity * F`` float64.  A tick's upload grows by two words and one byte
    per stream.

    `plp`: a :class:`post.PLP` (or what ``alias_factory_subclass_from_arg(PostProcessor, ...)`` makes one: ``"plp"``,
    ``{"name": "plp", "num_ceps": 13}``); ``None``: none.  It stands in `cepstra`'s place -- giving it together with
    `cepstra` or `pcen` is a ``ValueError`` -- and every static row becomes its `num_ceps` PLP cepstra, which `cmvn` /
    `sliding_cmvn`, `deltas` and `stack` work on: a stream's rows are ``stack(deltas(cmvn(plp.apply(statics))))`` of the
    offline objects over its whole utterance, bit for bit.  The object's centre frequencies and `energy` are taken from
    `computer` where it leaves them open; a computer built with ``use_log=True`` and a width the object refuses are
    ``ValueError`` s.  No additional device memory, no additional upload.

    `dither`: a :class:`pre.Dither` (or what ``alias_factory_subclass_from_arg(PreProcessor, ...)`` makes one:
    ``"dither"``, ``{"name": "dither", "coeff": 1.0, "seed": 5}``); ``None`` or a coefficient of 0: none.  Every
    stream's raw signal, converted to `dtype`, is dithered as ``Dither.apply`` does it over the whole signal, whatever
    the cuts, before the pre-emphasis if there is one.  The batch numbers the utterances it begins from 0 -- streams
    begin in tick order and within a tick in the order of `ids` --, and the n-th is dithered with seed
    ``dither_base + n`` (:attr:`dither_base`: the ``Dither``'s seed, which must lie in ``[0, 2**63)``, or a 63-bit value
    drawn at construction); ``finalize`` ends a stream's utterance, and its next chunk begins a new one.
    :func:`dither_seeds` returns the seeds of the streams' current utterances, so
    ``Dither(coeff, seed=sb.dither_seeds([i])[0]).apply(x)`` reproduces the samples offline.  The ``Dither`` itself is
    not changed.  No additional device memory; a tick's upload grows by two words per stream.

    Under ``config.FLOAT64_ARITHMETIC == "float32"`` float64 samples are rounded to float32 once in the work buffer
    (after a dither and a pre-emphasis, which work in float64) and the float32 features widened (within the float32 tolerance of
    the computer's path, not bit for bit); a `cmvn` then works on the widened features.
    """

    _computer_type = ShortTimeFourierTransformFrameComputer
    _wrong_computer = ("StreamBatch serves STFT frame computers (streaming short integration is not supported here: "
                       "multistream_si.SiStreamBatch serves those)")

    @staticmethod
    def _new_state(computer, capacity):
        return (StreamState(capacity, computer.frame_length, computer.frame_shift, computer.pad_left),
                computer.frame_length)

    @staticmethod
    def _emit_order(step, emit):
        """sorted by carry pad: the left reflection is launch-wide"""
        return emit[np.argsort(step["cp"][emit], kind="stable")]

    def _feature_launch(self, signal, d_lm, order, step, off, span, rows, stream):
        """the STFT batch launches of one tick (on the current stream, as the computer launches): streams `order`, one
        launch per distinct carry pad; `d_lm` is the device int64[4, len(order)] of their offsets, lengths, frame
        counts and rows"""
        torch = self._torch
        k, cp, R = step["k"], step["cp"], int(rows[-1])
        f32_arith = self.dtype == np.float64 and config.FLOAT64_ARITHMETIC == "float32"
        if f32_arith:
            signal = signal.to(torch.float32)
        feats = torch.empty((R, self._F0), dtype=torch.float32 if f32_arith else self._tdtype, device=self.device)
        if len(order):
            pads = cp[order]
            cuts = [0, *(np.flatnonzero(np.diff(pads)) + 1).tolist(), len(order)]
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                sel = order[lo:hi]
                # (rows go to the tick's order through d_meta[3]; host row_offsets only bound the output)
                layout = PackedLayout(B=hi - lo, extent=int((off[sel] + span[sel]).max()),
                                      nframes=k[sel], row_offsets=np.append(rows[:-1][sel], R), d_meta=d_lm[:, lo:hi])
                self._comp.launch(signal, layout, out=feats, pad_left=int(pads[lo]))
        return feats.to(self._tdtype) if f32_arith else feats
