"""Batched streaming for short-integration computers: ``compute_chunk`` / ``finalize`` of many streams per launch

:class:`multistream.StreamBatch` serves the STFT computer; :class:`SiStreamBatch` is its counterpart for
:class:`si.ShortIntegrationFrameComputer` (alias ``si``), with the same public surface:

    sb = SiStreamBatch(computer, capacity=4096)       # computer: a short-integration frame computer
    outs = sb.compute_chunks(ids, chunks)             # ids: distinct ints; chunks: 1-D arrays -> list of (k_i, C)
    outs = sb.finalize(ids)                           # the last frames; the streams are reset and may be reused
    feats, rows = sb.compute_chunks_packed(ids, d_samples, lengths)   # GPU in, GPU out
    sb.close()

    sb = SiStreamBatch(computer, capacity=4096, deltas=Deltas(2), preemphasis=0.97)   # as for StreamBatch
    sb = SiStreamBatch(computer, capacity=4096, cmvn=Standardize(), cmvn_running=True)  # as for StreamBatch
    sb = SiStreamBatch(computer, capacity=4096, stack=Stack(3))                         # as for StreamBatch
    sb = SiStreamBatch(computer, capacity=4096, dither=Dither(1.0, seed=5))             # as for StreamBatch

Every stream gets, call by call, what a private copy of `computer` returns from ``compute_chunk`` / ``finalize`` for
the same chunks: the same row counts, dtype and -- for float32 and float64 samples alike -- the same values bit for
bit.  That holds by construction: a stream's work span of a tick (carried samples, then the chunk) is exactly the
private computer's kept tail after its concatenation, the kernel's `start` and the frame count are the same numbers,
and positions outside ``[0, length)`` read as zero in both, so the direct kernel and the overlap-save transforms see
identical inputs at identical alignment; neither's arithmetic depends on how many utterances or frames a call has.
Which streams a tick names, and in which order, changes no stream's result.  Chunks of 16-bit PCM (int16) give the
values of the same chunks converted to `dtype` first (the single-stream computer refuses integer chunks; the batch
takes them as ``StreamBatch`` does).  With `deltas` a stream's rows are ``Deltas.apply`` of its whole sequence of
statics, delayed by :attr:`SiStreamBatch.lookahead` frames; with `preemphasis` they are those of the pre-emphasised
whole signal; both bit for bit, as documented in :mod:`multistream`.  With `cmvn` (a :class:`post.Standardize`) every
static row is standardised as it is produced: running (``cmvn_running=True``), the reference's ``cmvn.accumulate(x);
cmvn.apply(x)`` frame by frame -- cumulative mean and variance normalisation, on top of the statistics passed in, if
any -- or global (``cmvn_running=False``), ``cmvn.apply(x)`` with those fixed statistics; float64, bit for bit, rounded
to `dtype` once; a stream's first frame without a prior is a row of zeros, a NaN stays in its stream's sums until the
``finalize``, the reference's "0 variance" warning is not raised, and deltas are taken of the normalised statics.  The
arithmetic is spelled out in :mod:`multistream`.  With `stack` (a :class:`post.Stack`) every ``num_vectors`` consecutive
rows of a stream, after `cmvn` and `deltas`, are returned side by side as one, groups running on across ticks: the
stream's rows are ``stack.apply`` of its rows without `stack`, bit for bit, as documented in :mod:`multistream`.

A tick: :class:`SiStreamState` -- the array form of ``si.py``'s ``compute_chunk`` / ``_emit`` / ``finalize``
bookkeeping -- is advanced on the host, which fixes every size without reading the device; samples and metadata go up
in one copy from pinned memory; one ``pds_multistream_assemble_*`` launch writes the tick's packed work buffer (carry
+ chunk of every stream) and the new carries into the other pool half; one ``pds_si_batch_starts_*`` call computes
the frames of every stream that has any, each continued at its own `start` (float32: the plan's overlap-save form
when it has one, else direct filtering; float64: direct filtering -- the choices the single-stream computer makes);
optionally one ``pds_multistream_cmvn_*`` launch, one ``pds_multistream_deltas_*`` launch and one
``pds_multistream_stack_*`` launch, in that order; one download.  ``finalize`` reads the carries where they lie in the
pool.  The pipeline is :func:`multistream._TickBatch._tick`, shared with ``StreamBatch``; this module adds the state,
the tick order of the emitting streams, the `start` row of the launch metadata and the ``pds_si_batch_starts_*`` call.

The per-utterance start is what makes one call enough.  A stream's `start` is ``skip0 - lead + done * S - tail_at``:
the position of its next frame's first integrated sample, relative to the first sample it still keeps.  Once
``keep_from = skip0 - lead + done * S - (M - 1)`` has passed 0 the kept tail starts there and `start` is ``M - 1`` for
every stream; before that -- the stream's first ``M - 1`` or so samples -- ``tail_at`` is 0 and `start` grows with
``done``, so streams begun at different times differ.

The carried tail is bounded: ``carry_len < max(M - 1, skip0) + 2 S`` (``M`` the longest support, ``S`` the frame shift).
After any call ``waiting < 2 S`` (a call emits ``waiting // S - 1`` frames), and with ``P`` samples received so far
``P = waiting + skip0 - lead + done * S`` once the skip is consumed.  While no frame has been emitted ``tail_at`` is 0
and the tail is everything: ``P < skip0`` under a pending skip, else ``P < skip0 + 2 S`` (``lead > 0`` only with
``skip0 == 0``).  After an emission ``tail_at = max(0, keep_from)``, so ``P - tail_at <= P - keep_from = waiting + M - 1
< M - 1 + 2 S``.  That bound is the pool's row length, and :func:`SiStreamState.chunk_step` asserts it.

Not thread-safe; works on the current torch stream of the device that was current at construction.
"""
import numpy as np

from . import _native
from .compute import _MAX_UTTS_PER_CALL
from .multistream import _StreamWords, _TickBatch
from .si import ShortIntegrationFrameComputer

__all__ = ["SiStreamBatch", "SiStreamState"]


class SiStreamState(_StreamWords):
    """Host bookkeeping of many short-integration streams: ``si.py``'s ``_reset_stream`` / ``compute_chunk`` / ``_emit``
    / ``finalize`` applied to arrays of streams.  Needs no device.

    Geometry (one computer's): `frame_shift` S, `max_support` M, `translation`, `skip0` samples consumed before
    integration starts, `lead` virtual zeros in front (at most one of the two is positive), `centered` frames.

    Per stream: ``done`` frames emitted, ``waiting`` integrated samples received but not yet framed, ``skip_left`` of the
    skip still pending, ``tail_at`` stream position of the first kept sample, ``carry_len`` kept samples (always
    < :attr:`row_length`), and ``started``, ``has_sample`` and ``half`` as :class:`multistream.StreamState` has them.
    """

    def __init__(self, capacity: int, frame_shift: int, max_support: int, translation: int, skip0: int, lead: int,
                 centered: bool):
        super().__init__(capacity)
        capacity = self.capacity
        self.S, self.M, self.translation = int(frame_shift), int(max_support), int(translation)
        self.skip0, self.lead, self.centered = int(skip0), int(lead), bool(centered)
        if self.S < 1 or self.M < 1 or self.skip0 < 0 or self.lead < 0 or (self.skip0 and self.lead):
            raise ValueError("not the geometry of a short-integration computer")
        self.frame_length = self.M + self.S - 1
        # carry_len < row_length always (module docstring); the row length of the carry pool
        self.row_length = max(self.M - 1, self.skip0) + 2 * self.S
        self.done = np.zeros(capacity, dtype=np.int64)
        self.waiting = np.zeros(capacity, dtype=np.int64)
        self.skip_left = np.zeros(capacity, dtype=np.int64)
        self.tail_at = np.zeros(capacity, dtype=np.int64)
        self.carry_len = np.zeros(capacity, dtype=np.int64)

    @classmethod
    def of(cls, computer: ShortIntegrationFrameComputer, capacity: int) -> "SiStreamState":
        """the state of `capacity` streams of `computer`"""
        return cls(capacity, computer.frame_shift, computer._max_support, computer._translation, computer._skip0,
                   computer._lead, computer.frame_style == "centered")

    def _start(self, done, tail_at):
        """the kernel's `start` for a span that begins at stream position `tail_at`, continued at frame `done`"""
        return self.skip0 - self.lead + done * self.S - tail_at

    def chunk_step(self, ids: np.ndarray, lengths: np.ndarray) -> dict:
        """What ``compute_chunk`` of chunks of `lengths` does to streams `ids`, without changing the state: per stream
        the carry (`carry_len`), the work span `avail` = carry + chunk (nothing of a chunk is dropped: skipped samples
        stay in the tail until ``keep_from`` passes them), its frame count `k`, the kernel's `start` for the span, where
        the new carry starts in the span (`new_carry`: ``keep_from - tail_at``, 0 when no frame is emitted) and the new
        state (``commit_chunks`` applies it)"""
        S = self.S
        lengths = np.asarray(lengths, dtype=np.int64)
        fresh = ~self.started[ids]  # the first chunk since the start or a finalize
        skip_left = np.where(fresh, self.skip0, self.skip_left[ids])
        waiting = np.where(fresh, self.lead, self.waiting[ids])
        done, tail_at, c, word = self.done[ids], self.tail_at[ids], self.carry_len[ids], self.word[ids]
        consumed = np.minimum(skip_left, lengths)
        skip_left = skip_left - consumed
        waiting = waiting + lengths - consumed
        avail = c + lengths
        k = np.maximum(0, waiting // S - 1)
        next_done = done + k
        # samples before the first one the next frame's filters can reach are no longer needed (only a call that
        # emits trims: _emit returns before that when it has no frame)
        keep_from = np.where(k > 0, np.maximum(tail_at, self._start(next_done, 0) - (self.M - 1)), tail_at)
        new_carry = keep_from - tail_at
        step = dict(
            carry_len=c, avail=avail, k=k, start=self._start(done, tail_at), new_carry=new_carry,
            next_done=next_done, next_waiting=waiting - k * S, next_skip_left=skip_left, next_tail_at=keep_from,
            next_carry_len=avail - new_carry,
            word=word, next_word=self.next_word(word, lengths),
        )
        assert (new_carry >= 0).all() and (new_carry <= avail).all()
        assert (step["next_carry_len"] < self.row_length).all()
        return step

    def commit_chunks(self, ids: np.ndarray, step: dict) -> None:
        self.done[ids] = step["next_done"]
        self.waiting[ids] = step["next_waiting"]
        self.skip_left[ids] = step["next_skip_left"]
        self.tail_at[ids] = step["next_tail_at"]
        self.carry_len[ids] = step["next_carry_len"]
        self.started[ids] = True
        # (the assemble kernel wrote the new carries and previous samples to the other half)
        self.word[ids] = step["next_word"]

    def tail_frames(self, waiting: np.ndarray, skip_left: np.ndarray) -> np.ndarray:
        """``ShortIntegrationFrameComputer._tail_frames`` over arrays: frames ``finalize`` adds"""
        S = self.S
        borrowed = S if self.centered else 0
        buf_len = self.translation - skip_left + waiting - borrowed
        want = np.maximum(0, (buf_len + S // 2) // S)
        pad_right = (want - 1) * S + self.frame_length - buf_len
        pad_raw = pad_right - np.minimum(skip_left, pad_right)
        return np.where(want < 1, 0, np.minimum(want, np.maximum(0, (waiting + pad_raw) // S - 1))).astype(np.int64)

    def finalize_step(self, ids: np.ndarray) -> dict:
        """What ``finalize`` does: frames `k` from the carry (`carry_len` samples in pool `half`) at `start`; none for
        a stream that was not started"""
        started = self.started[ids]
        k = np.where(started, self.tail_frames(self.waiting[ids], self.skip_left[ids]), 0)
        return dict(carry_len=self.carry_len[ids], k=k, start=self._start(self.done[ids], self.tail_at[ids]),
                    half=self.word[ids] & 1)

    def reset(self, ids: np.ndarray) -> None:
        self.done[ids] = 0
        self.waiting[ids] = 0
        self.skip_left[ids] = 0
        self.tail_at[ids] = 0
        self.carry_len[ids] = 0
        self.started[ids] = False
        self.word[ids] &= 1


class SiStreamBatch(_TickBatch):
    """``compute_chunk`` / ``finalize`` of many streams of one short-integration computer, one tick per call

    `computer`: a :class:`si.ShortIntegrationFrameComputer` (its plan and configuration are used; its own streaming
    state is not touched).  `capacity`, `dtype`, `deltas`, `preemphasis`, `cmvn`, `cmvn_running`, `stack`, `dither`, `cepstra`,
    `sliding_cmvn` (sliding-window CMVN in the place of `cmvn`; its ring of ``cmn_window + 1`` rows per stream is added
    to the device memory below), `pcen` (per-channel energy normalisation as the first post stage, for a computer with
    ``use_log=False``; ``capacity * F`` float64 more), `plp` (PLP cepstra in `cepstra`'s place, for a computer with
    ``use_log=False``; no device memory of its own) and every method (``cmvn_stats`` and ``dither_seeds`` among them): as :class:`multistream.StreamBatch` -- with `dither`
    every stream's raw signal is dithered across ticks, before the pre-emphasis; with `cmvn` the static rows are
    standardised frame by frame, running or by fixed statistics, before the deltas are taken, and with `stack` the rows
    are stacked last.  Device memory: the carry pool, ``2 * capacity * row_length`` samples with
    ``row_length = max(max_support - 1, skip0) + 2 * frame_shift`` (:attr:`SiStreamState.row_length`), plus what
    `deltas`, `preemphasis`, `cmvn` (the running sums, ``2 * capacity * F`` float64) and `stack` (the pending rows) add
    there, and per tick the work buffer and, for float32 with the overlap-save form, its
    scratch (``pds_si_scratch_len`` of the tick's streams and its largest frame count).
    """

    _computer_type = ShortIntegrationFrameComputer
    _wrong_computer = ("SiStreamBatch serves short-integration frame computers (multistream.StreamBatch serves STFT "
                       "ones)")
    _launch_extra = ("start",)

    @staticmethod
    def _new_state(computer, capacity):
        state = SiStreamState.of(computer, capacity)
        return state, state.row_length

    @staticmethod
    def _emit_order(step, emit):
        return emit  # (tick order: every stream brings its own start)

    def _feature_launch(self, signal, d_lm, order, step, off, span, rows, stream):
        """the frames of a tick: one pds_si_batch_starts call over streams `order`; `d_lm` is the device
        int64[5, len(order)] of their offsets in `signal`, lengths, frame counts, first rows and starts; more than one
        call only beyond the utterances a call takes"""
        torch = self._torch
        lib = self._lib
        f64 = self.dtype == np.float64
        batch = lib.pds_si_batch_starts_f64 if f64 else lib.pds_si_batch_starts_f32
        feats = torch.empty((int(rows[-1]), self._F0), dtype=self._tdtype, device=self.device)
        k = step["k"][order]
        E = len(k)
        for lo in range(0, E, _MAX_UTTS_PER_CALL):
            hi = min(E, lo + _MAX_UTTS_PER_CALL)
            most = int(k[lo:hi].max())
            at, row = d_lm.data_ptr() + 8 * lo, 8 * d_lm.stride(0)  # (int64[5, E], a row per argument)
            args = (self._plan.handle, signal.data_ptr()) + tuple(at + r * row for r in range(5)) + (hi - lo, most)
            if f64:
                rc = batch(*args, feats.data_ptr(), feats.stride(0), stream.cuda_stream)
            else:
                # the overlap-save form when the plan has it (it needs scratch memory), else direct filtering: the
                # choice of ShortIntegrationFrameComputer._launch
                need = int(lib.pds_si_scratch_len(self._plan.handle, hi - lo, most))
                scratch = torch.empty(need, dtype=torch.float32, device=self.device) if need else None
                rc = batch(*args, scratch.data_ptr() if need else None, feats.data_ptr(), feats.stride(0),
                           stream.cuda_stream)
            _native.check(rc, "pds_si_batch_starts")
        return feats
