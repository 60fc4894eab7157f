"""ctypes binding of the package's shared libraries: ``libpds_amd.so`` (C ABI: ``include/pds_amd.h``) and the
stages libraries ``libpds_amd_stages*.so``, each a capped library of stage kernels outside the fused kernel's
instantiation matrix with a header (``include/pds_amd_stages*.h``) and an error string of its own.  Every one of them
is a :class:`Library`; ``LIBRARIES`` lists them.

There is deliberately no fallback: if a shared library is missing or a compute call
is made without a HIP device, an exception is raised.  Nothing in this package computes
features on the CPU.
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_int32, c_int64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))

PDS_OK = 0


class NativeError(RuntimeError):
    """A call into libpds_amd.so failed"""


class StftDesc(Structure):
    # mirrors pds_stft_desc (include/pds_amd.h)
    _fields_ = [
        ("frame_length", c_int32),
        ("frame_shift", c_int32),
        ("dft_size", c_int32),
        ("pad_left", c_int32),
        ("num_filts", c_int32),
        ("nnz", c_int32),
        ("use_power", c_int32),
        ("use_log", c_int32),
        ("include_energy", c_int32),
        ("reserved", c_int32),
        ("log_floor", c_double),
    ]


class SiDesc(Structure):
    # mirrors pds_si_desc (include/pds_amd.h)
    _fields_ = [
        ("frame_shift", c_int32),
        ("max_support", c_int32),
        ("num_coeffs", c_int32),
        ("taps_complex", c_int32),
        ("use_power", c_int32),
        ("use_log", c_int32),
        ("reserved", c_int32),
        ("reserved2", c_int32),
        ("log_floor", c_double),
    ]


_SI_BATCH_ARGS = [
    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int64,
    c_void_p, c_int64, c_void_p,
]

_BATCH_ARGS = [
    c_void_p,  # plan
    c_void_p,  # d_signal
    c_void_p,  # d_offsets
    c_void_p,  # d_lengths
    c_void_p,  # d_nframes
    c_void_p,  # d_row_off
    c_int32,  # B
    c_int64,  # max_frames
    c_int32,  # pad_left
    c_double,  # preemph
    c_void_p,  # d_out
    c_int64,  # out_stride
    c_void_p,  # stream
]

_DELTAS_ARGS = [
    c_void_p, c_int64, c_int64, c_int64,  # d_in, outer, time, inner
    c_void_p, c_void_p, c_int32,  # d_filts, d_filt_off, K
    c_int32, c_int32,  # edge_clamp, max_off
    c_void_p, c_int64, c_int64, c_int64, c_int64,  # d_out, sk, so, st, si
    c_void_p,  # stream
]

_CMVN_ROWS_ARGS = [
    c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int32, c_int32,
    c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
]

# name -> (restype, argtypes); every symbol include/pds_amd.h declares
SIGNATURES = {
    "pds_version": (c_int32, []),
    "pds_build_experiments": (c_int32, []),
    "pds_last_error": (c_char_p, []),
    "pds_device_count": (c_int32, []),
    "pds_stft_plan_create": (
        c_int32,
        [POINTER(StftDesc), c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_void_p)],
    ),
    "pds_stft_plan_destroy": (None, [c_void_p]),
    "pds_stft_num_coeffs": (c_int32, [c_void_p]),
    "pds_stft_num_frames": (c_int64, [c_void_p, c_int64]),
    "pds_stft_plan_kernel_kind": (c_int32, [c_void_p]),
    "pds_stft_plan_filter_walk": (c_int32, [c_void_p]),
    "pds_stft_plan_geometry": (c_int32, [c_void_p, POINTER(c_int32)]),
    "pds_stft_batch_f32": (c_int32, _BATCH_ARGS),
    "pds_stft_batch_f64": (c_int32, _BATCH_ARGS),
    "pds_stft_batch_f32_generic": (c_int32, _BATCH_ARGS),
    "pds_stft_plan_has_f64in": (c_int32, [c_void_p]),
    "pds_stft_plan_has_fused_deltas": (c_int32, [c_void_p]),
    "pds_stft_plan_has_fused_cmvn": (c_int32, [c_void_p]),
    "pds_stft_cmvn_partials_len": (c_int64, [c_void_p, c_int32]),
    "pds_stft_prepare_chunk_prefix": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "pds_stft_cmvn_batch_f32": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_int32, c_void_p,
         c_int32, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int64, c_void_p, c_void_p],
    ),
    "pds_stft_deltas_batch": (
        c_int32,
        [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_double,
         c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_void_p],
    ),
    "pds_stft_deltas_batch_f32": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int32,
         c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p],
    ),
    "pds_stft_batch_f64in": (c_int32, _BATCH_ARGS[:11] + [c_int32] + _BATCH_ARGS[11:]),
    "pds_stft_plan_has_i16in": (c_int32, [c_void_p]),
    "pds_stft_batch_i16in": (c_int32, _BATCH_ARGS),
    "pds_stft_batch_ragged_f32": (c_int32, _BATCH_ARGS[:10] + [c_void_p] + _BATCH_ARGS[10:]),
    "pds_stft_batch_ragged_i16in": (c_int32, _BATCH_ARGS[:10] + [c_void_p] + _BATCH_ARGS[10:]),
    "pds_preemphasize_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_double, c_void_p, c_void_p]),
    "pds_preemphasize_f64": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_double, c_void_p, c_void_p]),
    "pds_dither_f32": (c_int32, [c_void_p, c_int64, c_double, ctypes.c_uint64, c_void_p, c_void_p]),
    "pds_dither_f64": (c_int32, [c_void_p, c_int64, c_double, ctypes.c_uint64, c_void_p, c_void_p]),
    "pds_dither_packed_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_double, c_void_p, c_void_p]),
    "pds_dither_packed_f64": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_double, c_void_p, c_void_p]),
    "pds_dither_packed_i16_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_double, c_void_p, c_void_p]),
    "pds_deltas_f32": (c_int32, _DELTAS_ARGS),
    "pds_deltas_f64": (c_int32, _DELTAS_ARGS),
    "pds_deltas_rows_f32": (
        c_int32,
        [c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_void_p,
         c_void_p, c_int32, c_int32, c_void_p, c_int64, c_void_p],
    ),
    "pds_stack_rows_f32": (
        c_int32,
        [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_int32,
         c_int32, c_void_p, c_int64, c_void_p],
    ),
    "pds_cepstra_rows_f32": (
        c_int32, [c_void_p, c_int64, c_int64, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_int64, c_void_p]),
    "pds_cepstra_rows_f64": (
        c_int32, [c_void_p, c_int64, c_int64, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_int64, c_void_p]),
    "pds_si_plan_create": (c_int32, [POINTER(SiDesc), c_void_p, c_void_p, POINTER(c_void_p)]),
    "pds_si_plan_destroy": (None, [c_void_p]),
    "pds_si_scratch_len": (c_int64, [c_void_p, c_int32, c_int64]),
    "pds_si_plan_fft_size": (c_int32, [c_void_p]),
    "pds_si_launch_shape": (c_int32, [c_void_p, c_int32, c_int64, c_int32, POINTER(c_int32)]),
    "pds_si_batch_f32": (c_int32, _SI_BATCH_ARGS[:9] + [c_void_p] + _SI_BATCH_ARGS[9:]),
    "pds_si_batch_f64": (c_int32, _SI_BATCH_ARGS),
    # ... with d_starts (one start per utterance) behind d_row_off and no scalar start
    "pds_si_batch_starts_f32": (c_int32, _SI_BATCH_ARGS[:6] + [c_void_p] + _SI_BATCH_ARGS[6:8] + [c_void_p]
                                + _SI_BATCH_ARGS[9:]),
    "pds_si_batch_starts_f64": (c_int32, _SI_BATCH_ARGS[:6] + [c_void_p] + _SI_BATCH_ARGS[6:8] + _SI_BATCH_ARGS[9:]),
    "pds_cmvn_scratch_len": (c_int64, [c_int64, c_int64]),
    "pds_cmvn_stats_f32": (c_int32, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "pds_cmvn_stats_f64": (c_int32, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "pds_cmvn_apply_f32": (c_int32, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pds_cmvn_apply_f64": (c_int32, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pds_cmvn_rows_f32": (c_int32, _CMVN_ROWS_ARGS),
    "pds_cmvn_rows_f32out": (c_int32, _CMVN_ROWS_ARGS),
    # host feed (pinned staging ring: upload / kernel / download of consecutive batches overlap)
    "pds_feed_create": (c_int32, [c_void_p, c_int32, c_int64, c_int32, c_int32, c_int32, POINTER(c_void_p)]),
    "pds_feed_destroy": (None, [c_void_p]),
    "pds_feed_slot_rows": (c_int64, [c_void_p]),
    "pds_feed_set_direct": (c_int32, [c_void_p, c_int32]),
    "pds_feed_acquire": (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_void_p)]),
    "pds_feed_pack": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32]),
    "pds_feed_submit": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_double, c_int32]),
    "pds_feed_submit_frames": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_double, c_int32]),
    "pds_feed_device_view": (c_int32, [c_void_p, c_int32, POINTER(c_void_p), POINTER(c_int64), POINTER(c_void_p),
                                       POINTER(c_void_p)]),
    "pds_feed_download": (c_int32, [c_void_p, c_int32, c_void_p, c_int64]),
    "pds_feed_collect": (c_int32, [c_void_p, c_int32, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_int64)]),
    "pds_feed_unpack": (c_int32, [c_void_p, c_int32, c_void_p, c_int64, c_int32]),
    "pds_feed_release": (c_int32, [c_void_p, c_int32]),
    # batched streaming (multistream.py)
    "pds_multistream_tile": (c_int32, []),
    "pds_multistream_assemble_f32": (
        c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_int32, c_int64, c_void_p, c_void_p]),
    "pds_multistream_assemble_f64": (
        c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_int32, c_int64, c_void_p, c_void_p]),
    "pds_multistream_assemble_pcm": (
        c_int32, [c_int32, c_int32, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_int32, c_int64, c_void_p,
                  c_double, c_void_p, c_void_p]),
    "pds_multistream_assemble_dither": (
        c_int32, [c_int32, c_int32, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_int32, c_int64, c_void_p,
                  c_double, c_void_p, c_void_p, c_double, c_void_p]),
    "pds_multistream_deltas_f32": (
        c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32,
                  c_int64, c_void_p, c_void_p]),
    "pds_multistream_deltas_f64": (
        c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32,
                  c_int64, c_void_p, c_void_p]),
    "pds_multistream_cmvn_f32": (
        c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_void_p]),
    "pds_multistream_cmvn_f64": (
        c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_void_p]),
    "pds_multistream_stack_f32": (
        c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_double,
                  c_void_p, c_void_p]),
    "pds_multistream_stack_f64": (
        c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_double,
                  c_void_p, c_void_p]),
    # multi-GPU gather over RCCL
    "pds_comm_unique_id": (c_int32, [c_void_p]),
    "pds_comm_init_rank": (c_int32, [c_void_p, c_int32, c_int32, POINTER(c_void_p)]),
    "pds_comm_init_all": (c_int32, [c_int32, c_void_p, POINTER(c_void_p)]),
    "pds_comm_world": (c_int32, [c_void_p]),
    "pds_comm_rank": (c_int32, [c_void_p]),
    "pds_comm_destroy": (None, [c_void_p]),
    "pds_comm_group_start": (c_int32, []),
    "pds_comm_group_end": (c_int32, []),
    "pds_gather_rows": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "pds_allreduce_sum_f64": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p]),
}

_SLIDING_ROWS_ARGS = [
    c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int64, c_int32,  # d_in, in_stride, d_row_off, d_nrows, B, max_rows, C
    c_int32, c_int32, c_int32, c_int32, c_int32,  # cmn_window, min_window, center, norm_vars, refresh
    c_void_p, c_int64, c_void_p,  # d_out, out_stride, stream
]
_MS_SLIDING_ARGS = [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32,
                    c_void_p]
_RESAMPLE_PACKED_ARGS = [
    c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64,  # d_in, d_in_off, d_in_len, d_out_off, B, max_len
    c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,  # in_unit, out_unit, max_taps, d_first, d_ntaps, d_weights
    c_void_p, c_void_p,  # d_out, stream
]
_MS_RESAMPLE_ARGS = [
    c_void_p, c_void_p, c_int64,  # d_samples, d_hist, capacity
    c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,  # in_unit, out_unit, max_taps, d_first, d_ntaps, d_weights
    c_void_p, c_int32, c_void_p, c_void_p,  # d_meta, n, d_out, stream
]
_VAD_ENERGY_ARGS = [
    c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int64,  # d_energy, stride, d_row_off, d_nrows, B, max_rows
    c_double, c_double, c_int32, c_double,  # energy_threshold, energy_mean_scale, frames_context, proportion_threshold
    c_void_p, c_void_p, c_void_p,  # d_voiced, d_count, stream
]
_SELECT_ROWS_ARGS = [
    c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_int32, c_int64,  # d_in, in_stride, words, d_row_off, d_nrows, B, max_rows
    c_void_p, c_void_p, c_void_p, c_int64, c_void_p,  # d_keep, d_out_row_off, d_out, out_stride, stream
]

# name -> (restype, argtypes); every symbol include/pds_amd_stages.h declares
STAGES_SIGNATURES = {
    "pds_stages_version": (c_int32, []),
    "pds_stages_last_error": (c_char_p, []),
    "pds_sliding_cmvn_rows_f32": (c_int32, _SLIDING_ROWS_ARGS),
    "pds_sliding_cmvn_rows_f64": (c_int32, _SLIDING_ROWS_ARGS),
    "pds_multistream_sliding_f32": (c_int32, _MS_SLIDING_ARGS),
    "pds_multistream_sliding_f64": (c_int32, _MS_SLIDING_ARGS),
    "pds_resample_packed_f32": (c_int32, _RESAMPLE_PACKED_ARGS),
    "pds_resample_packed_f64": (c_int32, _RESAMPLE_PACKED_ARGS),
    "pds_resample_packed_i16_f32": (c_int32, _RESAMPLE_PACKED_ARGS),
    "pds_multistream_resample_f32": (c_int32, _MS_RESAMPLE_ARGS),
    "pds_multistream_resample_f64": (c_int32, _MS_RESAMPLE_ARGS),
    "pds_multistream_resample_i16_f32": (c_int32, _MS_RESAMPLE_ARGS),
    "pds_vad_energy_rows_f32": (c_int32, _VAD_ENERGY_ARGS),
    "pds_vad_energy_rows_f64": (c_int32, _VAD_ENERGY_ARGS),
    "pds_select_rows_w32": (c_int32, _SELECT_ROWS_ARGS),
}

_PCEN_SMOOTH_ARGS = [
    c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int32,  # d_in, in_stride, d_row_off, d_nrows, B, C
    c_double, c_double, c_void_p, c_int64, c_void_p,  # smooth, oms, d_m, m_stride, stream
]
_PCEN_COMPRESS_ARGS = [
    c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32,  # d_in, in_stride, d_m, m_stride, rows, C
    c_double, c_double, c_double, c_double, c_double,  # gain, bias, power, eps, bp
    c_void_p, c_int64, c_void_p,  # d_out, out_stride, stream
]
_MS_PCEN_ARGS = [
    c_void_p, c_void_p, c_int64, c_int32,  # d_statics, d_state, capacity, C
    c_double, c_double, c_double, c_double, c_double, c_double, c_double,  # smooth, oms, gain, bias, power, eps, bp
    c_void_p, c_void_p, c_void_p, c_int32, c_void_p,  # d_ids, d_rows, d_fresh, n, stream
]

# name -> (restype, argtypes); every symbol include/pds_amd_stages2.h declares
STAGES2_SIGNATURES = {
    "pds_stages2_version": (c_int32, []),
    "pds_stages2_last_error": (c_char_p, []),
    "pds_pcen_smooth_rows_f32": (c_int32, _PCEN_SMOOTH_ARGS),
    "pds_pcen_smooth_rows_f64": (c_int32, _PCEN_SMOOTH_ARGS),
    "pds_pcen_compress_rows_f32": (c_int32, _PCEN_COMPRESS_ARGS),
    "pds_pcen_compress_rows_f64": (c_int32, _PCEN_COMPRESS_ARGS),
    "pds_multistream_pcen_f32": (c_int32, _MS_PCEN_ARGS),
    "pds_multistream_pcen_f64": (c_int32, _MS_PCEN_ARGS),
}

_SPECAUG_MEAN_ARGS = [
    c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p,  # d_in, in_stride, d_row_off, d_nrows, B, C, d_mean, stream
]
_SPECAUG_APPLY_ARGS = [
    c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int32,  # d_in, in_stride, d_row_off, d_nrows, B, C
    c_void_p, c_int32, c_int32, c_void_p, c_double,  # d_plan, freq_masks, time_masks, d_mean_or_null, fill
    c_void_p, c_int64, c_int64, c_void_p,  # d_out, out_stride, max_rows, stream
]

# name -> (restype, argtypes); every symbol include/pds_amd_stages3.h declares
STAGES3_SIGNATURES = {
    "pds_stages3_version": (c_int32, []),
    "pds_stages3_last_error": (c_char_p, []),
    "pds_specaug_tile_rows": (c_int32, []),
    "pds_specaug_plan": (
        c_int32,
        [c_void_p, c_void_p, c_int32, c_int32,  # d_nrows, d_keys, B, C
         c_int32, c_int64, c_int32, c_int64, c_double, c_int64,  # freq_masks, freq_width, time_masks, time_width, time_ratio, warp
         c_void_p, c_void_p],  # d_plan, stream
    ),
    "pds_specaug_mean_rows_f32": (c_int32, _SPECAUG_MEAN_ARGS),
    "pds_specaug_mean_rows_f64": (c_int32, _SPECAUG_MEAN_ARGS),
    "pds_specaug_apply_rows_f32": (c_int32, _SPECAUG_APPLY_ARGS),
    "pds_specaug_apply_rows_f64": (c_int32, _SPECAUG_APPLY_ARGS),
}

_PLP_ROWS_ARGS = [
    c_void_p, c_int64, c_int64, c_int32, c_int32,  # d_in, in_stride, R, F, copy
    c_void_p, c_void_p, c_void_p, c_int32, c_int32,  # d_w, d_B, d_L, p, K
    c_double, c_double, c_void_p, c_int64, c_void_p, c_void_p,  # compress_factor, floor, d_out, out_stride, d_aux_or_null, stream
]

# name -> (restype, argtypes); every symbol include/pds_amd_stages4.h declares
STAGES4_SIGNATURES = {
    "pds_stages4_version": (c_int32, []),
    "pds_stages4_last_error": (c_char_p, []),
    "pds_plp_block_rows": (c_int32, []),
    "pds_plp_lds_bytes": (c_int64, [c_int32]),
    "pds_plp_rows_f32": (c_int32, _PLP_ROWS_ARGS),
    "pds_plp_rows_f64": (c_int32, _PLP_ROWS_ARGS),
}

_MIX_ENERGY_ARGS = [
    c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_void_p, c_void_p,  # d_x, d_off, d_len, d_chunk_base, B, total_chunks, d_partials, stream
]
_MIX_APPLY_ARGS = [
    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,  # d_x, d_off, d_len, d_bank, d_clip_off, d_clip_len, d_start
    c_void_p, c_int32, c_int64, c_void_p, c_void_p,  # d_gain, B, max_len, d_out, stream
]

# name -> (restype, argtypes); every symbol include/pds_amd_stages5.h declares
STAGES5_SIGNATURES = {
    "pds_stages5_version": (c_int32, []),
    "pds_stages5_last_error": (c_char_p, []),
    "pds_mix_chunk_samples": (c_int64, []),
    "pds_mix_chunk_count": (c_int64, [c_int64]),
    "pds_mix_tile_samples": (c_int64, []),
    "pds_mix_chunk_energy_f32": (c_int32, _MIX_ENERGY_ARGS),
    "pds_mix_chunk_energy_f64": (c_int32, _MIX_ENERGY_ARGS),
    "pds_mix_chunk_energy_i16": (c_int32, _MIX_ENERGY_ARGS),
    "pds_mix_gain": (
        c_int32,
        [c_void_p, c_void_p, c_void_p, c_int32, c_int32,  # d_partials, d_chunk_base, d_len, B, mode
         c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p],  # d_clip, d_ratio, d_applied, d_pn, K, d_out, stream
    ),
}
STAGES5_SIGNATURES.update({f"pds_mix_apply_{x}_{z}": (c_int32, _MIX_APPLY_ARGS)
                           for x in ("f32", "f64", "i16") for z in ("f32", "f64", "i16")})

_REVERB_SPECTRA_ARGS = [
    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64,  # d_x, d_off, d_len, d_rir, d_spec_base, B, total_units
    c_void_p, c_void_p, c_void_p,  # d_twiddle, d_workspace, stream
]

# name -> (restype, argtypes); every symbol include/pds_amd_stages6.h declares
STAGES6_SIGNATURES = {
    "pds_stages6_version": (c_int32, []),
    "pds_stages6_last_error": (c_char_p, []),
    "pds_reverb_block_samples": (c_int64, []),
    "pds_reverb_max_taps": (c_int64, []),
    "pds_reverb_partitions": (c_int64, [c_int64]),
    "pds_reverb_spectra_units": (c_int64, [c_int64]),
    "pds_reverb_convolve_units": (c_int64, [c_int64, c_int64, c_int32]),
    "pds_reverb_workspace_bytes": (c_int64, [c_int64]),
    "pds_reverb_twiddles": (c_int32, [c_void_p]),
    "pds_reverb_spectra_f32": (c_int32, _REVERB_SPECTRA_ARGS),
    "pds_reverb_spectra_f64": (c_int32, _REVERB_SPECTRA_ARGS),
    "pds_reverb_spectra_i16": (c_int32, _REVERB_SPECTRA_ARGS),
    "pds_reverb_convolve": (
        c_int32,
        [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64,  # d_x, xtype, d_off, d_len, d_rir, d_spec_base, d_unit_base, B, total_units
         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,  # d_workspace, d_h, d_rir_base, d_rir_parts, d_rir_peak, d_rir_tap, d_rir_gain, K
         c_void_p, c_void_p, c_void_p],  # d_twiddle, d_out, stream
    ),
    "pds_reverb_scale": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_void_p]),  # d_out, d_off, d_len, d_gain, B, max_len, stream
}


class Library:
    """One shared library: its path (from ``variable`` in the environment, which selects another build of the same
    library, or else ``default``), its ``name -> (restype, argtypes)`` table, the symbol that returns its own error
    string, and the exceptions of its return codes (``-1`` is a ``ValueError`` everywhere; any code without an entry is
    a :class:`NativeError` that names it).  Calling the object gives the loaded library."""

    def __init__(self, variable, default, signatures, last_error, errors=()):
        self.variable = variable
        self.path = os.environ.get(variable) or default
        self.signatures = signatures
        self.errors = {-1: ValueError, **dict(errors)}
        self._last_error = last_error
        self._handle = None

    def __call__(self) -> ctypes.CDLL:
        """The loaded library; raises :class:`NativeError` if it has not been built"""
        if self._handle is None:
            if not os.path.exists(self.path):
                raise NativeError(
                    f"{self.path} is missing: build it with `python -c 'import __graft_entry__ as g; "
                    "g.build()'` or `make -C pydrobert-speech_amd/csrc` (there is no CPU fallback)"
                )
            # torch's HIP runtime first where torch is installed: the library's own dependency on libamdhip64
            # then resolves to the copy already in the process (loaded the other way round, the two runtimes
            # disagree about the devices)
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
            loaded = ctypes.CDLL(self.path)
            for name, (restype, argtypes) in self.signatures.items():
                fn = getattr(loaded, name)  # AttributeError if the .so is stale
                fn.restype = restype
                fn.argtypes = argtypes
            self._handle = loaded
        return self._handle

    def last_error(self) -> str:
        return getattr(self(), self._last_error)().decode("utf-8", "replace")

    def check(self, rc: int, what: str) -> None:
        """Raises the exception of a return code other than ``PDS_OK``, with the library's own error string"""
        if rc != PDS_OK:
            msg = self.last_error()
            if rc in self.errors:
                raise self.errors[rc](f"{what}: {msg}")
            raise NativeError(f"{what}: {msg} (code {rc})")


_CSRC = os.path.join(_HERE, "csrc")
lib = Library("PDS_AMD_LIB", os.path.join(_CSRC, "libpds_amd.so"), SIGNATURES, "pds_last_error", {-3: MemoryError})
# the first stages library is looked for in csrc/ wherever PDS_AMD_LIB points, the later ones beside the first library,
# so that PDS_AMD_LIB moves them with it: an asymmetry that integrators rely on by now
_BESIDE = os.path.dirname(lib.path)
stages_lib = Library("PDS_AMD_STAGES_LIB", os.path.join(_CSRC, "libpds_amd_stages.so"), STAGES_SIGNATURES,
                     "pds_stages_last_error")
stages2_lib = Library("PDS_AMD_STAGES2_LIB", os.path.join(_BESIDE, "libpds_amd_stages2.so"), STAGES2_SIGNATURES,
                      "pds_stages2_last_error")
stages3_lib = Library("PDS_AMD_STAGES3_LIB", os.path.join(_BESIDE, "libpds_amd_stages3.so"), STAGES3_SIGNATURES,
                      "pds_stages3_last_error")
stages4_lib = Library("PDS_AMD_STAGES4_LIB", os.path.join(_BESIDE, "libpds_amd_stages4.so"), STAGES4_SIGNATURES,
                      "pds_stages4_last_error")
stages5_lib = Library("PDS_AMD_STAGES5_LIB", os.path.join(_BESIDE, "libpds_amd_stages5.so"), STAGES5_SIGNATURES,
                      "pds_stages5_last_error")
stages6_lib = Library("PDS_AMD_STAGES6_LIB", os.path.join(_BESIDE, "libpds_amd_stages6.so"), STAGES6_SIGNATURES,
                      "pds_stages6_last_error")
LIBRARIES = (lib, stages_lib, stages2_lib, stages3_lib, stages4_lib, stages5_lib, stages6_lib)
(LIB_PATH, STAGES_LIB_PATH, STAGES2_LIB_PATH, STAGES3_LIB_PATH, STAGES4_LIB_PATH, STAGES5_LIB_PATH,
 STAGES6_LIB_PATH) = (library.path for library in LIBRARIES)
(check, check_stages, check_stages2, check_stages3, check_stages4, check_stages5,
 check_stages6) = (library.check for library in LIBRARIES)
last_error = lib.last_error


def require_device():
    """torch with a visible HIP device, or an exception -- never a CPU path"""
    import torch

    if not torch.cuda.is_available():
        raise NativeError(
            "no HIP device is visible: this package computes features on an MI355X only "
            "(no CPU fallback); the CPU restatement in oracle/ is test infrastructure"
        )
    return torch
