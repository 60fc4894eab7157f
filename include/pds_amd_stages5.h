/* C ABI of libpds_amd_stages5.so: the fifth capped library of stage kernels for gfx950 (AMD Instinct MI355X).
 * libpds_amd_stages.so is full, libpds_amd_stages2.so holds the PCEN kernels and no other, libpds_amd_stages3.so the
 * SpecAugment kernels and no other and libpds_amd_stages4.so the PLP kernels and no other (DESIGN.md sections 4.3 and
 * 4.9 to 4.12); the rule is one capped library per family of stage kernels, 64 KiB of device code each, none of them a
 * home for the fused STFT kernel's instantiations.  This one has its own size cap, its own version and its own error
 * string.  It shares no state and no header with the other five libraries and may be loaded with or without them.
 *
 * Conventions as in pds_amd.h: every pointer named d_* is device memory of the current HIP device; `stream` is a
 * hipStream_t (NULL: the default stream); calls are asynchronous on it; a return value other than 0 leaves a message
 * for the calling thread in the string the last-error call returns.  There is no CPU path. */
#ifndef PDS_AMD_STAGES5_H
#define PDS_AMD_STAGES5_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDS_STAGES5_OK 0
#define PDS_STAGES5_ERR_INVALID -1 /* bad argument */
#define PDS_STAGES5_ERR_HIP -2     /* a HIP runtime call failed */

/* 100 * major + minor of this library; independent of the other five */
int32_t pds_stages5_version(void);
/* the calling thread's message of its last failed call into this library ("" before any) */
const char *pds_stages5_last_error(void);

/* ---------------------------------------------------------------------------------
 * Noise mixing at a drawn signal-to-noise ratio over packed utterances, modelled on Kaldi's wav-reverberate
 * --additive-signals --snrs; pre.AddNoise.
 *
 * The definition.
 *
 * Segment energy `E(x, n)` of `n` samples, float64:
 *
 * - Chunk `c` covers samples `[c·16384, min(n, (c+1)·16384))`.
 * - In a chunk, lane `l` of 64 starts at `p_l = +0.0`. For `i = l, l+64, …` inside the chunk, in that order, it takes
 *   `v = float64(x[i])` and `p_l = p_l + v·v`. The product is rounded by itself, and it is exact for float32 and int16
 *   samples.
 * - The chunk sum is the fixed tree: for `s = 32, 16, 8, 4, 2, 1`, `p_l = p_l + p_{l+s}` for all `l < s`. The result
 *   is `p_0`.
 * - `E` starts at `+0.0` and takes the chunk sums in ascending order.
 * - `E(x, 0) = 0.0`.
 * - Mean power is `P = E / float64(n)` for `n > 0`, else `0.0`.
 *
 * Plan of utterance `b`, built on the host in integers and float64:
 *
 * - One Philox4x32-10 block: key = the utterance's 64-bit key (low word, high word, as `dither_noise.h` splits it),
 *   counter = `(0, 0, 0, 0x4D495831)`. `dither_noise.h` and `specaug_rule.h` leave the fourth counter word zero, so
 *   this counter differs from every one of theirs.
 * - Output words `x0..x3`, with `K` clips and `L_j` the length of clip `j`:
 *   - clip `j = (uint64(x0) · K) >> 32`
 *   - start `s = (uint64(x1) · L_j) >> 32`
 *   - `snr = lo + (hi − lo) · (float64(x2) · 2⁻³²)`, each operation rounded by itself. It is exactly `lo` when
 *     `lo == hi`.
 *   - `applied = float64(x3) · 2⁻³² < prob`
 *   - ratio `r = math.pow(10.0, snr / 10.0)`, one scalar call per utterance.
 *
 * Gain, on the device, float64, one lane per utterance:
 *
 * - `Ps` is the mean power of the utterance's samples. `Pn` is that of the whole clip `j`.
 * - If `applied`, `Ps > 0` and `Pn > 0`, then `g = sqrt(Ps / (Pn · r))`. The product, the quotient and the root are
 *   each rounded by itself.
 * - Otherwise `g = 0.0`. The comparisons are false for NaN.
 *
 * Mix:
 *
 * - For `0 ≤ t < n`: `y[t] = T(float64(x[t]) + g · float64(z[o_j + ((s + t) mod L_j)]))`. `z` is the noise bank;
 *   `o_j` and `L_j` are clip `j`'s offset and length in it. Product and sum are rounded separately, and there is one
 *   rounding to `T`.
 * - `T` is float32 for float32 and int16 signals, and float64 for float64 signals.
 * - When `g` is exactly `0.0` the utterance is copied. Float input goes byte for byte. int16 is widened.
 * - A clip shorter than the utterance wraps as often as needed.
 * - Float samples outside every utterance keep their values. For int16 input only the utterance spans are defined.
 * - `+inf` anywhere is only promised not to disturb other utterances.
 *
 * pds_mix_chunk_samples: the samples of a chunk (16384).  pds_mix_chunk_count: the chunks of a segment of n samples
 * (0 for n <= 0).  pds_mix_tile_samples: the samples a block of the apply kernel covers.
 *
 * pds_mix_chunk_energy_*: the chunk sums of B segments of d_x, segment b being d_x[d_off[b] .. d_off[b] + d_len[b]).
 * d_chunk_base[b] is the number of chunks of the segments before b (ascending, d_chunk_base[0] = 0) and total_chunks
 * that of all B; chunk c of segment b goes to d_partials[d_chunk_base[b] + c].  One wave per chunk; the same call
 * serves utterances and the clips of a bank.
 *
 * pds_mix_gain: one lane per segment adds its chunk sums in order.  mode 0 writes E to d_out[b], mode 1 the mean
 * power P (what finishes a bank's Pn), mode 2 the gain g from P, d_pn[d_clip[b]] (K clips; a clip outside [0, K)
 * gives 0.0), d_ratio[b] and d_applied[b] != 0.  d_clip, d_ratio, d_applied and d_pn are looked at in mode 2 only.
 *
 * pds_mix_apply_<x>_<z>: the mix for a signal of type x (f32, f64, i16) and a bank of type z, B <= 65535 utterances a
 * call, none longer than max_len.  d_out has the signal's length; its type is float for f32 and i16 signals, double
 * for f64 signals.  Utterance b reads clip d_clip_off[b], d_clip_len[b] of d_bank from d_start[b] (reduced modulo the
 * length; a length below 1 copies the utterance) with gain d_gain[b].  Samples outside every utterance are not written.
 *
 * Argument errors return PDS_STAGES5_ERR_INVALID before any HIP call: a negative size, more than 65535 utterances in
 * one apply call, more than 2^31 - 1 blocks, a mode outside 0..2, null pointers.  B == 0 (and total_chunks == 0, and
 * max_len == 0) returns 0 without looking at the pointers.
 * --------------------------------------------------------------------------------- */
int64_t pds_mix_chunk_samples(void);
int64_t pds_mix_chunk_count(int64_t n);
int64_t pds_mix_tile_samples(void);

int32_t pds_mix_chunk_energy_f32(const float *d_x, const int64_t *d_off, const int64_t *d_len,
                                 const int64_t *d_chunk_base, int32_t B, int64_t total_chunks, double *d_partials,
                                 void *stream);
int32_t pds_mix_chunk_energy_f64(const double *d_x, const int64_t *d_off, const int64_t *d_len,
                                 const int64_t *d_chunk_base, int32_t B, int64_t total_chunks, double *d_partials,
                                 void *stream);
int32_t pds_mix_chunk_energy_i16(const int16_t *d_x, const int64_t *d_off, const int64_t *d_len,
                                 const int64_t *d_chunk_base, int32_t B, int64_t total_chunks, double *d_partials,
                                 void *stream);

int32_t pds_mix_gain(const double *d_partials, const int64_t *d_chunk_base, const int64_t *d_len, int32_t B,
                     int32_t mode, const int64_t *d_clip, const double *d_ratio, const int64_t *d_applied,
                     const double *d_pn, int32_t K, double *d_out, void *stream);

int32_t pds_mix_apply_f32_f32(const float *d_x, const int64_t *d_off, const int64_t *d_len, const float *d_bank,
                              const int64_t *d_clip_off, const int64_t *d_clip_len, const int64_t *d_start,
                              const double *d_gain, int32_t B, int64_t max_len, float *d_out, void *stream);
int32_t pds_mix_apply_f32_f64(const float *d_x, const int64_t *d_off, const int64_t *d_len, const double *d_bank,
                              const int64_t *d_clip_off, const int64_t *d_clip_len, const int64_t *d_start,
                              const double *d_gain, int32_t B, int64_t max_len, float *d_out, void *stream);
int32_t pds_mix_apply_f32_i16(const float *d_x, const int64_t *d_off, const int64_t *d_len, const int16_t *d_bank,
                              const int64_t *d_clip_off, const int64_t *d_clip_len, const int64_t *d_start,
                              const double *d_gain, int32_t B, int64_t max_len, float *d_out, void *stream);
int32_t pds_mix_apply_f64_f32(const double *d_x, const int64_t *d_off, const int64_t *d_len, const float *d_bank,
                              const int64_t *d_clip_off, const int64_t *d_clip_len, const int64_t *d_start,
                              const double *d_gain, int32_t B, int64_t max_len, double *d_out, void *stream);
int32_t pds_mix_apply_f64_f64(const double *d_x, const int64_t *d_off, const int64_t *d_len, const double *d_bank,
                              const int64_t *d_clip_off, const int64_t *d_clip_len, const int64_t *d_start,
                              const double *d_gain, int32_t B, int64_t max_len, double *d_out, void *stream);
int32_t pds_mix_apply_f64_i16(const double *d_x, const int64_t *d_off, const int64_t *d_len, const int16_t *d_bank,
                              const int64_t *d_clip_off, const int64_t *d_clip_len, const int64_t *d_start,
                              const double *d_gain, int32_t B, int64_t max_len, double *d_out, void *stream);
int32_t pds_mix_apply_i16_f32(const int16_t *d_x, const int64_t *d_off, const int64_t *d_len, const float *d_bank,
                              const int64_t *d_clip_off, const int64_t *d_clip_len, const int64_t *d_start,
                              const double *d_gain, int32_t B, int64_t max_len, float *d_out, void *stream);
int32_t pds_mix_apply_i16_f64(const int16_t *d_x, const int64_t *d_off, const int64_t *d_len, const double *d_bank,
                              const int64_t *d_clip_off, const int64_t *d_clip_len, const int64_t *d_start,
                              const double *d_gain, int32_t B, int64_t max_len, float *d_out, void *stream);
int32_t pds_mix_apply_i16_i16(const int16_t *d_x, const int64_t *d_off, const int64_t *d_len, const int16_t *d_bank,
                              const int64_t *d_clip_off, const int64_t *d_clip_len, const int64_t *d_start,
                              const double *d_gain, int32_t B, int64_t max_len, float *d_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PDS_AMD_STAGES5_H */
