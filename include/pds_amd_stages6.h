/* C ABI of libpds_amd_stages6.so: the sixth capped library of stage kernels for gfx950 (AMD Instinct MI355X).
 * libpds_amd_stages.so is full, libpds_amd_stages2.so holds the PCEN kernels and no other, libpds_amd_stages3.so the
 * SpecAugment kernels, libpds_amd_stages4.so the PLP kernels and libpds_amd_stages5.so the noise-mixing kernels
 * (DESIGN.md sections 4.3 and 4.9 to 4.13); the rule is one capped library per family of stage kernels, 64 KiB of device
 * code each, none of them a home for the fused STFT kernel's instantiations.  This one has its own size cap, its own
 * version and its own error string.  It shares no state and no header with the other six libraries and may be loaded
 * with or without them.
 *
 * Conventions as in pds_amd.h: every pointer named d_* is device memory of the current HIP device; `stream` is a
 * hipStream_t (NULL: the default stream); calls are asynchronous on it; a return value other than 0 leaves a message
 * for the calling thread in the string the last-error call returns.  There is no CPU path. */
#ifndef PDS_AMD_STAGES6_H
#define PDS_AMD_STAGES6_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDS_STAGES6_OK 0
#define PDS_STAGES6_ERR_INVALID -1 /* bad argument */
#define PDS_STAGES6_ERR_HIP -2     /* a HIP runtime call failed */

/* 100 * major + minor of this library; independent of the other six */
int32_t pds_stages6_version(void);
/* the calling thread's message of its last failed call into this library ("" before any) */
const char *pds_stages6_last_error(void);

/* ---------------------------------------------------------------------------------
 * Room impulse response convolution over packed utterances, modelled on Kaldi's wav-reverberate --impulse-response
 * --shift-output --normalize-output; pre.Reverb.
 *
 * The definition.
 *
 * Bank:
 *
 * - `K` room impulse responses (RIRs), each one channel of `1 ≤ L_j ≤ 2²⁰` taps, float32, float64 or int16.
 * - Partition size is `B = 512` taps and transform size is `N = 1024`, so `P_j = ceil(L_j / 512)`.
 * - The partition spectra are built on the host in float64: `H_{j,p} = fft(taps[512p : 512p+512]` zero-padded to
 *   1024`)`. Each spectrum is rounded once to complex64, uploaded once per device and cached.
 * - The peak is `d_j = ` the first index of `max |h_j[k]|` when `shift_output` is set, else `0`. The taps are compared
 *   as float64.
 *
 * Plan of utterance `b`, built on the host in integers and float64:
 *
 * - One Philox4x32-10 block: key = the utterance's 64-bit key from `pre.dither_keys` (low word, high word), counter =
 *   `(0, 0, 0, 0x52495231)`. The fourth word differs from `dither_noise.h`, `specaug_rule.h` and `mix_rule.h`.
 * - RIR `j = (uint64(x0) · K) >> 32`.
 * - `applied = float64(x3) · 2⁻³² < prob`.
 *
 * Wet signal, float32 whatever the sample dtype:
 *
 * - With `x` zero outside `[0, n)`, `y_full[τ] = Σ_k h[k]·x[τ−k]` and `wet[t] = y_full[t + d]` for `0 ≤ t < n`. The
 *   reverberant tail past the last sample is dropped.
 * - It is evaluated by uniformly partitioned overlap-save in float32. The blocks of `y_full` stand on multiples of 512
 *   of `τ`, anchored at the utterance's own first sample, not at the buffer's.
 * - float64 samples are rounded to float32 at the load. int16 samples are widened.
 * - A RIR with exactly one non-zero tap `g` at `k0` is a delay and a gain. No transform is taken:
 *   `wet[t] = float32(g)·x[t + d − k0]`, one float32 product, `+0.0` where `t + d − k0` lies outside `[0, n)`. A unit
 *   impulse therefore returns the samples as loaded.
 * - Independence: an utterance's wet bytes depend on its samples, the RIR and the parameters alone, not on the batch it
 *   stands in, its offset in the buffer (aligned or not), its neighbours or the launch. The summation order over `p` is
 *   fixed and there are no atomics.
 * - Locality: take `τ` in the block beginning at `b0 = 512·floor(τ/512)`. `wet` at `τ − d` depends, round-off
 *   included, only on input samples `b0 − 512·(P+2) ≤ i < b0 + 1536`. Two adjacent real blocks are packed into one
 *   complex transform: `ifft(fft(a + i·b)·H) = a⊛h + i·(b⊛h)`. Where that window holds no non-zero sample, the output
 *   is exactly `±0.0`.
 *
 * Normalisation (`normalize_output`):
 *
 * - `Ps` is the mean power of the utterance's samples in their own dtype, `Py` that of the float32 wet signal. Both are
 *   the segment energy `E(·, n) / n` of `pds_amd_stages5.h`: the same chunks, lanes and tree.
 * - If `Ps > 0` and `Py > 0`, then `out[t] = float32(float64(wet[t]) · c)` with `c = sqrt(Ps / Py)`. The quotient, the
 *   root and the product are each rounded by themselves.
 * - Otherwise the wet signal stands as it is. The comparisons are false for NaN.
 *
 * Not applied: a float32 utterance is copied byte for byte, with NaN payloads and signed zeros intact. int16 is widened.
 * float64 is rounded once.
 *
 * Gaps and bad samples:
 *
 * - Float32 samples outside every utterance keep their bytes. For int16 and float64 input only the utterance spans are
 *   defined.
 * - A NaN or infinite sample spoils only the outputs whose window holds it. With `normalize_output` it spoils its own
 *   utterance's scale. It never spoils another utterance.
 *
 * The form.  Block k of y_full covers tau in [512 k, 512 k + 512); blocks 2 m and 2 m + 1 are pair m.  Spectrum k of an
 * utterance, k = -1 .. floor((n - 1) / 512) + 1, is the transform of z[s] = x[512 (k - 1) + s] + i x[512 k + s],
 * 0 <= s < 1024, and lies in slot k + 1 of the utterance's part of the workspace, bin 32 q + l at complex index
 * 32 q + l (natural order).  Pair m, k = 2 m, is the sum over p of Z_{k - p} H_p for the p in 0 .. P - 1 whose spectrum
 * exists, ascending, one inverse transform, elements 512 .. 1023 scaled by 2^-10: the real part is block k, the
 * imaginary part block k + 1.  A unit is the work of half a wave: one spectrum, one pair, or 1024 samples of a copied
 * utterance; an utterance's units are rounded up to an even count.
 *
 * pds_reverb_block_samples: 512.  pds_reverb_partitions: P of L taps, -1 (and a
 * message) for L < 1 or L > 2^20.  pds_reverb_spectra_units: the spectra slots (and
 * spectra-kernel units) of an applied utterance of n samples.  pds_reverb_convolve_units: the convolve-kernel units of
 * an utterance of n samples with peak d, transformed (applied, and more than one non-zero tap) or not.  pds_reverb_workspace_bytes: the bytes of a workspace of
 * `units` slots (8192 each), -1 where the count needs more than 2^31 - 1 blocks.  pds_reverb_twiddles: fills a host
 * array of 1024 complex64 (2048 floats) with W_1024^(q l) at [q * 32 + l], formed in float64; the caller uploads it.
 *
 * pds_reverb_spectra_*: the spectra of B utterances of d_x, utterance b being d_x[d_off[b] .. d_off[b] + d_len[b]).
 * d_rir[b] is the utterance's RIR or -1 where it is not transformed; d_spec_base[b] the slots of the utterances before b
 * (ascending; an utterance that is not transformed has none) and total_units that of all B.
 *
 * pds_reverb_convolve: writes every utterance's span of d_out (float32): the wet signal where d_rir[b] is in [0, K), a
 * copy of the samples (xtype 0 float32, 1 float64, 2 int16) elsewhere.  d_unit_base[b] counts the convolve units of the
 * utterances before b, total_units all of them.  d_h holds the partition spectra, RIR j's at slots d_rir_base[j] ..
 * d_rir_base[j] + d_rir_parts[j] - 1 of 1024 complex64; d_rir_peak[j] is d_j; d_rir_tap[j] is k0 where RIR j has exactly
 * one non-zero tap (d_rir_gain[j] is that tap as float32), else -1.  Here d_rir[b] is the RIR of every applied utterance.
 * d_workspace may be null where no utterance is transformed (total_units of the spectra call was 0).
 *
 * pds_reverb_scale: d_out[t] = float(double(d_out[t]) * d_gain[b]) over utterance b's span, B <= 65535 utterances a
 * call, none longer than max_len; a gain that is exactly 0.0 leaves the utterance.
 *
 * Argument errors return PDS_STAGES6_ERR_INVALID before any HIP call: a negative size, more than 2^31 - 1 blocks, more
 * than 65535 utterances in one scale call, an xtype outside 0..2, null pointers.  B == 0 (and total_units == 0, and
 * max_len == 0) returns 0 without looking at the pointers.
 * --------------------------------------------------------------------------------- */
int64_t pds_reverb_block_samples(void);
int64_t pds_reverb_max_taps(void);
int64_t pds_reverb_partitions(int64_t L);
int64_t pds_reverb_spectra_units(int64_t n);
int64_t pds_reverb_convolve_units(int64_t n, int64_t d, int32_t transformed);
int64_t pds_reverb_workspace_bytes(int64_t units);
int32_t pds_reverb_twiddles(float *host_out);

int32_t pds_reverb_spectra_f32(const float *d_x, const int64_t *d_off, const int64_t *d_len, const int64_t *d_rir,
                               const int64_t *d_spec_base, int32_t B, int64_t total_units, const float *d_twiddle,
                               float *d_workspace, void *stream);
int32_t pds_reverb_spectra_f64(const double *d_x, const int64_t *d_off, const int64_t *d_len, const int64_t *d_rir,
                               const int64_t *d_spec_base, int32_t B, int64_t total_units, const float *d_twiddle,
                               float *d_workspace, void *stream);
int32_t pds_reverb_spectra_i16(const int16_t *d_x, const int64_t *d_off, const int64_t *d_len, const int64_t *d_rir,
                               const int64_t *d_spec_base, int32_t B, int64_t total_units, const float *d_twiddle,
                               float *d_workspace, void *stream);

int32_t pds_reverb_convolve(const void *d_x, int32_t xtype, const int64_t *d_off, const int64_t *d_len,
                            const int64_t *d_rir, const int64_t *d_spec_base, const int64_t *d_unit_base, int32_t B,
                            int64_t total_units, const float *d_workspace, const float *d_h, const int64_t *d_rir_base,
                            const int64_t *d_rir_parts, const int64_t *d_rir_peak, const int64_t *d_rir_tap,
                            const float *d_rir_gain, int32_t K, const float *d_twiddle, float *d_out, void *stream);

int32_t pds_reverb_scale(float *d_out, const int64_t *d_off, const int64_t *d_len, const double *d_gain, int32_t B,
                         int64_t max_len, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PDS_AMD_STAGES6_H */
