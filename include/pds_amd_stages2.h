/* C ABI of libpds_amd_stages2.so: the second capped library of stage kernels for gfx950 (AMD Instinct MI355X).
 * libpds_amd_stages.so is full (DESIGN.md sections 4.3 and 4.9); the rule is one capped library per 64 KiB of stage
 * kernels, none of them a home for the fused STFT kernel's instantiations.  This one has its own size cap (64 KiB of
 * device code), its own version and its own error string.  It shares no state and no header with libpds_amd.so or
 * libpds_amd_stages.so and may be loaded with or without them.
 *
 * Conventions as in pds_amd.h: every pointer named d_* is device memory of the current HIP device; `stream` is a
 * hipStream_t (NULL: the default stream); calls are asynchronous on it; a return value other than 0 leaves a message
 * for the calling thread in the string the last-error call returns.  There is no CPU path. */
#ifndef PDS_AMD_STAGES2_H
#define PDS_AMD_STAGES2_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDS_STAGES2_OK 0
#define PDS_STAGES2_ERR_INVALID -1 /* bad argument */
#define PDS_STAGES2_ERR_HIP -2     /* a HIP runtime call failed */

/* 100 * major + minor of this library; independent of the other two */
int32_t pds_stages2_version(void);
/* the calling thread's message of its last failed call into this library ("" before any) */
const char *pds_stages2_last_error(void);

/* ---------------------------------------------------------------------------------
 * Per-channel energy normalisation (PCEN; Wang et al. 2017, librosa.pcen); post.PCEN.
 *
 * The definition.
 *
 * Per utterance of T >= 1 rows and per column c, in float64, every operation rounded by itself (no contraction):
 *
 * 1. oms = 1.0 - smooth, rounded once on the host, and bp = bias ** power as numpy float64 on the host.  Both are
 *    passed to the kernels as arguments.  The device never recomputes them.
 * 2. M[0] = E[0], widened exactly.  For t >= 1, M[t] = (oms * M[t-1]) + (smooth * E[t]): two products and one sum,
 *    each rounded once.  This is librosa's steady-state start.
 * 3. y[t] = pow(E[t] / pow(eps + M[t], gain) + bias, power) - bp.  Every operation is float64.  There are no special
 *    cases for particular exponents.  The result is rounded once to the row type.
 *
 * The output has the input's type (float32 or float64) and shape.  Every column is treated alike, including an energy
 * column.  The input is meant to be the non-negative linear energies of a computer with use_log=False.  A negative
 * base gives what IEEE pow gives.  A NaN or infinite E[t] stays in M for the rest of the utterance, because a one-pole
 * filter does not forget.  T = 0 gives nothing.
 *
 * M is plain IEEE arithmetic: a host model reproduces it bit for bit.  y goes through the device's pow, which is not
 * the host's; between the entry points below y is bit-identical, because all of them inline one function
 * (csrc/pcen_rule.h) on the same (E, M).
 *
 * The offline calls work on a packed ragged batch: utterance b is the d_nrows[b] rows from row d_row_off[b] on, of C
 * values each, rows in_stride elements apart in d_in.
 *
 * pds_pcen_smooth_rows_*: step 2.  One lane per (utterance, column), adjacent lanes adjacent columns; a lane walks its
 * utterance in order with four rows' loads in flight.  M[t] of utterance b, column c goes to
 * d_m[(d_row_off[b] + t) * m_stride + c] as float64 (the same row indices as d_in).  Rows of d_m outside every
 * utterance are not written.  B == 0 returns 0 without looking at the pointers; bad sizes, strides below C, a smooth
 * outside (0, 1], an oms outside [0, 1] and null pointers return PDS_STAGES2_ERR_INVALID before any HIP call, as does a
 * batch whose B * C lanes need more than 2^31 - 1 blocks of 256 (split the batch).
 * --------------------------------------------------------------------------------- */
int32_t pds_pcen_smooth_rows_f32(const float *d_in, int64_t in_stride, const int64_t *d_row_off,
                                 const int64_t *d_nrows, int32_t B, int32_t C, double smooth, double oms, double *d_m,
                                 int64_t m_stride, void *stream);
int32_t pds_pcen_smooth_rows_f64(const double *d_in, int64_t in_stride, const int64_t *d_row_off,
                                 const int64_t *d_nrows, int32_t B, int32_t C, double smooth, double oms, double *d_m,
                                 int64_t m_stride, void *stream);

/* pds_pcen_compress_rows_*: step 3, elementwise over `rows` rows of C values with a grid-stride loop: row r, column c
 * reads d_in[r * in_stride + c] and d_m[r * m_stride + c] and writes d_out[r * out_stride + c].  d_out may be d_in (an
 * element is read and written by one lane).  Where all three strides equal C the rows lie back to back and the kernel
 * addresses element i at i (the same values, without the division of the mapping).  rows == 0 returns 0 without looking at the pointers; a row stride below C,
 * a null pointer and rows * C >= 2^63 return PDS_STAGES2_ERR_INVALID before any HIP call. */
int32_t pds_pcen_compress_rows_f32(const float *d_in, int64_t in_stride, const double *d_m, int64_t m_stride,
                                   int64_t rows, int32_t C, double gain, double bias, double power, double eps,
                                   double bp, float *d_out, int64_t out_stride, void *stream);
int32_t pds_pcen_compress_rows_f64(const double *d_in, int64_t in_stride, const double *d_m, int64_t m_stride,
                                   int64_t rows, int32_t C, double gain, double bias, double power, double eps,
                                   double bp, double *d_out, int64_t out_stride, void *stream);

/* pds_multistream_pcen_*: steps 2 and 3 of one tick of batched streaming (multistream.StreamBatch), in place.  Entry e
 * of the tick (0 <= e < n) is stream d_ids[e], whose new rows are rows d_rows[e] .. d_rows[e + 1] - 1 of d_statics
 * (contiguous rows of C values; d_rows is an ascending prefix of n + 1 row indices); d_fresh[e] != 0 says that the
 * first of them is the first row of the stream's utterance, so M = E there.  One lane per (entry, column) takes the
 * entry's rows in order.  d_state is float64[capacity][C], every stream's last M: read unless the entry is fresh,
 * written after the entry's last row; an entry without rows, or whose id lies outside [0, capacity), touches nothing.
 * A stream must not appear twice in one call.  d_statics may be null when no entry has rows.  n == 0 returns 0. */
int32_t pds_multistream_pcen_f32(float *d_statics, double *d_state, int64_t capacity, int32_t C, double smooth,
                                 double oms, double gain, double bias, double power, double eps, double bp,
                                 const int64_t *d_ids, const int64_t *d_rows, const uint8_t *d_fresh, int32_t n,
                                 void *stream);
int32_t pds_multistream_pcen_f64(double *d_statics, double *d_state, int64_t capacity, int32_t C, double smooth,
                                 double oms, double gain, double bias, double power, double eps, double bp,
                                 const int64_t *d_ids, const int64_t *d_rows, const uint8_t *d_fresh, int32_t n,
                                 void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PDS_AMD_STAGES2_H */
