/* C ABI of libpds_amd_stages3.so: the third capped library of stage kernels for gfx950 (AMD Instinct MI355X).
 * libpds_amd_stages.so is full and libpds_amd_stages2.so holds the PCEN kernels and no other (DESIGN.md sections 4.3,
 * 4.9 and 4.10); the rule is one capped library per family of stage kernels, 64 KiB of device code each, none of them a
 * home for the fused STFT kernel's instantiations.  This one has its own size cap, its own version and its own error
 * string.  It shares no state and no header with libpds_amd.so, libpds_amd_stages.so or libpds_amd_stages2.so and may
 * be loaded with or without them.
 *
 * Conventions as in pds_amd.h: every pointer named d_* is device memory of the current HIP device; `stream` is a
 * hipStream_t (NULL: the default stream); calls are asynchronous on it; a return value other than 0 leaves a message
 * for the calling thread in the string the last-error call returns.  There is no CPU path. */
#ifndef PDS_AMD_STAGES3_H
#define PDS_AMD_STAGES3_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDS_STAGES3_OK 0
#define PDS_STAGES3_ERR_INVALID -1 /* bad argument */
#define PDS_STAGES3_ERR_HIP -2     /* a HIP runtime call failed */

/* 100 * major + minor of this library; independent of the other three */
int32_t pds_stages3_version(void);
/* the calling thread's message of its last failed call into this library ("" before any) */
const char *pds_stages3_last_error(void);

/* ---------------------------------------------------------------------------------
 * SpecAugment (Park et al. 2019): a time warp, frequency masks and time masks over a feature matrix; post.SpecAugment.
 *
 * The definition.
 *
 * Per utterance of T ≥ 1 rows and C ≥ 1 columns with a 64-bit key k:
 *
 * 0. Generator.
 *    - `P(i, d)` is one Philox4x32-10 block with counter words `(i, 0, d, 0)` and key words `(k mod 2³², k >> 32)`.
 *      Its output words are `r0..r3`. The round function is the one `csrc/dither_noise.h` already has.
 *    - `U(r, n) = (uint64(r) · uint64(n + 1)) >> 32` for 0 ≤ n < 2³¹. It is an integer in [0, n].
 * 1. Warp.
 *    - If `warp = W ≥ 1` and `T ≥ 2W + 3`, let `r = P(0, 1)`.
 *    - `w0 = W + 1 + U(r0, T − 3 − 2W)`.
 *    - `w1 = w0 − W + U(r1, 2W)`.
 *    - Then `W + 1 ≤ w0 ≤ T − 2 − W` and `1 ≤ w1 ≤ T − 2`.
 *    - Otherwise `w0 = w1 = −1` (no warp).
 * 2. Frequency mask j, 0 ≤ j < freq_masks.
 *    - `r = P(j, 2)`.
 *    - `f = U(r0, min(freq_width, C))`.
 *    - `f0 = U(r1, C − f)`.
 *    - The mask covers columns `[f0, f0 + f)`.
 * 3. Time mask j, 0 ≤ j < time_masks.
 *    - `b = min(time_width, (int64) floor(time_ratio · (double) T))`, the product rounded once.
 *    - `r = P(j, 3)`.
 *    - `t = U(r0, b)`.
 *    - `t0 = U(r1, T − t)`.
 *    - The mask covers rows `[t0, t0 + t)`.
 * 4. Warped value `v[t][c]`.
 *    - Without a warp, `v[t][c]` is `x[t][c]`, copied.
 *    - With one, the source position is float64 with every operation rounded by itself (no contraction):
 *      - for `t ≤ w1`: `s = ((double) t · (double) w0) / (double) w1`
 *      - for `t > w1`: `s = (double) w0 + ((double)(t − w1) · (double)(T − 1 − w0)) / (double)(T − 1 − w1)`
 *    - `i = floor(s)` and `a = s − i`.
 *    - If `a == 0`, the value is `x[i][c]`, copied.
 *    - Otherwise the value is `x[i][c] + a · (x[i+1][c] − x[i][c])`, with the samples widened exactly, the
 *      difference, product and sum each rounded once, and the result rounded once to the row type.
 *    - I checked on the CPU for every T < 60, W < 8 and every admissible (w0, w1) that:
 *      - s is strictly increasing,
 *      - s(0) = 0, s(w1) = w0 and s(T − 1) = T − 1 exactly,
 *      - `i + 1 ≤ T − 1` whenever `a > 0`.
 * 5. Mean (only for `fill="mean"`).
 *    - It is taken over the utterance's T · C input elements in float64, as 64 interleaved partial sums.
 *    - `p_j` sums the elements with flat index `e = t · C + c ≡ j (mod 64)`, in ascending e, starting from +0.0.
 *    - `s = ((+0.0 + p_0) + p_1) + … + p_63`.
 *    - `m = s / (double)(T · C)`.
 *    - This is the rule and the reason of §4.8. Lane j of one wave owns `p_j`, and the host restates it in a few
 *      lines.
 * 6. Output.
 *    - `out[t][c]` is the fill value, rounded once to the row type, if c lies in any frequency mask or t in any time
 *      mask.
 *    - Otherwise `out[t][c]` is `v[t][c]`.
 *    - T = 0 gives nothing.
 *
 * Consequences: the plan (steps 1 to 3) is integers only; unmasked values without a warp, or at a == 0, are copies,
 * byte for byte (NaN payloads and signed zeros pass); everything else is plain IEEE float64 arithmetic, which a host
 * model reproduces bit for bit; a computed NaN (inf - inf in the interpolation) is only promised to be a NaN.  The
 * draws are defined for T < 2^31; the Python layer refuses a longer utterance, and the plan kernel gives it the plan of
 * an empty one.
 *
 * The calls work on a packed ragged batch: utterance b is the d_nrows[b] rows from row d_row_off[b] on, of C values
 * each, rows in_stride elements apart in d_in.  Argument errors return PDS_STAGES3_ERR_INVALID before any HIP call;
 * B == 0 returns 0 without looking at the pointers.
 *
 * pds_specaug_tile_rows: the rows of a block's tile of the apply kernel.
 *
 * pds_specaug_plan: steps 1 to 3, one lane per utterance.  d_keys holds the utterances' 64-bit keys (their bits, as
 * int64).  Writes int64 d_plan[B][2 + 2 * freq_masks + 2 * time_masks] = w0, w1, (f0, f) per frequency mask, (t0, t) per
 * time mask; an utterance with T = 0 gets -1, -1 and zeros.  freq_masks / time_masks outside [0, 16], widths outside
 * [0, 2^31 - 2], a time_ratio outside (0, 1] and a warp outside [0, 2^29] are refused.
 * --------------------------------------------------------------------------------- */
int32_t pds_specaug_tile_rows(void);
int32_t pds_specaug_plan(const int64_t *d_nrows, const int64_t *d_keys, int32_t B, int32_t C, int32_t freq_masks,
                         int64_t freq_width, int32_t time_masks, int64_t time_width, double time_ratio, int64_t warp,
                         int64_t *d_plan, void *stream);

/* pds_specaug_mean_rows_*: step 5.  One wave per utterance; lane j owns p_j, keeps sixteen loads in flight and adds them
 * in order; lane 0 combines the 64 sums in lane order.  Writes float64 d_mean[B]; NaN for an utterance with T = 0. */
int32_t pds_specaug_mean_rows_f32(const float *d_in, int64_t in_stride, const int64_t *d_row_off,
                                  const int64_t *d_nrows, int32_t B, int32_t C, double *d_mean, void *stream);
int32_t pds_specaug_mean_rows_f64(const double *d_in, int64_t in_stride, const int64_t *d_row_off,
                                  const int64_t *d_nrows, int32_t B, int32_t C, double *d_mean, void *stream);

/* pds_specaug_apply_rows_*: steps 4 and 6.  One block per (utterance, tile of pds_specaug_tile_rows() rows), the tiles
 * counted on max_rows (the longest utterance's rows: rows of an utterance past max_rows are not written); blocks of
 * shorter utterances leave at once.  The block reads its utterance's row of d_plan (as pds_specaug_plan wrote it, or
 * as the caller did) once; its lanes take the tile's elements in row-major order, adjacent lanes adjacent columns.
 * Row t, column c of utterance b goes to d_out[(d_row_off[b] + t) * out_stride + c]; rows outside every utterance are
 * not written.  A masked element is stored without a load.  The fill value is d_mean[b] where d_mean is not null, else
 * `fill`.  A plan row whose w0 or w1 lies outside [1, T - 2] is not warped, and its mask words are only compared, so no
 * plan row leads outside the utterance.  d_out == d_in is allowed only when no plan row has w0 >= 1 (an element is
 * then read and written by one lane).  More than 2^31 - 1 blocks is refused (split the batch), as are a row stride
 * below C, mask counts outside [0, 16] and null pointers (d_mean may be null); max_rows == 0 returns 0. */
int32_t pds_specaug_apply_rows_f32(const float *d_in, int64_t in_stride, const int64_t *d_row_off,
                                   const int64_t *d_nrows, int32_t B, int32_t C, const int64_t *d_plan,
                                   int32_t freq_masks, int32_t time_masks, const double *d_mean, double fill,
                                   float *d_out, int64_t out_stride, int64_t max_rows, void *stream);
int32_t pds_specaug_apply_rows_f64(const double *d_in, int64_t in_stride, const int64_t *d_row_off,
                                   const int64_t *d_nrows, int32_t B, int32_t C, const int64_t *d_plan,
                                   int32_t freq_masks, int32_t time_masks, const double *d_mean, double fill,
                                   double *d_out, int64_t out_stride, int64_t max_rows, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PDS_AMD_STAGES3_H */
