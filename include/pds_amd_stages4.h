/* C ABI of libpds_amd_stages4.so: the fourth capped library of stage kernels for gfx950 (AMD Instinct MI355X).
 * libpds_amd_stages.so is full, libpds_amd_stages2.so holds the PCEN kernels and no other and libpds_amd_stages3.so the
 * SpecAugment kernels and no other (DESIGN.md sections 4.3 and 4.9 to 4.11); the rule is one capped library per family
 * of stage kernels, 64 KiB of device code each, none of them a home for the fused STFT kernel's instantiations.  This
 * one has its own size cap, its own version and its own error string.  It shares no state and no header with
 * libpds_amd.so, libpds_amd_stages.so, libpds_amd_stages2.so or libpds_amd_stages3.so and may be loaded with or without
 * them.
 *
 * Conventions as in pds_amd.h: every pointer named d_* is device memory of the current HIP device; `stream` is a
 * hipStream_t (NULL: the default stream); calls are asynchronous on it; a return value other than 0 leaves a message
 * for the calling thread in the string the last-error call returns.  There is no CPU path. */
#ifndef PDS_AMD_STAGES4_H
#define PDS_AMD_STAGES4_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDS_STAGES4_OK 0
#define PDS_STAGES4_ERR_INVALID -1 /* bad argument */
#define PDS_STAGES4_ERR_HIP -2     /* a HIP runtime call failed */

/* 100 * major + minor of this library; independent of the other four */
int32_t pds_stages4_version(void);
/* the calling thread's message of its last failed call into this library ("" before any) */
const char *pds_stages4_last_error(void);

/* ---------------------------------------------------------------------------------
 * Perceptual linear prediction (PLP) cepstra of linear filter-bank energies, modelled on Kaldi's feature-plp.cc;
 * post.PLP.
 *
 * The definition.
 *
 * Notation for a row `x` of width `W`:
 *
 * - `copy = int(energy)`
 * - `F = W − copy ≥ 1`
 * - `D = F + 2`
 * - `p = lpc_order`
 * - `K = num_ceps`
 *
 * Refused with `ValueError`, before any device work:
 *
 * - `W > 256`
 * - `p` outside `[1, min(F + 1, 32)]`
 * - `K` outside `[1, p + 1]`
 * - `compress_factor` not finite or not positive
 * - `floor` not positive
 * - `lifter` or `scale` as `Cepstra` checks its `lifter`
 * - `equal_loudness=True` without `F` centre frequencies
 *
 * Host tables, float64, built once per `(width, device)`:
 *
 * - `w[f]`, the equal-loudness weight.
 *   - It is `1.0` when `equal_loudness=False`.
 *   - Otherwise `fsq = c_f²`, `fs = fsq / (fsq + 1.6e5)` and `w[f] = fs · fs · ((fsq + 1.44e6) / (fsq + 9.61e6))` for
 *     centre `c_f` in Hz.
 * - `B[i][j]` for `0 ≤ i ≤ p`, `0 ≤ j < D`, with `s = 1 / (2 (D − 1))` and `θ = π / (D − 1)`:
 *   - `B[i][0] = s`
 *   - `B[i][j] = 2 s cos(θ i j)` for `0 < j < D − 1`
 *   - `B[i][D−1] = s cos(θ i (D − 1))`
 * - `L[k] = scale · (1 + 0.5 Q sin(π k / Q))` with `Q = lifter`, for `0 ≤ k < K`.
 *   - `lifter` of `0` or `None` means no lifter: `L[k] = scale`.
 *
 * Per row, float64 throughout. Every operation is rounded by itself (no contraction: `-ffp-contract=off` for the
 * object).
 *
 * 1. Widen the row exactly: `e[f] = float64(x[copy + f])`.
 * 2. Floor: `g[f] = (e[f] < floor) ? floor : e[f]`. A NaN passes.
 * 3. Compress: `h[f] = pow(g[f] · w[f], compress_factor)`. The product is rounded once, then the device's `pow`.
 * 4. Duplicate the edges: `d[0] = h[0]`, `d[1 + f] = h[f]`, `d[D − 1] = h[F − 1]`.
 * 5. Autocorrelation: `r[i]` starts at `+0.0` and takes `r[i] = r[i] + B[i][j] · d[j]` for `j = 0 … D − 1`, in that
 *    order.
 * 6. Durbin. `E = r[0]`. For `i = 0 … p − 1`:
 *    1. `k = r[i+1]`, then `k = k + a[j] · r[i − j]` for `j = 0 … i − 1`.
 *    2. `k = k / E`.
 *    3. `c = 1 − k · k`, then `c = (c < 1e-5) ? 1e-5 : c`.
 *    4. `E = E · c`.
 *    5. `t[i] = −k`, and `t[j] = a[j] − k · a[i − j − 1]` for `j < i`.
 *    6. `a[0..i] = t[0..i]`.
 * 7. Cepstrum. For `i = 0 … p − 1`:
 *    1. `s = +0.0`.
 *    2. `s = s + (double(i − j) · a[j]) · q[i − j − 1]` for `j = 0 … i − 1`.
 *    3. `q[i] = −a[i] − s / double(i + 1)`.
 * 8. Output, each value rounded once to the row's dtype.
 *    - Without `energy`: `out[0] = L[0] · log(E)`, using the device's `log`.
 *    - With `energy`: `out[0] = log((e0 < floor) ? floor : e0)`, where `e0` is the widened column 0. It is neither
 *      lifted nor scaled.
 *    - `out[k] = L[k] · q[k − 1]` for `1 ≤ k < K`.
 *    - The output width is `K`.
 *
 * Consequences:
 *
 * - Everything but the `pow` of step 3 and the `log` of step 8 is plain IEEE arithmetic, so numpy reproduces it bit
 *   for bit **given the same `d`**.
 * - A row holding a NaN gives NaN in every computed column, and the clamp in step 6 is written so that it does.
 * - A row holding +inf is only promised not to disturb other rows.
 * - A row of zeros is finite, because of the floor.
 *
 * pds_plp_block_rows: the rows of a block (one lane per row, adjacent lanes on adjacent rows).
 * pds_plp_lds_bytes: the bytes of LDS a block takes at LPC order p (2 p + 1 float64 words per row); -1 for a p outside
 * [1, 32].
 *
 * pds_plp_rows_*: steps 1 to 8 for R rows of F + copy values each (copy is 0 or 1: the energy column), in_stride
 * elements apart in d_in.  d_w is float64[F], d_B float64[p + 1][F + 2] and d_L float64[K], as the definition builds
 * them.  Row i's K output values go to d_out + i * out_stride; columns past K and the input are not written.  Where
 * d_aux is not null it is float64[R][F + 3]: the row's d[0 .. D - 1] and, behind them, its final E.  Argument errors
 * return PDS_STAGES4_ERR_INVALID before any HIP call: a shape the definition refuses, a compress_factor that is not
 * finite and positive, a floor that is not positive, a row stride below the row's width, more than 2^31 - 1 blocks
 * (split the rows), null pointers (d_aux may be null).  R == 0 returns 0 without looking at the pointers.
 * --------------------------------------------------------------------------------- */
int32_t pds_plp_block_rows(void);
int64_t pds_plp_lds_bytes(int32_t p);
int32_t pds_plp_rows_f32(const float *d_in, int64_t in_stride, int64_t R, int32_t F, int32_t copy, const double *d_w,
                         const double *d_B, const double *d_L, int32_t p, int32_t K, double compress_factor,
                         double floor, float *d_out, int64_t out_stride, double *d_aux, void *stream);
int32_t pds_plp_rows_f64(const double *d_in, int64_t in_stride, int64_t R, int32_t F, int32_t copy, const double *d_w,
                         const double *d_B, const double *d_L, int32_t p, int32_t K, double compress_factor,
                         double floor, double *d_out, int64_t out_stride, double *d_aux, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PDS_AMD_STAGES4_H */
