/* C ABI of libpds_amd_stages.so: stage kernels for gfx950 (AMD Instinct MI355X) that are not part of the fused STFT
 * kernel's instantiation matrix.  libpds_amd.so's device code is held to a size bound that guards that matrix
 * (DESIGN.md section 4.3); stages that stand alone are built into this second, small library, which has a size cap of
 * its own (64 KiB of device code), its own version and its own error string.  It shares no state with libpds_amd.so
 * and may be loaded with or without it.
 *
 * Conventions as in pds_amd.h: every pointer named d_* is device memory of the current HIP device; `stream` is a
 * hipStream_t (NULL: the default stream); calls are asynchronous on it; a return value other than 0 leaves a message
 * for the calling thread in the string the last-error call returns.  There is no CPU path. */
#ifndef PDS_AMD_STAGES_H
#define PDS_AMD_STAGES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDS_STAGES_OK 0
#define PDS_STAGES_ERR_INVALID -1 /* bad argument */
#define PDS_STAGES_ERR_HIP -2     /* a HIP runtime call failed */

/* 100 * major + minor of this library; independent of libpds_amd.so's */
int32_t pds_stages_version(void);
/* the calling thread's message of its last failed call into this library ("" before any) */
const char *pds_stages_last_error(void);

/* ---------------------------------------------------------------------------------
 * Sliding-window cepstral mean (and variance) normalisation: Kaldi's apply-cmvn-sliding; post.SlidingCMVN.
 *
 * The definition.  For an utterance of T frames, frame t, W = cmn_window >= 1, min_window >= 1, the window [ws, we) is
 *
 *     center:      ws = t - W / 2;  we = ws + W            (integer division)
 *     not center:  ws = t - W;      we = t + 1
 *     if ws < 0:                 we -= ws;  ws = 0
 *     if not center and we > t:  we = max(t + 1, min_window)
 *     if we > T:                 ws -= we - T;  we = T;  ws = max(ws, 0)
 *
 * so that 0 <= ws <= t < we <= T, ws and we each move by 0 or 1 from one frame to the next, and the window holds at
 * most max(W + 1, min_window) frames (the causal window is W + 1 frames wide once it is full, as Kaldi's).  Per
 * coefficient, in float64, with x widened first and every operation rounded separately (division and square root
 * correctly rounded), refresh >= 1:
 *
 *     t % refresh == 0:  s1 = s2 = 0;  for u = ws .. we - 1 in order:  s1 += x_u;  s2 += x_u * x_u
 *     else:              if ws moved:  s1 -= x_old;  s2 -= x_old * x_old      (x_old: the frame that left)
 *                        then, if we moved:  s1 += x_new;  s2 += x_new * x_new  (x_new: the frame that entered)
 *     n = we - ws;  mean = s1 / n;  y = x_t - mean
 *     norm_vars:  n == 1:  y = 0
 *                 else:    var = s2 / n - mean * mean;  if !(var > 1e-10) then var = 1e-10;  y = y * (1 / sqrt(var))
 *
 * and y is rounded once to the input's type.  `refresh` is part of the result (in its last bits): segments of
 * `refresh` frames are independent, rounding does not drift over a long stream, and a NaN or infinite frame stops
 * affecting the output at the first refresh after it has left the window.
 *
 * The offline call, over a packed ragged batch: utterance b is the d_nrows[b] rows from row d_row_off[b] on, of C
 * values each, rows in_stride elements apart in d_in and out_stride apart in d_out (both >= C; row indices are the
 * same in both).  One lane handles one (utterance, segment, coefficient), adjacent lanes adjacent coefficients;
 * max_rows is the largest d_nrows[b] (it sizes the grid; an utterance's rows beyond it are not written).  d_out must
 * not overlap d_in: a lane reads rows that other lanes write.  Any C >= 1, any row count including 0 and 1.  B == 0 or
 * max_rows == 0 returns 0 without looking at the pointers; bad sizes, strides and null pointers return
 * PDS_STAGES_ERR_INVALID before any HIP call, as does a batch whose B * ceil(max_rows / refresh) * C lanes need more
 * than 2^31 - 1 blocks of 256 (split the batch).
 * --------------------------------------------------------------------------------- */
int32_t pds_sliding_cmvn_rows_f32(const float *d_in, int64_t in_stride, const int64_t *d_row_off,
                                  const int64_t *d_nrows, int32_t B, int64_t max_rows, int32_t C, int32_t cmn_window,
                                  int32_t min_window, int32_t center, int32_t norm_vars, int32_t refresh, float *d_out,
                                  int64_t out_stride, void *stream);
int32_t pds_sliding_cmvn_rows_f64(const double *d_in, int64_t in_stride, const int64_t *d_row_off,
                                  const int64_t *d_nrows, int32_t B, int64_t max_rows, int32_t C, int32_t cmn_window,
                                  int32_t min_window, int32_t center, int32_t norm_vars, int32_t refresh, double *d_out,
                                  int64_t out_stride, void *stream);

/* ---------------------------------------------------------------------------------
 * The same normalisation per stream across the ticks of batched streaming (StreamBatch(sliding_cmvn=...)): the causal
 * window with min_window = 1, ws = max(0, t - W), we = t + 1, which needs nothing of the future.  The call runs once
 * per tick, in place on the tick's statics in d_statics (contiguous rows of `coeffs` values), where the running CMVN
 * call of libpds_amd.so would run: before the deltas.  Per stream the device keeps
 *   a ring of its last W + 1 input rows, d_ring = T[capacity][W + 1][coeffs]: frame t lies in slot t % (W + 1), so the
 *     slot frame t overwrites holds exactly the frame that leaves the window at t, frame t - W - 1;
 *   its sums, d_sums = double[capacity][2][coeffs] (s1, then s2).
 * One pool each, no ping-pong: a (stream, coefficient) pair is read and written by one thread of a call, which takes
 * the tick's rows in order.  d_meta holds n entries of 8 int64:
 *   [0] stream s (0 <= s < capacity)   [1] flags: bit 0 fresh (the stream has seen no frame: ring and sums are not read)
 *   [2] first row of the stream's new statics in d_statics (row index)   [3] their number k (may be 0)
 *   [4] frames t0 the stream has seen before this call (0 if fresh): the new rows are frames t0 .. t0 + k - 1
 *   [5..7] reserved, 0
 * and every row is normalised by the definition above (at a refresh frame the sums are rebuilt from the ring, in
 * frame order), bit for bit what the offline call gives over the stream's whole sequence of statics with center = 0
 * and min_window = 1.  An entry with k > 0 writes its k rows to the ring and its sums back.  Streams of one call are
 * distinct.  d_statics may be NULL when no entry has rows.  n == 0 returns 0 without looking at the pointers; bad
 * sizes and null pointers return PDS_STAGES_ERR_INVALID before any HIP call.
 * --------------------------------------------------------------------------------- */
int32_t pds_multistream_sliding_f32(float *d_statics, float *d_ring, double *d_sums, int64_t capacity, int32_t coeffs,
                                    int32_t cmn_window, int32_t norm_vars, int32_t refresh, const int64_t *d_meta,
                                    int32_t n, void *stream);
int32_t pds_multistream_sliding_f64(double *d_statics, double *d_ring, double *d_sums, int64_t capacity,
                                    int32_t coeffs, int32_t cmn_window, int32_t norm_vars, int32_t refresh,
                                    const int64_t *d_meta, int32_t n, void *stream);

/* ---------------------------------------------------------------------------------
 * Windowed-sinc rate conversion: Kaldi's LinearResample with its feature-extraction defaults; pre.Resample.
 *
 * The definition.  from_rate and to_rate are positive integers, num_zeros >= 1, 0 < rolloff <= 1.
 *
 *     g = gcd(from_rate, to_rate);  in_unit = from_rate / g;  out_unit = to_rate / g
 *     cutoff = rolloff * 0.5 * min(from_rate, to_rate);  width = num_zeros / (2 * cutoff)
 *     for phase p in [0, out_unit):  t = p / to_rate
 *         first[p] = ceil((t - width) * from_rate);  last[p] = floor((t + width) * from_rate)
 *         ntaps[p] = last[p] - first[p] + 1
 *         for j in [0, ntaps[p]):  d = (first[p] + j) / from_rate - t
 *             w[p][j] = f(d) * h(d) / from_rate
 *             f(d) = sin(2 pi cutoff d) / (pi d), and 2 cutoff at d == 0
 *             h(d) = 0.5 (1 + cos(2 pi cutoff / num_zeros d)) for |d| < width, else 0
 *
 * The table is built on the host in float64: first and ntaps as int32, w as float64 padded with zeros to max_taps,
 * the largest ntaps[p].  An utterance of n samples gives m = ceil(n * to_rate / from_rate) output samples (Kaldi's
 * flush form), and output k = u * out_unit + p, 0 <= p < out_unit, is
 *
 *     y[k] = sum over j in [0, ntaps[p]) of w[p][j] * x[first[p] + u * in_unit + j]
 *
 * in float64, over j in ascending order, starting from +0.0, with x widened first and each product and each sum
 * rounded separately; a tap whose index falls outside [0, n) contributes nothing; y[k] is rounded once to the output
 * type: float32 for float32 and int16 input (int16 is widened exactly), float64 for float64 input.  NaN and infinite
 * samples reach exactly the outputs whose windows hold them.
 *
 * The tables of a call: d_first and d_ntaps, int32[out_unit]; d_weights, double[max_taps][out_unit] -- tap-major, the
 * transpose of w above, so that adjacent lanes, which own adjacent phases, read adjacent weights.  A table of more than
 * out_unit * max_taps = 1048576 entries is refused (PDS_STAGES_ERR_INVALID): indices into it are 32-bit.
 *
 * The offline call, over a packed ragged batch: utterance b is the d_in_len[b] samples from d_in + d_in_off[b] on
 * (any offset: no alignment is assumed), and its m_b outputs go to d_out + d_out_off[b].  One lane computes one output
 * sample, adjacent lanes adjacent outputs of one utterance; max_len is the largest d_in_len[b] (it sizes the grid: an
 * utterance's outputs beyond ceil(max_len * out_unit / in_unit) are not written).  d_out must not overlap d_in.
 * B == 0 or max_len == 0 returns 0 without looking at the pointers; bad sizes and null pointers return
 * PDS_STAGES_ERR_INVALID before any HIP call, as does a batch whose B * ceil(max_out / 256) blocks exceed 2^31 - 1
 * (split the batch).
 * --------------------------------------------------------------------------------- */
int32_t pds_resample_packed_f32(const float *d_in, const int64_t *d_in_off, const int64_t *d_in_len,
                                const int64_t *d_out_off, int32_t B, int64_t max_len, int32_t in_unit,
                                int32_t out_unit, int32_t max_taps, const int32_t *d_first, const int32_t *d_ntaps,
                                const double *d_weights, float *d_out, void *stream);
int32_t pds_resample_packed_f64(const double *d_in, const int64_t *d_in_off, const int64_t *d_in_len,
                                const int64_t *d_out_off, int32_t B, int64_t max_len, int32_t in_unit,
                                int32_t out_unit, int32_t max_taps, const int32_t *d_first, const int32_t *d_ntaps,
                                const double *d_weights, double *d_out, void *stream);
int32_t pds_resample_packed_i16_f32(const int16_t *d_in, const int64_t *d_in_off, const int64_t *d_in_len,
                                    const int64_t *d_out_off, int32_t B, int64_t max_len, int32_t in_unit,
                                    int32_t out_unit, int32_t max_taps, const int32_t *d_first,
                                    const int32_t *d_ntaps, const double *d_weights, float *d_out, void *stream);

/* ---------------------------------------------------------------------------------
 * The same conversion per stream across the ticks of batched streaming (multistream_resample.ResampleBatch).  After a
 * stream has been given n samples in all, the due outputs are those k with
 * first[p] + u * in_unit + ntaps[p] - 1 <= n - 1: the outputs whose whole window has arrived (the last index is
 * non-decreasing in k, so this is a count); at the stream's end the rest up to ceil(n * to_rate / from_rate) follow,
 * with the missing future read as nothing.  Per stream the device keeps its last max_taps - 1 input samples,
 * d_hist = T[capacity][max_taps - 1] in the chunks' type: slot i holds sample n - (max_taps - 1) + i of a stream that
 * has seen n samples (slots of samples below 0 are never read).  The call runs once per tick, one block per entry;
 * d_meta holds n entries of 8 int64:
 *   [0] stream s (0 <= s < capacity)   [1] offset of the stream's chunk in d_samples   [2] its length c (may be 0)
 *   [3] samples n0 the stream has seen before this call (0 if fresh: the history is not read)
 *   [4] the first output k0 to compute   [5] their number (may be 0)   [6] offset of these outputs in d_out
 *   [7] reserved, 0
 * and outputs k0 .. k0 + [5] - 1 are computed by the definition above over the stream's samples [0, n0 + c), bit for
 * bit what the offline call gives over the stream's whole signal when the host follows the rule above.  An entry with
 * c > 0 then writes the stream's next history.  Streams of one call are distinct.  d_samples and d_out may be NULL
 * when no entry has samples or outputs.  n == 0 returns 0 without looking at the pointers; bad sizes and null pointers
 * return PDS_STAGES_ERR_INVALID before any HIP call.
 * --------------------------------------------------------------------------------- */
int32_t pds_multistream_resample_f32(const float *d_samples, float *d_hist, int64_t capacity, int32_t in_unit,
                                     int32_t out_unit, int32_t max_taps, const int32_t *d_first,
                                     const int32_t *d_ntaps, const double *d_weights, const int64_t *d_meta, int32_t n,
                                     float *d_out, void *stream);
int32_t pds_multistream_resample_f64(const double *d_samples, double *d_hist, int64_t capacity, int32_t in_unit,
                                     int32_t out_unit, int32_t max_taps, const int32_t *d_first,
                                     const int32_t *d_ntaps, const double *d_weights, const int64_t *d_meta, int32_t n,
                                     double *d_out, void *stream);
int32_t pds_multistream_resample_i16_f32(const int16_t *d_samples, int16_t *d_hist, int64_t capacity, int32_t in_unit,
                                         int32_t out_unit, int32_t max_taps, const int32_t *d_first,
                                         const int32_t *d_ntaps, const double *d_weights, const int64_t *d_meta,
                                         int32_t n, float *d_out, void *stream);

/* ---------------------------------------------------------------------------------
 * Energy VAD: Kaldi's voiced-frame decision (compute-vad-energy, ComputeVadEnergy); post.EnergyVAD.  Library
 * version 101 on.
 *
 * The definition.  For an utterance of T >= 1 frames with log energies e_t, each widened to float64 first,
 * energy_mean_scale >= 0, frames_context >= 0, 0 < proportion_threshold < 1:
 *
 *     if energy_mean_scale != 0:
 *         p_j = sum of e_t over t = j, j + 64, j + 128, .. in that order, starting from +0.0      (0 <= j < 64)
 *         s   = +0.0;  for j = 0 .. 63 in order:  s += p_j
 *         thr = energy_threshold + (energy_mean_scale * s) / T       (each operation rounded once, in float64)
 *     else:
 *         thr = energy_threshold                                      (the energies are not summed)
 *     for frame t:  lo = max(0, t - frames_context);  hi = min(T - 1, t + frames_context)
 *         den = hi - lo + 1;  num = the number of u in [lo, hi] with e_u > thr
 *         voiced_t = (double) num >= (double) den * proportion_threshold
 *
 * The 64 interleaved partial sums are part of the result (in its last bits): lane j of a wave owns p_j, and the host
 * reproduces the sum.  A NaN energy is never above the threshold; a NaN or infinite sum makes every comparison false
 * or true as IEEE says; nothing is special-cased.  csrc/vad_rule.h holds the rule for host and device.
 *
 * The call, over a packed ragged batch: utterance b is the d_nrows[b] rows from row d_row_off[b] on; d_energy points
 * at the energy of row 0 and the energy of row r lies r * stride elements behind it (stride >= 1: the row stride of
 * the feature matrix whose column this is).  d_voiced[r] becomes 0 or 1 for every row r of every utterance -- rows of
 * no utterance are not written -- and d_count[b] the number of voiced rows of utterance b (0 for an empty one).  One
 * wave handles one utterance.  max_rows is the largest d_nrows[b]; it only tells a batch without rows.  B == 0 or
 * max_rows == 0 returns 0 without looking at the pointers (nothing is written then, d_count included); bad sizes,
 * parameters outside the ranges above and null pointers return PDS_STAGES_ERR_INVALID before any HIP call.
 * --------------------------------------------------------------------------------- */
int32_t pds_vad_energy_rows_f32(const float *d_energy, int64_t stride, const int64_t *d_row_off,
                                const int64_t *d_nrows, int32_t B, int64_t max_rows, double energy_threshold,
                                double energy_mean_scale, int32_t frames_context, double proportion_threshold,
                                uint8_t *d_voiced, int64_t *d_count, void *stream);
int32_t pds_vad_energy_rows_f64(const double *d_energy, int64_t stride, const int64_t *d_row_off,
                                const int64_t *d_nrows, int32_t B, int64_t max_rows, double energy_threshold,
                                double energy_mean_scale, int32_t frames_context, double proportion_threshold,
                                uint8_t *d_voiced, int64_t *d_count, void *stream);

/* ---------------------------------------------------------------------------------
 * Selection of the kept rows of a packed ragged batch, in order (Kaldi's select-voiced-frames); post.EnergyVAD.
 *
 * Rows are `words` 32-bit words wide and are copied as they are, byte for byte (NaN payloads and signed zeros pass):
 * a float32 row of C values has C words, a float64 row 2 C.  in_stride and out_stride, the distances from row to
 * row, are in 32-bit words too (both >= words).  Utterance b is the d_nrows[b] rows from row d_row_off[b] of d_in on,
 * d_keep[r] belongs to row r of d_in, and the rows of utterance b whose d_keep is not 0 are written, in order, to
 * rows d_out_row_off[b], d_out_row_off[b] + 1, .. of d_out; nothing else of d_out is written.  The caller sizes d_out
 * and lays out d_out_row_off from the counts of kept rows (those of the decision call above, for its d_voiced).
 * d_out must not overlap d_in.
 *
 * One block handles one (utterance, tile of 256 rows): it counts the kept rows in front of its tile, ranks its own by
 * ballots, and all its lanes copy the kept rows, adjacent lanes adjacent words; max_rows is the largest d_nrows[b] (it
 * sizes the grid; an utterance's rows beyond it are not looked at).  B == 0 or max_rows == 0 returns 0 without
 * looking at the pointers; bad sizes, strides and null pointers return PDS_STAGES_ERR_INVALID before any HIP call, as
 * does a batch whose B * ceil(max_rows / 256) blocks exceed 2^31 - 1 (split the batch).
 * --------------------------------------------------------------------------------- */
int32_t pds_select_rows_w32(const void *d_in, int64_t in_stride, int32_t words, const int64_t *d_row_off,
                            const int64_t *d_nrows, int32_t B, int64_t max_rows, const uint8_t *d_keep,
                            const int64_t *d_out_row_off, void *d_out, int64_t out_stride, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PDS_AMD_STAGES_H */
