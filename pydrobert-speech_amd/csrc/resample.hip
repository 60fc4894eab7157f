// libpds_amd_stages.so: windowed-sinc rate conversion for gfx950, offline over packed ragged batches and per stream
// across the ticks of batched streaming.  Declarations and the definition of the arithmetic:
// include/pds_amd_stages.h; the index arithmetic: resample_index.h.
// Built without contraction (Makefile): every float64 product and sum is rounded separately, as the definition says.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pds_amd_stages.h"
#include "resample_index.h"
#include "stages_internal.h"

namespace pds {

constexpr int RS_THREADS = 256;
constexpr int RS_AHEAD = 4;  // taps whose loads are in flight together (the sum is sequential, the loads are not)

// One output: the taps of phase p in ascending order from +0.0.  `base` is the input index of tap 0, inputs exist at
// [0, hi), `load(i)` gives input i for i in [clo, hi) (clo <= every index a counted tap has).  A tap beyond ntaps or
// outside [0, hi) is loaded from a clamped index and not added: it contributes nothing, whatever lies there.
// `w` is the table tap-major, w[j * out_unit + p], so that adjacent lanes (adjacent phases) read adjacent weights.
template <typename Load>
__device__ __forceinline__ double resample_output(int32_t p, int64_t base, int64_t clo, int64_t hi, int32_t nt,
                                                  int32_t max_taps, int32_t out_unit,
                                                  const double *__restrict__ w, Load load) {
  double s = 0.0;
  for (int32_t j0 = 0; j0 < max_taps; j0 += RS_AHEAD) {
    double xv[RS_AHEAD], wv[RS_AHEAD];
    bool ok[RS_AHEAD];
#pragma unroll
    for (int a = 0; a < RS_AHEAD; ++a) {
      const int32_t j = j0 + a;
      const int64_t idx = base + j;
      ok[a] = j < nt && idx >= 0 && idx < hi;
      const int32_t jj = j < max_taps ? j : max_taps - 1;
      int64_t ci = idx < hi ? idx : hi - 1;
      ci = ci > clo ? ci : clo;
      xv[a] = (double)load(ci);
      wv[a] = w[jj * out_unit + p];
    }
#pragma unroll
    for (int a = 0; a < RS_AHEAD; ++a) {
      const double t = __dadd_rn(s, __dmul_rn(wv[a], xv[a]));
      s = ok[a] ? t : s;
    }
  }
  return s;
}

// The same sum for an output whose whole window, rounded up to whole groups of RS_AHEAD taps, lies inside its utterance
// (all but the outputs at an utterance's two ends): `xp` points at the input of tap 0, nothing is clamped, and the
// loads carry their tap as a constant offset.  A group is summed without conditions where every lane of the wave
// that is here still has RS_AHEAD taps to go; the same products and sums in the same order as above.
template <typename TI>
__device__ __forceinline__ double resample_interior(const TI *__restrict__ xp, int32_t p, int32_t nt, int32_t max_taps,
                                                    int32_t out_unit, const double *__restrict__ w) {
  double s = 0.0;
  for (int32_t j0 = 0; j0 < max_taps; j0 += RS_AHEAD) {
    double xv[RS_AHEAD], wv[RS_AHEAD];
#pragma unroll
    for (int a = 0; a < RS_AHEAD; ++a) {
      const int32_t jj = j0 + a < max_taps ? j0 + a : max_taps - 1;  // (uniform over the wave)
      const double *wj = w + (int64_t)jj * out_unit;
      xv[a] = (double)xp[j0 + a];
      wv[a] = wj[(uint32_t)p];
    }
    const int32_t rem = nt - j0;
    if (__all(rem >= RS_AHEAD)) {
#pragma unroll
      for (int a = 0; a < RS_AHEAD; ++a) s = __dadd_rn(s, __dmul_rn(wv[a], xv[a]));
    } else {
#pragma unroll
      for (int a = 0; a < RS_AHEAD; ++a) {
        const double t = __dadd_rn(s, __dmul_rn(wv[a], xv[a]));
        s = a < rem ? t : s;
      }
    }
  }
  return s;
}

// ---- offline: one lane per output sample, adjacent lanes adjacent outputs of one utterance -------------------------
// A wave's 64 stores are one contiguous run, and at every tap its 64 loads fall into one span of about
// 64 * in_unit / out_unit samples that moves by one sample per tap: each cache line of the input is fetched from
// memory once and then served by the vector cache for the other taps, with no staging pass and no limit on the ratio.

template <typename TI, typename TO>
__global__ __launch_bounds__(RS_THREADS) void resample_packed_kernel(
    const TI *__restrict__ in, const int64_t *__restrict__ in_off, const int64_t *__restrict__ in_len,
    const int64_t *__restrict__ out_off, int64_t tiles, int32_t in_unit, int32_t out_unit, int32_t max_taps,
    const int32_t *__restrict__ first, const int32_t *__restrict__ ntaps, const double *__restrict__ w,
    TO *__restrict__ out) {
  const int64_t blk = blockIdx.x;
  const int64_t b = blk / tiles;
  const int64_t k = (blk - b * tiles) * RS_THREADS + threadIdx.x;
  const int64_t n = in_len[b];
  if (k >= resample_num_output_samples(n, in_unit, out_unit)) return;  // (a shorter utterance, or an empty one)
  int64_t u;
  int32_t p;
  resample_split(k, out_unit, u, p);
  const TI *x = in + in_off[b];
  const int64_t base = resample_base(u, in_unit, first[p]);
  const int32_t groups = (max_taps + RS_AHEAD - 1) / RS_AHEAD * RS_AHEAD;  // the taps the interior form loads
  double y;
  if (base >= 0 && base + groups <= n)
    y = resample_interior(x + base, p, ntaps[p], max_taps, out_unit, w);
  else
    y = resample_output(p, base, 0, n, ntaps[p], max_taps, out_unit, w, [&](int64_t i) { return x[i]; });
  out[out_off[b] + k] = (TO)y;
}

static int32_t check_table(int32_t in_unit, int32_t out_unit, int32_t max_taps, const char *bad_size,
                           const char *too_large) {
  if (in_unit <= 0 || out_unit <= 0 || max_taps <= 0) return stages_invalid(bad_size);
  if ((int64_t)out_unit * max_taps > RESAMPLE_MAX_TABLE) return stages_invalid(too_large);
  return PDS_STAGES_OK;
}

template <typename TI, typename TO>
static int32_t launch_resample_packed(const TI *d_in, const int64_t *d_in_off, const int64_t *d_in_len,
                                      const int64_t *d_out_off, int32_t B, int64_t max_len, int32_t in_unit,
                                      int32_t out_unit, int32_t max_taps, const int32_t *d_first,
                                      const int32_t *d_ntaps, const double *d_weights, TO *d_out, void *stream) {
  if (B < 0 || max_len < 0) return stages_invalid("resample_packed: bad size");
  const int32_t rc = check_table(in_unit, out_unit, max_taps, "resample_packed: the units and max_taps must be positive",
                                 "resample_packed: the weight table has more than 1048576 entries");
  if (rc != PDS_STAGES_OK) return rc;
  if (max_len > ((int64_t)1 << 62)) return stages_invalid("resample_packed: bad size");
  if (B == 0 || max_len == 0) return PDS_STAGES_OK;
  const int64_t max_out = resample_num_output_samples(max_len, in_unit, out_unit);
  const int64_t tiles = (max_out + RS_THREADS - 1) / RS_THREADS;  // blocks per utterance; B * tiles in 64 bits
  if (tiles > (int64_t)0x7fffffff / B)
    return stages_invalid("resample_packed: too many lanes in one call (split the batch)");
  if (!d_in || !d_in_off || !d_in_len || !d_out_off || !d_first || !d_ntaps || !d_weights || !d_out)
    return stages_invalid("resample_packed: null pointer");
  hipLaunchKernelGGL((resample_packed_kernel<TI, TO>), dim3((unsigned)(tiles * B)), dim3(RS_THREADS), 0,
                     (hipStream_t)stream, d_in, d_in_off, d_in_len, d_out_off, tiles, in_unit, out_unit, max_taps,
                     d_first, d_ntaps, d_weights, d_out);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return stages_hip_fail(err, "resample_packed launch");
  return PDS_STAGES_OK;
}

// ---- streaming: one block per stream of the tick ---------------------------------------------------------------------
// The block computes the stream's due outputs from its history (the last max_taps - 1 samples before this chunk) and
// the chunk, then -- behind a barrier, nobody reads the old history any more -- writes the next history.

enum { MR_STREAM = 0, MR_CHUNK, MR_LEN, MR_SEEN, MR_FIRST_OUT, MR_NUM_OUT, MR_OUT, MR_FIELDS = 8 };

template <typename TI, typename TO>
__global__ __launch_bounds__(RS_THREADS) void multistream_resample_kernel(
    const TI *__restrict__ samples, TI *__restrict__ hist_pool, int64_t capacity, int32_t in_unit, int32_t out_unit,
    int32_t max_taps, const int32_t *__restrict__ first, const int32_t *__restrict__ ntaps,
    const double *__restrict__ w, const int64_t *__restrict__ meta, TO *__restrict__ out) {
  const int64_t *m = meta + (int64_t)blockIdx.x * MR_FIELDS;
  const int64_t sid = m[MR_STREAM], c = m[MR_LEN], n0 = m[MR_SEEN];
  if (sid < 0 || sid >= capacity) return;  // (no slot of the pool: the caller's ids are checked on the host)
  if (c < 0 || n0 < 0) return;
  const int64_t H = max_taps - 1;
  TI *hist = hist_pool + sid * H;  // samples n0 - H .. n0 - 1 of the stream (those below 0 are never read)
  const TI *chunk = samples + m[MR_CHUNK];  // samples n0 .. n0 + c - 1
  const int64_t n1 = n0 + c, k0 = m[MR_FIRST_OUT], count = m[MR_NUM_OUT];
  const int64_t clo = n0 - H > 0 ? n0 - H : 0;
  TO *y = out + m[MR_OUT];
  const bool any = n1 > clo;  // (else no sample can be loaded and none is counted: every output is +0.0)
  for (int64_t r = threadIdx.x; r < count; r += RS_THREADS) {
    int64_t u;
    int32_t p;
    resample_split(k0 + r, out_unit, u, p);
    double v = 0.0;
    if (any)
      v = resample_output(p, resample_base(u, in_unit, first[p]), clo, n1, ntaps[p], max_taps, out_unit, w,
                          [&](int64_t i) { return i >= n0 ? chunk[i - n0] : hist[i - (n0 - H)]; });
    y[r] = (TO)v;
  }
  if (c == 0 || H == 0) return;  // (the history stays what it is; uniform over the block)
  // next history: slot i holds sample n1 - H + i, from the chunk where that is >= n0, else from old slot i + c.  In
  // passes of one block's width, ascending: a pass reads slots at or above its own, which no earlier pass wrote.
  for (int64_t i0 = 0; i0 < H; i0 += RS_THREADS) {
    __syncthreads();  // (first pass: the outputs above have read the old history)
    const int64_t i = i0 + threadIdx.x;
    const int64_t s = n1 - H + i;  // the sample's index in the stream
    TI v = (TI)0;
    if (i < H) v = s >= n0 ? chunk[s - n0] : hist[i + c];
    __syncthreads();
    if (i < H) hist[i] = v;
  }
}

template <typename TI, typename TO>
static int32_t launch_ms_resample(const TI *d_samples, TI *d_hist, int64_t capacity, int32_t in_unit, int32_t out_unit,
                                  int32_t max_taps, const int32_t *d_first, const int32_t *d_ntaps,
                                  const double *d_weights, const int64_t *d_meta, int32_t n, TO *d_out, void *stream) {
  if (n < 0 || capacity < 0) return stages_invalid("multistream_resample: bad size");
  const int32_t rc =
      check_table(in_unit, out_unit, max_taps, "multistream_resample: the units and max_taps must be positive",
                  "multistream_resample: the weight table has more than 1048576 entries");
  if (rc != PDS_STAGES_OK) return rc;
  if (n == 0) return PDS_STAGES_OK;
  // (d_samples and d_out may be null in a tick without samples or without outputs; d_hist where max_taps == 1)
  if (!d_meta || !d_first || !d_ntaps || !d_weights || (!d_hist && max_taps > 1))
    return stages_invalid("multistream_resample: null pointer");
  hipLaunchKernelGGL((multistream_resample_kernel<TI, TO>), dim3((unsigned)n), dim3(RS_THREADS), 0,
                     (hipStream_t)stream, d_samples, d_hist, capacity, in_unit, out_unit, max_taps, d_first, d_ntaps,
                     d_weights, d_meta, d_out);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return stages_hip_fail(err, "multistream_resample launch");
  return PDS_STAGES_OK;
}

}  // namespace pds

extern "C" {

#define PDS_RESAMPLE_PACKED(NAME, TI, TO)                                                                            \
  int32_t NAME(const TI *d_in, const int64_t *d_in_off, const int64_t *d_in_len, const int64_t *d_out_off, int32_t B, \
               int64_t max_len, int32_t in_unit, int32_t out_unit, int32_t max_taps, const int32_t *d_first,          \
               const int32_t *d_ntaps, const double *d_weights, TO *d_out, void *stream) {                            \
    return pds::launch_resample_packed<TI, TO>(d_in, d_in_off, d_in_len, d_out_off, B, max_len, in_unit, out_unit,    \
                                               max_taps, d_first, d_ntaps, d_weights, d_out, stream);                 \
  }
PDS_RESAMPLE_PACKED(pds_resample_packed_f32, float, float)
PDS_RESAMPLE_PACKED(pds_resample_packed_f64, double, double)
PDS_RESAMPLE_PACKED(pds_resample_packed_i16_f32, int16_t, float)
#undef PDS_RESAMPLE_PACKED

#define PDS_MS_RESAMPLE(NAME, TI, TO)                                                                                 \
  int32_t NAME(const TI *d_samples, TI *d_hist, int64_t capacity, int32_t in_unit, int32_t out_unit, int32_t max_taps, \
               const int32_t *d_first, const int32_t *d_ntaps, const double *d_weights, const int64_t *d_meta,        \
               int32_t n, TO *d_out, void *stream) {                                                                  \
    return pds::launch_ms_resample<TI, TO>(d_samples, d_hist, capacity, in_unit, out_unit, max_taps, d_first,         \
                                           d_ntaps, d_weights, d_meta, n, d_out, stream);                             \
  }
PDS_MS_RESAMPLE(pds_multistream_resample_f32, float, float)
PDS_MS_RESAMPLE(pds_multistream_resample_f64, double, double)
PDS_MS_RESAMPLE(pds_multistream_resample_i16_f32, int16_t, float)
#undef PDS_MS_RESAMPLE

}  // extern "C"
