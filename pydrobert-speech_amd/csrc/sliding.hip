// libpds_amd_stages.so: sliding-window CMVN for gfx950, offline over packed ragged batches and per stream across the
// ticks of batched streaming.  Declarations and the definition of the arithmetic: include/pds_amd_stages.h.
// Built without contraction (Makefile): every float64 operation is rounded separately, as the definition says.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/pds_amd_stages.h"
#include "sliding_window.h"
#include "stages_internal.h"

namespace pds {

static thread_local std::string g_stages_error;

// (shared with resample.hip through stages_internal.h: one error string for the whole library)
int32_t stages_invalid(const char *msg) {
  g_stages_error = msg;
  return PDS_STAGES_ERR_INVALID;
}

int32_t stages_hip_fail(hipError_t err, const char *what) {
  g_stages_error = std::string(what) + ": " + hipGetErrorString(err);
  return PDS_STAGES_ERR_HIP;
}

constexpr int SL_THREADS = 256;
constexpr int SL_AHEAD = 4;  // row loads in flight per lane while sums are rebuilt (the sums are sequential, the loads are not)

struct SlidingSums {
  double s1 = 0.0, s2 = 0.0;
  __device__ __forceinline__ void add(double d) {
    s1 = __dadd_rn(s1, d);
    s2 = __dadd_rn(s2, __dmul_rn(d, d));
  }
  __device__ __forceinline__ void sub(double d) {
    s1 = __dsub_rn(s1, d);
    s2 = __dsub_rn(s2, __dmul_rn(d, d));
  }
  // s1 = s2 = 0, then `count` values in order; load(j) gives value j
  template <typename Load>
  __device__ __forceinline__ void rebuild(int64_t count, Load load) {
    s1 = s2 = 0.0;
    for (int64_t j = 0; j < count; j += SL_AHEAD) {
      double v[SL_AHEAD];
#pragma unroll
      for (int u = 0; u < SL_AHEAD; ++u) v[u] = j + u < count ? load(j + u) : 0.0;
#pragma unroll
      for (int u = 0; u < SL_AHEAD; ++u)
        if (j + u < count) add(v[u]);
    }
  }
  // the normalised value of x over a window of n frames
  __device__ __forceinline__ double apply(double x, int64_t n, bool norm_vars) const {
    const double cnt = (double)n;
    const double mean = s1 / cnt;
    double y = __dsub_rn(x, mean);
    if (norm_vars) {
      if (n == 1) return 0.0;
      double var = __dsub_rn(s2 / cnt, __dmul_rn(mean, mean));
      if (!(var > 1e-10)) var = 1e-10;
      y = __dmul_rn(y, 1.0 / sqrt(var));
    }
    return y;
  }
};

// ---- offline: one lane per (utterance, segment of `refresh` frames, coefficient) ---------------------------------

template <typename T>
__global__ __launch_bounds__(SL_THREADS) void sliding_rows_kernel(
    const T *__restrict__ in, int64_t in_stride, const int64_t *__restrict__ row_off,
    const int64_t *__restrict__ nrows, int64_t max_segs, int32_t C, int64_t W, int64_t min_window, int32_t center,
    int32_t norm_vars, int64_t refresh, T *__restrict__ out, int64_t out_stride, int64_t total) {
  const int64_t g = (int64_t)blockIdx.x * SL_THREADS + threadIdx.x;
  if (g >= total) return;
  const int64_t e = g / C;
  const int c = (int)(g - e * C);
  const int64_t b = e / max_segs, seg = e - b * max_segs;
  const int64_t Tn = nrows[b];
  const int64_t t0 = seg * refresh;
  if (t0 >= Tn) return;  // (a shorter utterance of the batch, or an empty one)
  const int64_t t1 = t0 + refresh < Tn ? t0 + refresh : Tn;
  const T *x = in + row_off[b] * in_stride + c;
  T *y = out + row_off[b] * out_stride + c;
  int64_t ws, we;
  sliding_window(t0, Tn, W, min_window, center != 0, ws, we);
  SlidingSums s;
  s.rebuild(we - ws, [&](int64_t j) { return (double)x[(ws + j) * in_stride]; });
  // SL_AHEAD frames at a time: their windows first, with the loads of the frame itself, of the frame that may leave and
  // of the frame that may enter -- all without a condition (every row index lies in [0, Tn): the old ws, and
  // we - 1 < Tn; a frame past the segment's end repeats its last one), so that they are in flight together --, then
  // the sums and the stores in frame order.  At the segment's first frame the window is the one just summed: no move.
  for (int64_t t = t0; t < t1; t += SL_AHEAD) {
    double xv[SL_AHEAD], ov[SL_AHEAD], nv[SL_AHEAD];
    int64_t cnt[SL_AHEAD];
    bool left[SL_AHEAD], entered[SL_AHEAD];
#pragma unroll
    for (int u = 0; u < SL_AHEAD; ++u) {
      const int64_t tt = t + u < t1 ? t + u : t1 - 1;
      int64_t nws, nwe;
      sliding_window(tt, Tn, W, min_window, center != 0, nws, nwe);
      left[u] = nws != ws;
      entered[u] = nwe != we;
      xv[u] = (double)x[tt * in_stride];
      ov[u] = (double)x[ws * in_stride];
      nv[u] = (double)x[(nwe - 1) * in_stride];
      cnt[u] = nwe - nws;
      ws = nws;
      we = nwe;
    }
#pragma unroll
    for (int u = 0; u < SL_AHEAD; ++u) {
      if (t + u >= t1) continue;
      if (left[u]) s.sub(ov[u]);
      if (entered[u]) s.add(nv[u]);
      y[(t + u) * out_stride] = (T)s.apply(xv[u], cnt[u], norm_vars != 0);
    }
  }
}

template <typename T>
static int32_t launch_sliding_rows(const T *d_in, int64_t in_stride, const int64_t *d_row_off, const int64_t *d_nrows,
                                   int32_t B, int64_t max_rows, int32_t C, int32_t cmn_window, int32_t min_window,
                                   int32_t center, int32_t norm_vars, int32_t refresh, T *d_out, int64_t out_stride,
                                   void *stream) {
  if (B < 0 || max_rows < 0 || C <= 0) return stages_invalid("sliding_cmvn_rows: bad size");
  if (cmn_window < 1 || min_window < 1 || refresh < 1)
    return stages_invalid("sliding_cmvn_rows: cmn_window, min_window and refresh must be positive");
  if (B == 0 || max_rows == 0) return PDS_STAGES_OK;
  if (in_stride < C || out_stride < C) return stages_invalid("sliding_cmvn_rows: a row stride is below C");
  const int64_t max_segs = sliding_segments(max_rows, refresh);
  // lanes = B * max_segs * C, in 64 bits: each factor is below 2^31 and the product of the first two is checked
  const int64_t limit = (int64_t)0x7fffffff * SL_THREADS;
  if (max_segs > limit / B || (int64_t)B * max_segs > limit / C)
    return stages_invalid("sliding_cmvn_rows: too many lanes in one call (split the batch)");
  const int64_t total = (int64_t)B * max_segs * C;
  const int64_t blocks = (total + SL_THREADS - 1) / SL_THREADS;
  if (blocks > 0x7fffffff) return stages_invalid("sliding_cmvn_rows: too many lanes in one call (split the batch)");
  if (!d_in || !d_out || !d_row_off || !d_nrows) return stages_invalid("sliding_cmvn_rows: null pointer");
  hipLaunchKernelGGL(sliding_rows_kernel<T>, dim3((unsigned)blocks), dim3(SL_THREADS), 0, (hipStream_t)stream, d_in,
                     in_stride, d_row_off, d_nrows, max_segs, C, (int64_t)cmn_window, (int64_t)min_window, center,
                     norm_vars, (int64_t)refresh, d_out, out_stride, total);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return stages_hip_fail(err, "sliding_cmvn_rows launch");
  return PDS_STAGES_OK;
}

// ---- streaming: one thread per (stream, coefficient), the tick's rows in order, in place -------------------------

enum { MW_STREAM = 0, MW_FLAGS, MW_ROW, MW_ROWS, MW_SEEN, MW_FIELDS = 8 };
enum { MW_FLAG_FRESH = 1 };

template <typename T>
__global__ __launch_bounds__(SL_THREADS) void multistream_sliding_kernel(
    T *__restrict__ statics, T *__restrict__ ring, double *__restrict__ sums, int64_t capacity, int32_t F, int64_t W,
    int32_t norm_vars, int64_t refresh, const int64_t *__restrict__ meta, int64_t total) {
  const int64_t g = (int64_t)blockIdx.x * SL_THREADS + threadIdx.x;
  if (g >= total) return;
  const int64_t e = g / F;
  const int i = (int)(g - e * F);
  const int64_t *m = meta + e * MW_FIELDS;
  const int64_t k = m[MW_ROWS], sid = m[MW_STREAM];
  if (k <= 0) return;  // (nothing to normalise and, ring and sums being unchanged, nothing to write)
  if (sid < 0 || sid >= capacity) return;  // (no slot of the pools: the caller's ids are checked on the host)
  const int64_t slots = W + 1;
  T *rg = ring + sid * slots * F + i;  // slot q: rg[q * F]
  double *sm = sums + sid * 2 * (int64_t)F + i;
  int64_t t = m[MW_SEEN];
  SlidingSums s;
  if (!(m[MW_FLAGS] & MW_FLAG_FRESH)) {
    s.s1 = sm[0];
    s.s2 = sm[F];
  }
  T *x = statics + m[MW_ROW] * (int64_t)F + i;
  int64_t slot = sliding_ring_slot(t, W), phase = t % refresh;
  for (int64_t r = 0; r < k; ++r, ++t) {
    const T v = x[r * (int64_t)F];
    const double d = (double)v;
    const int64_t n = (t < W ? t : W) + 1;  // the window [max(0, t - W), t + 1)
    if (phase == 0) {
      // frames t - n + 1 .. t - 1 from the ring in frame order (this call's earlier rows among them), then this one
      int64_t q0 = slot - (n - 1);
      if (q0 < 0) q0 += slots;
      s.rebuild(n - 1, [&](int64_t j) {
        const int64_t q = q0 + j < slots ? q0 + j : q0 + j - slots;
        return (double)rg[q * F];
      });
      s.add(d);
    } else {
      if (t > W) s.sub((double)rg[slot * F]);  // the slot still holds frame t - W - 1, which leaves
      s.add(d);
    }
    rg[slot * F] = v;
    x[r * (int64_t)F] = (T)s.apply(d, n, norm_vars != 0);
    if (++slot == slots) slot = 0;
    if (++phase == refresh) phase = 0;
  }
  sm[0] = s.s1;
  sm[F] = s.s2;
}

template <typename T>
static int32_t launch_ms_sliding(T *d_statics, T *d_ring, double *d_sums, int64_t capacity, int32_t coeffs,
                                 int32_t cmn_window, int32_t norm_vars, int32_t refresh, const int64_t *d_meta,
                                 int32_t n, void *stream) {
  if (n < 0 || capacity < 0 || coeffs <= 0) return stages_invalid("multistream_sliding: bad size");
  if (cmn_window < 1 || refresh < 1) return stages_invalid("multistream_sliding: cmn_window and refresh must be positive");
  if (n == 0) return PDS_STAGES_OK;
  const int64_t total = (int64_t)n * coeffs;
  const int64_t blocks = (total + SL_THREADS - 1) / SL_THREADS;
  if (blocks > 0x7fffffff) return stages_invalid("multistream_sliding: too many elements in one call");
  // (d_statics may be null in a tick without new rows: no entry has any then)
  if (!d_meta || !d_ring || !d_sums) return stages_invalid("multistream_sliding: null pointer");
  hipLaunchKernelGGL(multistream_sliding_kernel<T>, dim3((unsigned)blocks), dim3(SL_THREADS), 0, (hipStream_t)stream,
                     d_statics, d_ring, d_sums, capacity, coeffs, (int64_t)cmn_window, norm_vars, (int64_t)refresh,
                     d_meta, total);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return stages_hip_fail(err, "multistream_sliding launch");
  return PDS_STAGES_OK;
}

}  // namespace pds

extern "C" {

int32_t pds_stages_version(void) { return 101; }  // 101: the energy VAD (vad.hip)

const char *pds_stages_last_error(void) { return pds::g_stages_error.c_str(); }

int32_t pds_sliding_cmvn_rows_f32(const float *d_in, int64_t in_stride, const int64_t *d_row_off,
                                  const int64_t *d_nrows, int32_t B, int64_t max_rows, int32_t C, int32_t cmn_window,
                                  int32_t min_window, int32_t center, int32_t norm_vars, int32_t refresh, float *d_out,
                                  int64_t out_stride, void *stream) {
  return pds::launch_sliding_rows<float>(d_in, in_stride, d_row_off, d_nrows, B, max_rows, C, cmn_window, min_window,
                                         center, norm_vars, refresh, d_out, out_stride, stream);
}
int32_t pds_sliding_cmvn_rows_f64(const double *d_in, int64_t in_stride, const int64_t *d_row_off,
                                  const int64_t *d_nrows, int32_t B, int64_t max_rows, int32_t C, int32_t cmn_window,
                                  int32_t min_window, int32_t center, int32_t norm_vars, int32_t refresh, double *d_out,
                                  int64_t out_stride, void *stream) {
  return pds::launch_sliding_rows<double>(d_in, in_stride, d_row_off, d_nrows, B, max_rows, C, cmn_window, min_window,
                                          center, norm_vars, refresh, d_out, out_stride, stream);
}

int32_t pds_multistream_sliding_f32(float *d_statics, float *d_ring, double *d_sums, int64_t capacity, int32_t coeffs,
                                    int32_t cmn_window, int32_t norm_vars, int32_t refresh, const int64_t *d_meta,
                                    int32_t n, void *stream) {
  return pds::launch_ms_sliding<float>(d_statics, d_ring, d_sums, capacity, coeffs, cmn_window, norm_vars, refresh,
                                       d_meta, n, stream);
}
int32_t pds_multistream_sliding_f64(double *d_statics, double *d_ring, double *d_sums, int64_t capacity,
                                    int32_t coeffs, int32_t cmn_window, int32_t norm_vars, int32_t refresh,
                                    const int64_t *d_meta, int32_t n, void *stream) {
  return pds::launch_ms_sliding<double>(d_statics, d_ring, d_sums, capacity, coeffs, cmn_window, norm_vars, refresh,
                                        d_meta, n, stream);
}

}  // extern "C"
