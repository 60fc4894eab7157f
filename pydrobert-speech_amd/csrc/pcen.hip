// libpds_amd_stages2.so: per-channel energy normalisation (PCEN) for gfx950, offline over packed ragged batches and per
// stream across the ticks of batched streaming.  Declarations and the definition of the arithmetic:
// include/pds_amd_stages2.h.  Built without contraction (Makefile): every float64 operation is rounded separately, as
// the definition says.  The library stands alone: its own version, its own error string, no header shared with
// libpds_amd.so or libpds_amd_stages.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/pds_amd_stages2.h"
#include "pcen_rule.h"

namespace pds {

static thread_local std::string g_stages2_error;

static int32_t stages2_invalid(const char *msg) {
  g_stages2_error = msg;
  return PDS_STAGES2_ERR_INVALID;
}

static int32_t stages2_hip_fail(hipError_t err, const char *what) {
  g_stages2_error = std::string(what) + ": " + hipGetErrorString(err);
  return PDS_STAGES2_ERR_HIP;
}

constexpr int64_t PCEN_COMPRESS_BLOCKS = 8192;  // the grid-stride loop's grid: enough blocks to fill every CU

// ---- offline, phase 1: one lane per (utterance, column) walks the utterance and writes M --------------------------

template <typename T>
__global__ __launch_bounds__(PCEN_THREADS) void pcen_smooth_rows_kernel(
    const T *__restrict__ in, int64_t in_stride, const int64_t *__restrict__ row_off,
    const int64_t *__restrict__ nrows, int64_t C, double smooth, double oms, double *__restrict__ m_out,
    int64_t m_stride, int64_t total) {
  const int64_t g = pcen_lane(blockIdx.x, threadIdx.x);
  if (g >= total) return;
  int64_t b, c;
  pcen_lane_map(g, C, b, c);
  const int64_t Tn = nrows[b];
  if (Tn <= 0) return;  // (an empty utterance of the batch)
  const T *x = in + row_off[b] * in_stride + c;
  double *m = m_out + row_off[b] * m_stride + c;
  // (pcen_rule.h: four rows' loads in flight, then the chain and the stores in row order)
  pcen_smooth_walk(
      Tn, oms, smooth, [&](int64_t t) { return (double)x[t * in_stride]; },
      [&](int64_t t, double v) { m[t * m_stride] = v; });
}

template <typename T>
static int32_t launch_smooth_rows(const T *d_in, int64_t in_stride, const int64_t *d_row_off, const int64_t *d_nrows,
                                  int32_t B, int32_t C, double smooth, double oms, double *d_m, int64_t m_stride,
                                  void *stream) {
  if (B < 0 || C <= 0) return stages2_invalid("pcen_smooth_rows: bad size");
  if (!(smooth > 0.0 && smooth <= 1.0) || !(oms >= 0.0 && oms <= 1.0))
    return stages2_invalid("pcen_smooth_rows: smooth must lie in (0, 1] and oms in [0, 1]");
  if (B == 0) return PDS_STAGES2_OK;
  if (in_stride < C || m_stride < C) return stages2_invalid("pcen_smooth_rows: a row stride is below C");
  const int64_t total = pcen_lane_count(B, C);
  const int64_t blocks = total < 0 ? -1 : pcen_block_count(total);
  if (blocks < 0) return stages2_invalid("pcen_smooth_rows: too many lanes in one call (split the batch)");
  if (!d_in || !d_m || !d_row_off || !d_nrows) return stages2_invalid("pcen_smooth_rows: null pointer");
  hipLaunchKernelGGL(pcen_smooth_rows_kernel<T>, dim3((unsigned)blocks), dim3(PCEN_THREADS), 0, (hipStream_t)stream,
                     d_in, in_stride, d_row_off, d_nrows, (int64_t)C, smooth, oms, d_m, m_stride, total);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return stages2_hip_fail(err, "pcen_smooth_rows launch");
  return PDS_STAGES2_OK;
}

// ---- offline, phase 2: elementwise over rows x C, a grid-stride loop ------------------------------------------------

// (in and out may be the same memory: an element is read and written by one lane)
template <typename T>
__global__ __launch_bounds__(PCEN_THREADS) void pcen_compress_rows_kernel(
    const T *in, int64_t in_stride, const double *__restrict__ m_in, int64_t m_stride, int64_t C, int64_t total,
    double gain, double bias, double power, double eps, double bp, T *out, int64_t out_stride, int32_t dense) {
  const int64_t step = (int64_t)gridDim.x * PCEN_THREADS;
  // no unroll: two float64 pow per element are the body, and copies of them are what spills
#pragma unroll 1
  for (int64_t i = pcen_lane(blockIdx.x, threadIdx.x); i < total; i += step) {
    // rows that lie back to back in all three arrays (`dense`, the same for every lane): element i is at i, and the
    // 64-bit division of the mapping is left out
    int64_t ei = i, mi = i, oi = i;
    if (!dense) {
      int64_t r, c;
      pcen_lane_map(i, C, r, c);
      ei = r * in_stride + c;
      mi = r * m_stride + c;
      oi = r * out_stride + c;
    }
    const double e = (double)in[ei];
    const double m = m_in[mi];
    out[oi] = (T)pcen_compress(e, m, gain, bias, power, eps, bp);
  }
}

template <typename T>
static int32_t launch_compress_rows(const T *d_in, int64_t in_stride, const double *d_m, int64_t m_stride,
                                    int64_t rows, int32_t C, double gain, double bias, double power, double eps,
                                    double bp, T *d_out, int64_t out_stride, void *stream) {
  if (rows < 0 || C <= 0) return stages2_invalid("pcen_compress_rows: bad size");
  if (rows == 0) return PDS_STAGES2_OK;
  if (in_stride < C || m_stride < C || out_stride < C)
    return stages2_invalid("pcen_compress_rows: a row stride is below C");
  const int64_t total = pcen_lane_count(rows, C);
  if (total < 0) return stages2_invalid("pcen_compress_rows: too many elements in one call");
  if (!d_in || !d_m || !d_out) return stages2_invalid("pcen_compress_rows: null pointer");
  int64_t blocks = (total + PCEN_THREADS - 1) / PCEN_THREADS;
  if (blocks > PCEN_COMPRESS_BLOCKS) blocks = PCEN_COMPRESS_BLOCKS;
  const int32_t dense = in_stride == C && m_stride == C && out_stride == C;
  hipLaunchKernelGGL(pcen_compress_rows_kernel<T>, dim3((unsigned)blocks), dim3(PCEN_THREADS), 0, (hipStream_t)stream,
                     d_in, in_stride, d_m, m_stride, (int64_t)C, total, gain, bias, power, eps, bp, d_out, out_stride,
                     dense);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return stages2_hip_fail(err, "pcen_compress_rows launch");
  return PDS_STAGES2_OK;
}

// ---- streaming: one lane per (stream, column), the tick's rows in order, in place ----------------------------------

template <typename T>
__global__ __launch_bounds__(PCEN_THREADS) void multistream_pcen_kernel(
    T *__restrict__ statics, double *__restrict__ state, int64_t capacity, int64_t C, double smooth, double oms,
    double gain, double bias, double power, double eps, double bp, const int64_t *__restrict__ ids,
    const int64_t *__restrict__ rows, const uint8_t *__restrict__ fresh, int64_t total) {
  const int64_t g = pcen_lane(blockIdx.x, threadIdx.x);
  if (g >= total) return;
  int64_t e, c;
  pcen_lane_map(g, C, e, c);
  const int64_t r0 = rows[e], k = rows[e + 1] - r0, sid = ids[e];
  if (k <= 0) return;  // (no row: the state stays as it is)
  if (sid < 0 || sid >= capacity) return;  // (no slot of the pool: the caller's ids are checked on the host)
  double *st = state + sid * C + c;
  bool first = fresh[e] != 0;
  double m = first ? 0.0 : *st;  // (a fresh stream's slot is not read)
  T *x = statics + r0 * C + c;
#pragma unroll 1
  for (int64_t r = 0; r < k; ++r) {
    const double en = (double)x[r * C];
    m = pcen_smooth_row(first, oms, smooth, m, en);
    first = false;
    x[r * C] = (T)pcen_compress(en, m, gain, bias, power, eps, bp);
  }
  *st = m;
}

template <typename T>
static int32_t launch_ms_pcen(T *d_statics, double *d_state, int64_t capacity, int32_t C, double smooth, double oms,
                              double gain, double bias, double power, double eps, double bp, const int64_t *d_ids,
                              const int64_t *d_rows, const uint8_t *d_fresh, int32_t n, void *stream) {
  if (n < 0 || capacity < 0 || C <= 0) return stages2_invalid("multistream_pcen: bad size");
  if (!(smooth > 0.0 && smooth <= 1.0) || !(oms >= 0.0 && oms <= 1.0))
    return stages2_invalid("multistream_pcen: smooth must lie in (0, 1] and oms in [0, 1]");
  if (n == 0) return PDS_STAGES2_OK;
  const int64_t total = pcen_lane_count(n, C);
  const int64_t blocks = total < 0 ? -1 : pcen_block_count(total);
  if (blocks < 0) return stages2_invalid("multistream_pcen: too many elements in one call");
  // (d_statics may be null in a tick without new rows: no entry has any then)
  if (!d_state || !d_ids || !d_rows || !d_fresh) return stages2_invalid("multistream_pcen: null pointer");
  hipLaunchKernelGGL(multistream_pcen_kernel<T>, dim3((unsigned)blocks), dim3(PCEN_THREADS), 0, (hipStream_t)stream,
                     d_statics, d_state, capacity, (int64_t)C, smooth, oms, gain, bias, power, eps, bp, d_ids, d_rows,
                     d_fresh, total);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return stages2_hip_fail(err, "multistream_pcen launch");
  return PDS_STAGES2_OK;
}

}  // namespace pds

extern "C" {

int32_t pds_stages2_version(void) { return 100; }

const char *pds_stages2_last_error(void) { return pds::g_stages2_error.c_str(); }

int32_t pds_pcen_smooth_rows_f32(const float *d_in, int64_t in_stride, const int64_t *d_row_off,
                                 const int64_t *d_nrows, int32_t B, int32_t C, double smooth, double oms, double *d_m,
                                 int64_t m_stride, void *stream) {
  return pds::launch_smooth_rows<float>(d_in, in_stride, d_row_off, d_nrows, B, C, smooth, oms, d_m, m_stride, stream);
}
int32_t pds_pcen_smooth_rows_f64(const double *d_in, int64_t in_stride, const int64_t *d_row_off,
                                 const int64_t *d_nrows, int32_t B, int32_t C, double smooth, double oms, double *d_m,
                                 int64_t m_stride, void *stream) {
  return pds::launch_smooth_rows<double>(d_in, in_stride, d_row_off, d_nrows, B, C, smooth, oms, d_m, m_stride, stream);
}

int32_t pds_pcen_compress_rows_f32(const float *d_in, int64_t in_stride, const double *d_m, int64_t m_stride,
                                   int64_t rows, int32_t C, double gain, double bias, double power, double eps,
                                   double bp, float *d_out, int64_t out_stride, void *stream) {
  return pds::launch_compress_rows<float>(d_in, in_stride, d_m, m_stride, rows, C, gain, bias, power, eps, bp, d_out,
                                          out_stride, stream);
}
int32_t pds_pcen_compress_rows_f64(const double *d_in, int64_t in_stride, const double *d_m, int64_t m_stride,
                                   int64_t rows, int32_t C, double gain, double bias, double power, double eps,
                                   double bp, double *d_out, int64_t out_stride, void *stream) {
  return pds::launch_compress_rows<double>(d_in, in_stride, d_m, m_stride, rows, C, gain, bias, power, eps, bp, d_out,
                                           out_stride, stream);
}

int32_t pds_multistream_pcen_f32(float *d_statics, double *d_state, int64_t capacity, int32_t C, double smooth,
                                 double oms, double gain, double bias, double power, double eps, double bp,
                                 const int64_t *d_ids, const int64_t *d_rows, const uint8_t *d_fresh, int32_t n,
                                 void *stream) {
  return pds::launch_ms_pcen<float>(d_statics, d_state, capacity, C, smooth, oms, gain, bias, power, eps, bp, d_ids,
                                    d_rows, d_fresh, n, stream);
}
int32_t pds_multistream_pcen_f64(double *d_statics, double *d_state, int64_t capacity, int32_t C, double smooth,
                                 double oms, double gain, double bias, double power, double eps, double bp,
                                 const int64_t *d_ids, const int64_t *d_rows, const uint8_t *d_fresh, int32_t n,
                                 void *stream) {
  return pds::launch_ms_pcen<double>(d_statics, d_state, capacity, C, smooth, oms, gain, bias, power, eps, bp, d_ids,
                                     d_rows, d_fresh, n, stream);
}

}  // extern "C"
