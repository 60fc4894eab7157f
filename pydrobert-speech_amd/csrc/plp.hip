// libpds_amd_stages4.so: perceptual linear prediction (PLP) cepstra for gfx950, one kernel over packed rows that the
// offline calls, the command-line tool and the streaming stage all launch.  Declarations and the definition of the
// arithmetic: include/pds_amd_stages4.h.  Built without contraction (Makefile): every float64 operation is rounded
// separately, as the definition says.  The library stands alone: its own version, its own error string, no header
// shared with the other four libraries.
//
// The form: one lane per row, adjacent lanes on adjacent rows, a block of one wave.  F and p are run-time values, and a
// per-lane array indexed at run time would go to scratch, so the working vectors (r, which q takes over, and a:
// 2 p + 1 float64 words a row) live in LDS element-major, v[j][lane]: the 64 lanes of an access sit on 64 consecutive
// 8-byte words, no bank conflicts.  LDS is sized per launch from p (12.8 KB at p = 12, 33.3 KB at p = 32).  B, w and L
// are read at wave-uniform addresses.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/pds_amd_stages4.h"
#include "plp_rule.h"

namespace pds {

static thread_local std::string g_stages4_error;

static int32_t stages4_invalid(const char *msg) {
  g_stages4_error = msg;
  return PDS_STAGES4_ERR_INVALID;
}

static int32_t stages4_hip_fail(hipError_t err, const char *what) {
  g_stages4_error = std::string(what) + ": " + hipGetErrorString(err);
  return PDS_STAGES4_ERR_HIP;
}

template <typename T>
__global__ __launch_bounds__(PLP_THREADS) void plp_rows_kernel(
    const T *__restrict__ in, int64_t in_stride, int64_t R, int F, int copy, const double *__restrict__ w,
    const double *__restrict__ B, const double *__restrict__ L, int p, int K, double compress_factor, double floor,
    T *__restrict__ out, int64_t out_stride, double *__restrict__ aux) {
  extern __shared__ __attribute__((aligned(16))) double plp_work[];  // [2 p + 1][PLP_THREADS]
  const int64_t row = plp_lane_row(blockIdx.x, threadIdx.x);
  if (row >= R) return;  // (no barrier in this kernel: a lane's words of the LDS are its own)
  const T *x = in + row * in_stride;
  T *y = out + row * out_stride;
  const int D = F + 2;
  double *ax = aux ? aux + row * (int64_t)(D + 1) : nullptr;
  plp_row(
      [&](int c) { return (double)x[c]; }, F, copy, w, B, L, p, K, compress_factor, floor, plp_work + threadIdx.x,
      (int64_t)PLP_THREADS, [](double b, double e) { return pow(b, e); }, [](double v) { return log(v); },
      [&](int k, double v) { y[k] = (T)v; }, ax != nullptr, [&](int j, double v) { ax[j] = v; });
}

template <typename T>
static int32_t launch_plp_rows(const T *d_in, int64_t in_stride, int64_t R, int32_t F, int32_t copy, const double *d_w,
                               const double *d_B, const double *d_L, int32_t p, int32_t K, double compress_factor,
                               double floor, T *d_out, int64_t out_stride, double *d_aux, void *stream) {
  if (R < 0) return stages4_invalid("plp_rows: bad size");
  if (!plp_shape_ok(F, copy, p, K))
    return stages4_invalid(
        "plp_rows: needs 1 <= F, F + copy <= 256, copy 0 or 1, 1 <= p <= min(F + 1, 32) and 1 <= K <= p + 1");
  if (!(compress_factor > 0.0) || !(compress_factor <= 1.7976931348623157e308))
    return stages4_invalid("plp_rows: compress_factor must be finite and positive");
  if (!(floor > 0.0)) return stages4_invalid("plp_rows: floor must be positive");
  if (R == 0) return PDS_STAGES4_OK;
  if (in_stride < (int64_t)F + copy || out_stride < K) return stages4_invalid("plp_rows: a row stride is below its width");
  const int64_t blocks = plp_block_count(R);
  if (blocks < 0) return stages4_invalid("plp_rows: too many rows in one call (split them)");
  if (!d_in || !d_w || !d_B || !d_L || !d_out) return stages4_invalid("plp_rows: null pointer");
  hipLaunchKernelGGL(plp_rows_kernel<T>, dim3((unsigned)blocks), dim3(PLP_THREADS), (size_t)plp_block_lds_bytes(p),
                     (hipStream_t)stream, d_in, in_stride, R, (int)F, (int)copy, d_w, d_B, d_L, (int)p, (int)K,
                     compress_factor, floor, d_out, out_stride, d_aux);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return stages4_hip_fail(err, "plp_rows launch");
  return PDS_STAGES4_OK;
}

}  // namespace pds

extern "C" {

int32_t pds_stages4_version(void) { return 100; }

const char *pds_stages4_last_error(void) { return pds::g_stages4_error.c_str(); }

int32_t pds_plp_block_rows(void) { return pds::PLP_THREADS; }

int64_t pds_plp_lds_bytes(int32_t p) {
  return (p < 1 || p > pds::PLP_MAX_ORDER) ? -1 : pds::plp_block_lds_bytes(p);
}

int32_t pds_plp_rows_f32(const float *d_in, int64_t in_stride, int64_t R, int32_t F, int32_t copy, const double *d_w,
                         const double *d_B, const double *d_L, int32_t p, int32_t K, double compress_factor,
                         double floor, float *d_out, int64_t out_stride, double *d_aux, void *stream) {
  return pds::launch_plp_rows<float>(d_in, in_stride, R, F, copy, d_w, d_B, d_L, p, K, compress_factor, floor, d_out,
                                     out_stride, d_aux, stream);
}
int32_t pds_plp_rows_f64(const double *d_in, int64_t in_stride, int64_t R, int32_t F, int32_t copy, const double *d_w,
                         const double *d_B, const double *d_L, int32_t p, int32_t K, double compress_factor,
                         double floor, double *d_out, int64_t out_stride, double *d_aux, void *stream) {
  return pds::launch_plp_rows<double>(d_in, in_stride, R, F, copy, d_w, d_B, d_L, p, K, compress_factor, floor, d_out,
                                      out_stride, d_aux, stream);
}

}  // extern "C"
