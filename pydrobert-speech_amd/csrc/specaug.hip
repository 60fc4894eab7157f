// libpds_amd_stages3.so: SpecAugment (time warp, frequency masks, time masks) for gfx950 over packed ragged batches.
// Declarations and the definition: include/pds_amd_stages3.h.  Built without contraction (Makefile): every float64
// operation is rounded separately, as the definition says.  The library stands alone: its own version, its own error
// string, no header shared with libpds_amd.so, libpds_amd_stages.so or libpds_amd_stages2.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/pds_amd_stages3.h"
#include "specaug_rule.h"

namespace pds {

static thread_local std::string g_stages3_error;

static int32_t stages3_invalid(const char *msg) {
  g_stages3_error = msg;
  return PDS_STAGES3_ERR_INVALID;
}

static int32_t stages3_hip_fail(hipError_t err, const char *what) {
  g_stages3_error = std::string(what) + ": " + hipGetErrorString(err);
  return PDS_STAGES3_ERR_HIP;
}

// ---- the plan: one lane per utterance -------------------------------------------------------------------------------

__global__ __launch_bounds__(SPECAUG_THREADS) void specaug_plan_kernel(
    const int64_t *__restrict__ nrows, const int64_t *__restrict__ keys, int32_t B, int64_t C, int32_t freq_masks,
    int64_t freq_width, int32_t time_masks, int64_t time_width, double time_ratio, int64_t warp,
    int64_t *__restrict__ plan) {
  const int64_t b = (int64_t)blockIdx.x * SPECAUG_THREADS + threadIdx.x;
  if (b >= B) return;
  specaug_plan_one(nrows[b], C, (uint64_t)keys[b], freq_masks, freq_width, time_masks, time_width, time_ratio, warp,
                   plan + b * specaug_plan_words(freq_masks, time_masks));
}

// ---- the mean: one wave per utterance, lane j owns partial sum j ----------------------------------------------------

template <typename T>
__global__ __launch_bounds__(SPECAUG_THREADS) void specaug_mean_rows_kernel(
    const T *__restrict__ in, int64_t in_stride, const int64_t *__restrict__ row_off,
    const int64_t *__restrict__ nrows, int32_t B, int64_t C, double *__restrict__ mean) {
  const int lane = threadIdx.x & (SPECAUG_WAVE - 1);
  const int64_t b = (int64_t)blockIdx.x * (SPECAUG_THREADS / SPECAUG_WAVE) + (threadIdx.x >> 6);
  if (b >= B) return;  // (the same in the whole wave)
  const int64_t Tn = nrows[b];
  const T *x = in + row_off[b] * in_stride;
  double p = 0.0;
  if (Tn > 0) p = specaug_lane_sum(lane, Tn, C, [&](int64_t t, int64_t c) { return (double)x[t * in_stride + c]; });
  // lane 0 adds the 64 partial sums in lane order (every lane runs the chain: the shuffles need them all)
  double s = 0.0;
#pragma unroll 8
  for (int j = 0; j < SPECAUG_WAVE; ++j) s = s + __shfl(p, j);
  if (lane == 0) mean[b] = s / (double)(Tn * C);  // (0 / 0 for an empty utterance: NaN)
}

template <typename T>
static int32_t launch_mean_rows(const T *d_in, int64_t in_stride, const int64_t *d_row_off, const int64_t *d_nrows,
                                int32_t B, int32_t C, double *d_mean, void *stream) {
  if (B < 0 || C <= 0) return stages3_invalid("specaug_mean_rows: bad size");
  if (B == 0) return PDS_STAGES3_OK;
  if (in_stride < C) return stages3_invalid("specaug_mean_rows: the row stride is below C");
  if (!d_in || !d_row_off || !d_nrows || !d_mean) return stages3_invalid("specaug_mean_rows: null pointer");
  const int64_t blocks = specaug_mean_blocks(B);  // (B < 2^31: always a grid)
  hipLaunchKernelGGL(specaug_mean_rows_kernel<T>, dim3((unsigned)blocks), dim3(SPECAUG_THREADS), 0,
                     (hipStream_t)stream, d_in, in_stride, d_row_off, d_nrows, B, (int64_t)C, d_mean);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return stages3_hip_fail(err, "specaug_mean_rows launch");
  return PDS_STAGES3_OK;
}

// ---- warp and masks: one block per (utterance, tile of SPECAUG_ROWS rows) -------------------------------------------
//
// The block reads its utterance's plan once into LDS, its first SPECAUG_ROWS lanes work out what each row of the tile
// needs (the source row, its weight and whether a time mask covers it: the one float64 division per row position),
// and then all its lanes go over the tile's elements in row-major order.  A masked element is stored without a load.
// The values move as words of the row type's width: what is copied is copied bit for bit.

template <typename T> struct SpecaugWord;
template <> struct SpecaugWord<float> { typedef uint32_t type; };
template <> struct SpecaugWord<double> { typedef uint64_t type; };

// (in and out may be the same memory where no utterance is warped: an element is then read and written by one lane)
template <typename T>
__global__ __launch_bounds__(SPECAUG_THREADS) void specaug_apply_rows_kernel(
    const typename SpecaugWord<T>::type *in, int64_t in_stride, const int64_t *__restrict__ row_off,
    const int64_t *__restrict__ nrows, int64_t tiles, int64_t C, const int64_t *__restrict__ plan, int32_t freq_masks,
    int32_t time_masks, const double *__restrict__ mean, double fill, typename SpecaugWord<T>::type *out,
    int64_t out_stride) {
  typedef typename SpecaugWord<T>::type Word;
  __shared__ int64_t s_plan[SPECAUG_PLAN_MAX];
  __shared__ int64_t s_src[SPECAUG_ROWS];
  __shared__ double s_weight[SPECAUG_ROWS];
  __shared__ int32_t s_masked[SPECAUG_ROWS];
  const int64_t b = (int64_t)blockIdx.x / tiles, tile = (int64_t)blockIdx.x - b * tiles;
  const int64_t Tn = nrows[b];
  const int64_t t0 = tile * SPECAUG_ROWS;
  if (t0 >= Tn) return;  // (a shorter utterance of the batch, or an empty one: the same in the whole block)
  const int32_t words = specaug_plan_words(freq_masks, time_masks);
  if ((int32_t)threadIdx.x < words) s_plan[threadIdx.x] = plan[b * words + threadIdx.x];
  __syncthreads();
  const int32_t rows = (int32_t)(Tn - t0 < SPECAUG_ROWS ? Tn - t0 : SPECAUG_ROWS);
  if ((int32_t)threadIdx.x < rows) {
    const SpecaugRow row = specaug_row(t0 + threadIdx.x, Tn, s_plan, freq_masks, time_masks);
    s_src[threadIdx.x] = row.i;
    s_weight[threadIdx.x] = row.a;
    s_masked[threadIdx.x] = row.masked;
  }
  __syncthreads();
  const T filled = (T)(mean ? mean[b] : fill);  // rounded once to the row type
  const Word fill_word = __builtin_bit_cast(Word, filled);
  const int64_t r0 = row_off[b];
  const Word *x = in + r0 * in_stride;
  Word *y = out + (r0 + t0) * out_stride;
  specaug_tile_walk(threadIdx.x, rows, C, [&](int32_t r, int64_t c) {
    Word v = fill_word;
    if (!s_masked[r] && !specaug_column_masked(c, s_plan, freq_masks)) {
      const int64_t i = s_src[r];
      const double a = s_weight[r];
      v = x[i * in_stride + c];
      if (a != 0.0) {  // (i + 1 <= Tn - 1 here: specaug_row)
        const Word next = x[(i + 1) * in_stride + c];
        const double mixed = specaug_mix((double)__builtin_bit_cast(T, v), (double)__builtin_bit_cast(T, next), a);
        v = __builtin_bit_cast(Word, (T)mixed);
      }
    }
    y[r * out_stride + c] = v;
  });
}

template <typename T>
static int32_t launch_apply_rows(const T *d_in, int64_t in_stride, const int64_t *d_row_off, const int64_t *d_nrows,
                                 int32_t B, int32_t C, const int64_t *d_plan, int32_t freq_masks, int32_t time_masks,
                                 const double *d_mean, double fill, T *d_out, int64_t out_stride, int64_t max_rows,
                                 void *stream) {
  typedef typename SpecaugWord<T>::type Word;
  if (B < 0 || C <= 0 || max_rows < 0) return stages3_invalid("specaug_apply_rows: bad size");
  if (freq_masks < 0 || freq_masks > SPECAUG_MAX_MASKS || time_masks < 0 || time_masks > SPECAUG_MAX_MASKS)
    return stages3_invalid("specaug_apply_rows: freq_masks and time_masks must lie in [0, 16]");
  if (B == 0 || max_rows == 0) return PDS_STAGES3_OK;
  if (in_stride < C || out_stride < C) return stages3_invalid("specaug_apply_rows: a row stride is below C");
  const int64_t tiles = specaug_tiles(max_rows);
  const int64_t blocks = specaug_apply_blocks(B, tiles);
  if (blocks < 0) return stages3_invalid("specaug_apply_rows: too many blocks in one call (split the batch)");
  if (!d_in || !d_out || !d_row_off || !d_nrows || !d_plan) return stages3_invalid("specaug_apply_rows: null pointer");
  hipLaunchKernelGGL(specaug_apply_rows_kernel<T>, dim3((unsigned)blocks), dim3(SPECAUG_THREADS), 0,
                     (hipStream_t)stream, (const Word *)d_in, in_stride, d_row_off, d_nrows, tiles, (int64_t)C, d_plan,
                     freq_masks, time_masks, d_mean, fill, (Word *)d_out, out_stride);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return stages3_hip_fail(err, "specaug_apply_rows launch");
  return PDS_STAGES3_OK;
}

}  // namespace pds

extern "C" {

int32_t pds_stages3_version(void) { return 100; }

const char *pds_stages3_last_error(void) { return pds::g_stages3_error.c_str(); }

int32_t pds_specaug_tile_rows(void) { return pds::SPECAUG_ROWS; }

int32_t pds_specaug_plan(const int64_t *d_nrows, const int64_t *d_keys, int32_t B, int32_t C, int32_t freq_masks,
                         int64_t freq_width, int32_t time_masks, int64_t time_width, double time_ratio, int64_t warp,
                         int64_t *d_plan, void *stream) {
  using namespace pds;
  if (B < 0 || C <= 0) return stages3_invalid("specaug_plan: bad size");
  if (freq_masks < 0 || freq_masks > SPECAUG_MAX_MASKS || time_masks < 0 || time_masks > SPECAUG_MAX_MASKS)
    return stages3_invalid("specaug_plan: freq_masks and time_masks must lie in [0, 16]");
  if (freq_width < 0 || freq_width > SPECAUG_MAX_WIDTH || time_width < 0 || time_width > SPECAUG_MAX_WIDTH)
    return stages3_invalid("specaug_plan: freq_width and time_width must lie in [0, 2^31 - 2]");
  if (!(time_ratio > 0.0 && time_ratio <= 1.0)) return stages3_invalid("specaug_plan: time_ratio must lie in (0, 1]");
  if (warp < 0 || warp > SPECAUG_MAX_WARP) return stages3_invalid("specaug_plan: warp must lie in [0, 2^29]");
  if (B == 0) return PDS_STAGES3_OK;
  if (!d_nrows || !d_keys || !d_plan) return stages3_invalid("specaug_plan: null pointer");
  const int64_t blocks = specaug_plan_blocks(B);  // (B < 2^31: always a grid)
  hipLaunchKernelGGL(specaug_plan_kernel, dim3((unsigned)blocks), dim3(SPECAUG_THREADS), 0, (hipStream_t)stream,
                     d_nrows, d_keys, B, (int64_t)C, freq_masks, freq_width, time_masks, time_width, time_ratio, warp,
                     d_plan);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return stages3_hip_fail(err, "specaug_plan launch");
  return PDS_STAGES3_OK;
}

int32_t pds_specaug_mean_rows_f32(const float *d_in, int64_t in_stride, const int64_t *d_row_off,
                                  const int64_t *d_nrows, int32_t B, int32_t C, double *d_mean, void *stream) {
  return pds::launch_mean_rows<float>(d_in, in_stride, d_row_off, d_nrows, B, C, d_mean, stream);
}
int32_t pds_specaug_mean_rows_f64(const double *d_in, int64_t in_stride, const int64_t *d_row_off,
                                  const int64_t *d_nrows, int32_t B, int32_t C, double *d_mean, void *stream) {
  return pds::launch_mean_rows<double>(d_in, in_stride, d_row_off, d_nrows, B, C, d_mean, stream);
}

int32_t pds_specaug_apply_rows_f32(const float *d_in, int64_t in_stride, const int64_t *d_row_off,
                                   const int64_t *d_nrows, int32_t B, int32_t C, const int64_t *d_plan,
                                   int32_t freq_masks, int32_t time_masks, const double *d_mean, double fill,
                                   float *d_out, int64_t out_stride, int64_t max_rows, void *stream) {
  return pds::launch_apply_rows<float>(d_in, in_stride, d_row_off, d_nrows, B, C, d_plan, freq_masks, time_masks,
                                       d_mean, fill, d_out, out_stride, max_rows, stream);
}
int32_t pds_specaug_apply_rows_f64(const double *d_in, int64_t in_stride, const int64_t *d_row_off,
                                   const int64_t *d_nrows, int32_t B, int32_t C, const int64_t *d_plan,
                                   int32_t freq_masks, int32_t time_masks, const double *d_mean, double fill,
                                   double *d_out, int64_t out_stride, int64_t max_rows, void *stream) {
  return pds::launch_apply_rows<double>(d_in, in_stride, d_row_off, d_nrows, B, C, d_plan, freq_masks, time_masks,
                                        d_mean, fill, d_out, out_stride, max_rows, stream);
}

}  // extern "C"
