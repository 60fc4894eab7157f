// Pre-processor kernels: Preemphasize (reference pre.py:103-149) and Dither (pre.py:67-100).
// Element-wise, HBM-bound; intermediate arithmetic in float64 like the reference, result cast
// back to the signal's type.  The STFT kernels can also apply pre-emphasis while loading frames
// (pds_stft_batch_*'s `preemph` argument), which saves this pass over the signal.
#include "pds_internal.h"
#include "dither_noise.h"

namespace pds {

static int32_t invalid_pre(const char *msg) {
  set_error(msg);
  return PDS_ERR_INVALID;
}

// packed utterances: new[i] = old[i] - coeff * old[i-1] for i >= 1, new[0] = old[0], per utterance
template <typename T>
__global__ __launch_bounds__(256) void preemph_kernel(const T *__restrict__ in,
                                                      const int64_t *__restrict__ offsets,
                                                      const int64_t *__restrict__ lengths,
                                                      double coeff, T *__restrict__ out) {
  const int b = blockIdx.y;
  const int64_t n = lengths[b];
  const T *x = in + offsets[b];
  T *y = out + offsets[b];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    double v = (double)x[i];
    if (i > 0) v = __dsub_rn(v, __dmul_rn(coeff, (double)x[i - 1]));
    y[i] = (T)v;
  }
}

// out[i] = in[i] + coeff * N(0, 1); one thread per 2 samples (one Box-Muller pair from 53+53 bits, dither_noise.h)
template <typename T>
__global__ __launch_bounds__(256) void dither_kernel(const T *__restrict__ in, int64_t total,
                                                     double coeff, uint64_t seed,
                                                     T *__restrict__ out) {
  const int64_t pairs = (total + 1) / 2;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < pairs;
       q += (int64_t)gridDim.x * blockDim.x) {
    double even, odd;
    dither_pair(q, seed, coeff, even, odd);
    const int64_t i = 2 * q;
    out[i] = dither_add<T>((double)in[i], even);
    if (i + 1 < total) out[i + 1] = dither_add<T>((double)in[i + 1], odd);
  }
}

// packed utterances, one launch: utterance b (blockIdx.y) is in[offsets[b] .. + lengths[b]) and takes the noise of
// dither_kernel over it alone under seed keys[b] -- pair q of the utterance is its samples 2q and 2q + 1, whatever the
// parity of offsets[b]; the last sample of an odd length takes the cosine branch of its pair alone.  `i16`: `in` holds
// 16-bit PCM, widened at the load, exactly (a launch-wide flag: a kernel of its own would be one more copy of the noise
// arithmetic for the sake of one load)
template <typename T>
__global__ __launch_bounds__(256) void dither_packed_kernel(const void *__restrict__ in, int32_t i16,
                                                            const int64_t *__restrict__ offsets,
                                                            const int64_t *__restrict__ lengths,
                                                            const uint64_t *__restrict__ keys, double coeff,
                                                            T *__restrict__ out) {
  const int b = blockIdx.y;
  const int64_t n = lengths[b], off = offsets[b];
  T *y = out + off;
  const uint64_t key = keys[b];
  const int64_t pairs = (n + 1) / 2;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < pairs;
       q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = 2 * q;
    const bool both = i + 1 < n;
    T x0, x1 = T(0);  // (the loads before the arithmetic)
    if (i16) {
      const int16_t *x = (const int16_t *)in + off;
      x0 = (T)x[i];
      if (both) x1 = (T)x[i + 1];
    } else {
      const T *x = (const T *)in + off;
      x0 = x[i];
      if (both) x1 = x[i + 1];
    }
    double even, odd;
    dither_pair(q, key, coeff, even, odd);
    y[i] = dither_add<T>((double)x0, even);
    if (both) y[i + 1] = dither_add<T>((double)x1, odd);
  }
}

template <typename T>
static int32_t launch_preemph(const T *d_in, const int64_t *d_off, const int64_t *d_len, int32_t B,
                              int64_t max_len, double coeff, T *d_out, void *stream) {
  if (B < 0 || max_len < 0) return invalid_pre("preemphasize: negative size");
  if (B == 0 || max_len == 0) return PDS_OK;
  if (B > 65535) return invalid_pre("preemphasize: B > 65535");
  if (!d_in || !d_off || !d_len || !d_out) return invalid_pre("preemphasize: null pointer");
  int64_t blocks = (max_len + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(preemph_kernel<T>, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, d_in, d_off, d_len, coeff, d_out);
  PDS_HIP(hipGetLastError());
  return PDS_OK;
}

template <typename T>
static int32_t launch_dither(const T *d_in, int64_t total, double coeff, uint64_t seed, T *d_out,
                             void *stream) {
  if (total < 0) return invalid_pre("dither: negative size");
  if (total == 0) return PDS_OK;
  if (!d_in || !d_out) return invalid_pre("dither: null pointer");
  int64_t blocks = ((total + 1) / 2 + 255) / 256;
  if (blocks > 65536 * 4) blocks = 65536 * 4;
  hipLaunchKernelGGL(dither_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     d_in, total, coeff, seed, d_out);
  PDS_HIP(hipGetLastError());
  return PDS_OK;
}

template <typename T>
static int32_t launch_dither_packed(const void *d_in, bool i16, const int64_t *d_off, const int64_t *d_len,
                                    const uint64_t *d_keys, int32_t B, int64_t max_len, double coeff,
                                    T *d_out, void *stream) {
  if (B < 0 || max_len < 0) return invalid_pre("dither_packed: negative size");
  if (B == 0 || max_len == 0) return PDS_OK;
  if (B > 65535) return invalid_pre("dither_packed: B > 65535");
  if (!d_in || !d_off || !d_len || !d_keys || !d_out) return invalid_pre("dither_packed: null pointer");
  if (i16 && (const void *)d_out == d_in) return invalid_pre("dither_packed: int16 samples cannot be dithered in place");
  int64_t blocks = ((max_len + 1) / 2 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(dither_packed_kernel<T>, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, d_in, (int32_t)i16, d_off, d_len, d_keys, coeff, d_out);
  PDS_HIP(hipGetLastError());
  return PDS_OK;
}

}  // namespace pds

extern "C" {

int32_t pds_preemphasize_f32(const float *d_in, const int64_t *d_offsets, const int64_t *d_lengths,
                             int32_t B, int64_t max_len, double coeff, float *d_out, void *stream) {
  return pds::launch_preemph<float>(d_in, d_offsets, d_lengths, B, max_len, coeff, d_out, stream);
}
int32_t pds_preemphasize_f64(const double *d_in, const int64_t *d_offsets,
                             const int64_t *d_lengths, int32_t B, int64_t max_len, double coeff,
                             double *d_out, void *stream) {
  return pds::launch_preemph<double>(d_in, d_offsets, d_lengths, B, max_len, coeff, d_out, stream);
}
int32_t pds_dither_f32(const float *d_in, int64_t total, double coeff, uint64_t seed, float *d_out,
                       void *stream) {
  return pds::launch_dither<float>(d_in, total, coeff, seed, d_out, stream);
}
int32_t pds_dither_f64(const double *d_in, int64_t total, double coeff, uint64_t seed,
                       double *d_out, void *stream) {
  return pds::launch_dither<double>(d_in, total, coeff, seed, d_out, stream);
}

int32_t pds_dither_packed_f32(const float *d_in, const int64_t *d_offsets, const int64_t *d_lengths,
                              const uint64_t *d_keys, int32_t B, int64_t max_len, double coeff,
                              float *d_out, void *stream) {
  return pds::launch_dither_packed<float>(d_in, false, d_offsets, d_lengths, d_keys, B, max_len, coeff,
                                          d_out, stream);
}
int32_t pds_dither_packed_f64(const double *d_in, const int64_t *d_offsets, const int64_t *d_lengths,
                              const uint64_t *d_keys, int32_t B, int64_t max_len, double coeff,
                              double *d_out, void *stream) {
  return pds::launch_dither_packed<double>(d_in, false, d_offsets, d_lengths, d_keys, B, max_len, coeff,
                                           d_out, stream);
}
int32_t pds_dither_packed_i16_f32(const int16_t *d_in, const int64_t *d_offsets,
                                  const int64_t *d_lengths, const uint64_t *d_keys, int32_t B,
                                  int64_t max_len, double coeff, float *d_out, void *stream) {
  return pds::launch_dither_packed<float>(d_in, true, d_offsets, d_lengths, d_keys, B, max_len, coeff,
                                          d_out, stream);
}

}  // extern "C"
