// libpds_amd_stages6.so: room impulse response convolution (pre.Reverb) for gfx950, three kernel families over packed
// utterances.  Declarations and the definition: include/pds_amd_stages6.h; the counting: reverb_rule.h.  The library
// stands alone: its own version, its own error string, no header shared with the other six libraries but the stateless
// in-lane transform templates (fft_inlane.h, twiddle_consts.h).
//
// The forms.  A 1024-point complex transform lives in half a wave, 32 lanes x 32 registers, element n in lane n % 32,
// register n / 32: an in-lane transform over the register index, the twiddle W_1024^(lane q) from an LDS table, a
// transposition through the half wave's own LDS area, an in-lane transform again.  The result has the layout of the
// input (bin k in lane k % 32, register k / 32), so spectra are stored and read in natural order, a half wave's row
// being 256 contiguous bytes, and the inverse transform is the same routine between two conjugations.  (This is the
// form of si_fft.hip, restated: that file belongs to another library.)
//
// reverb_spectra_kernel<T>: one half wave per spectrum of an utterance; the stretch of block k goes into the real part
// and that of block k + 1 into the imaginary part, so that one inverse transform later yields two blocks without any
// untangling.  reverb_convolve_kernel: one half wave per pair of blocks of y_full; it adds Z_{k - p} H_p in ascending p
// into 64 registers, the loads of the next partition issued before the multiply-adds of the current one, runs one
// inverse transform and stores elements 512 .. 1023 shifted by -d: the real part at block k, the imaginary part at
// block k + 1.  The units of an utterance are neighbours in the grid (a flat grid, the utterance found by a binary
// search), so its spectra and its response's are read from L2.  An utterance that is not applied is copied by the same
// kernel, 1024 samples per half wave, and so is one whose response has a single tap (a delay and a gain: no transform);
// both halves of a wave serve one utterance, so the branch is wave-uniform.
// reverb_scale_kernel: the normalisation product in place, four samples a lane where the buffer is aligned.
// No atomics; LDS holds the transposition areas and the twiddle table only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/pds_amd_stages6.h"
#include "fft_inlane.h"
#include "reverb_rule.h"

namespace pds {

static thread_local std::string g_stages6_error;

static int32_t stages6_invalid(const char *msg) {
  g_stages6_error = msg;
  return PDS_STAGES6_ERR_INVALID;
}

static int32_t stages6_hip_fail(hipError_t err, const char *what) {
  g_stages6_error = std::string(what) + ": " + hipGetErrorString(err);
  return PDS_STAGES6_ERR_HIP;
}

namespace {

constexpr int kL = 32;  // lanes = registers of a transform
constexpr int kRow = REVERB_ROW_STRIDE;
constexpr int kTwBatch = 16;  // twiddle rows read from LDS at a time

__device__ __forceinline__ void half_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// (zr, zi)[q] = element 32 q + l  ->  (zr, zi)[q] = bin 32 q + l of the 1024-point DFT; tw[q * 32 + l] = W_1024^(l q)
__device__ __forceinline__ void fft1024(float (&zr)[kL], float (&zi)[kL], float2 *xch, const float2 *tw, int l) {
  float ar[kL], ai[kL];
  inl::CFFT<kL, 1>::run(zr, zi, ar, ai);
#pragma unroll
  for (int q0 = 0; q0 < kL; q0 += kTwBatch) {
    float tr[kTwBatch], ti[kTwBatch];
#pragma unroll
    for (int i = 0; i < kTwBatch; ++i) {
      const float2 t = tw[(q0 + i) * kL + l];
      tr[i] = t.x;
      ti[i] = t.y;
    }
#pragma unroll
    for (int i = 0; i < kTwBatch; ++i) {
      const int q = q0 + i;
      float2 v;
      v.x = ar[q] * tr[i] - ai[q] * ti[i];
      v.y = ar[q] * ti[i] + ai[q] * tr[i];
      xch[q * kRow + l] = v;
    }
  }
  half_wave_sync();
#pragma unroll
  for (int q = 0; q < kL; ++q) {
    const float2 v = xch[l * kRow + q];
    ar[q] = v.x;
    ai[q] = v.y;
  }
  half_wave_sync();
  inl::CFFT<kL, 1>::run(ar, ai, zr, zi);
}

// the areas of a block: [REVERB_HALVES][32][33] transposition, [32][32] twiddles
struct ReverbLds {
  float2 xch[REVERB_HALVES * kL * kRow];
  float2 tw[kL * kL];
};

__device__ __forceinline__ void stage_twiddles(ReverbLds &lds, const float2 *__restrict__ twiddle) {
  for (int i = threadIdx.x; i < kL * kL; i += REVERB_THREADS) lds.tw[i] = twiddle[i];
  __syncthreads();
}

template <typename T> __device__ __forceinline__ float to_f32(T v) { return (float)v; }

// ---- spectra --------------------------------------------------------------------------------------------------------

template <typename T>
__global__ __launch_bounds__(REVERB_THREADS) void reverb_spectra_kernel(
    const T *__restrict__ x, const int64_t *__restrict__ offs, const int64_t *__restrict__ lens,
    const int64_t *__restrict__ rir, const int64_t *__restrict__ spec_base, int B, int64_t total,
    const float2 *__restrict__ twiddle, float2 *__restrict__ ws) {
  __shared__ ReverbLds lds;
  stage_twiddles(lds, twiddle);
  const int half = threadIdx.x >> 5, l = threadIdx.x & 31;
  const int64_t u = (int64_t)blockIdx.x * REVERB_HALVES + half;
  if (u >= total) return;
  const int b = reverb_find(spec_base, B, u & ~(int64_t)1);  // (the wave's utterance: units come in twos)
  const int64_t n = lens[b];
  const int64_t slot = u - spec_base[b];
  if (rir[b] < 0 || slot < 0 || slot >= reverb_spectra(n)) return;  // (the padding unit, or a table that does not fit)
  const int64_t k = slot - 1;
  const T *seg = x + offs[b];
  float zr[kL], zi[kL];
#pragma unroll
  for (int q = 0; q < kL; ++q) {
    const int64_t ir = reverb_stretch_re(k, kL * q + l), ii = reverb_stretch_im(k, kL * q + l);
    zr[q] = reverb_inside(ir, n) ? to_f32<T>(seg[ir]) : 0.0f;
    zi[q] = reverb_inside(ii, n) ? to_f32<T>(seg[ii]) : 0.0f;
  }
  fft1024(zr, zi, lds.xch + half * kL * kRow, lds.tw, l);
  float2 *dst = ws + u * REVERB_FFT + l;
#pragma unroll
  for (int q = 0; q < kL; ++q) dst[q * kL] = make_float2(zr[q], zi[q]);
}

template <typename T>
static int32_t launch_spectra(const T *d_x, const int64_t *d_off, const int64_t *d_len, const int64_t *d_rir,
                              const int64_t *d_spec_base, int32_t B, int64_t total, const float *d_twiddle, float *d_ws,
                              void *stream) {
  if (B < 0 || total < 0) return stages6_invalid("reverb_spectra: bad size");
  const int64_t blocks = reverb_blocks(total);
  if (blocks < 0) return stages6_invalid("reverb_spectra: more than 2^31 - 1 blocks in one call (split the batch)");
  if (B == 0 || total == 0) return PDS_STAGES6_OK;
  if (!d_x || !d_off || !d_len || !d_rir || !d_spec_base || !d_twiddle || !d_ws)
    return stages6_invalid("reverb_spectra: null pointer");
  hipLaunchKernelGGL(reverb_spectra_kernel<T>, dim3((unsigned)blocks), dim3(REVERB_THREADS), 0, (hipStream_t)stream,
                     d_x, d_off, d_len, d_rir, d_spec_base, (int)B, total, (const float2 *)d_twiddle, (float2 *)d_ws);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return stages6_hip_fail(err, "reverb_spectra launch");
  return PDS_STAGES6_OK;
}

// ---- convolve -------------------------------------------------------------------------------------------------------

struct ReverbConvArgs {
  const void *x;
  int xtype;
  const int64_t *offs, *lens, *rir, *spec_base, *unit_base;
  int B;
  int64_t total;
  const float2 *ws, *h;
  const int64_t *rir_base, *rir_parts, *rir_peak, *rir_tap;
  const float *rir_gain;
  int K;
  const float2 *twiddle;
  float *out;
};

template <typename T>
__device__ __forceinline__ void copy_stretch(const T *__restrict__ src, float *__restrict__ dst, int64_t begin,
                                             int64_t n, int l) {
#pragma unroll 4
  for (int q = 0; q < kL; ++q) {
    const int64_t t = begin + kL * q + l;
    if (t < n) dst[t] = to_f32<T>(src[t]);
  }
}

// a response of one tap g at k0: wet[t] = g x[t + s] with s = d - k0, zero where that leaves the utterance
template <typename T>
__device__ __forceinline__ void delay_stretch(const T *__restrict__ src, float *__restrict__ dst, int64_t begin,
                                              int64_t n, int64_t s, float g, int l) {
#pragma unroll 4
  for (int q = 0; q < kL; ++q) {
    const int64_t t = begin + kL * q + l;
    if (t < n) dst[t] = reverb_inside(t + s, n) ? g * to_f32<T>(src[t + s]) : 0.0f;
  }
}

__global__ __launch_bounds__(REVERB_THREADS) void reverb_convolve_kernel(const ReverbConvArgs a) {
  __shared__ ReverbLds lds;
  stage_twiddles(lds, a.twiddle);
  const int half = threadIdx.x >> 5, l = threadIdx.x & 31;
  const int64_t u = (int64_t)blockIdx.x * REVERB_HALVES + half;
  if (u >= a.total) return;
  const int b = reverb_find(a.unit_base, a.B, u & ~(int64_t)1);  // (the wave's utterance: units come in twos)
  const int64_t n = a.lens[b], off = a.offs[b];
  const int64_t unit = u - a.unit_base[b];
  const int64_t j = a.rir[b];
  float *ys = a.out + off;
  if (unit < 0) return;
  const bool known = j >= 0 && j < a.K;
  const int64_t tap = known ? a.rir_tap[j] : -1;
  if (!known || tap >= 0) {  // not applied: copied; one tap: a delay and a gain (wave-uniform: j is the utterance's)
    const int64_t begin = unit * REVERB_FFT;
    if (begin >= n) return;
    if (known) {
      const int64_t s = a.rir_peak[j] - tap;
      const float g = a.rir_gain[j];
      if (a.xtype == 0) delay_stretch<float>((const float *)a.x + off, ys, begin, n, s, g, l);
      else if (a.xtype == 1) delay_stretch<double>((const double *)a.x + off, ys, begin, n, s, g, l);
      else delay_stretch<int16_t>((const int16_t *)a.x + off, ys, begin, n, s, g, l);
    } else if (a.xtype == 0) {
      // (bytes, not values: a NaN's payload must not pass through a conversion)
      const uint32_t *src = (const uint32_t *)a.x + off;
      uint32_t *dst = (uint32_t *)ys;
#pragma unroll 4
      for (int q = 0; q < kL; ++q) {
        const int64_t t = begin + kL * q + l;
        if (t < n) dst[t] = src[t];
      }
    } else if (a.xtype == 1) {
      copy_stretch<double>((const double *)a.x + off, ys, begin, n, l);
    } else {
      copy_stretch<int16_t>((const int16_t *)a.x + off, ys, begin, n, l);
    }
    return;
  }
  const int64_t d = a.rir_peak[j], P = a.rir_parts[j];
  if (unit >= reverb_pairs(n, d)) return;  // (the padding unit)
  const int64_t k = 2 * (reverb_first_pair(d) + unit);
  const int64_t p_lo = reverb_first_part(k, n), p_hi = reverb_last_part(k, P);
  // spectrum k - p of the utterance lies in slot k - p + 1; response partition p in slot rir_base + p
  const float2 *zb = a.ws + (a.spec_base[b] + k + 1) * REVERB_FFT + l;
  const float2 *hb = a.h + a.rir_base[j] * REVERB_FFT + l;
  float accr[kL], acci[kL];
#pragma unroll
  for (int q = 0; q < kL; ++q) accr[q] = acci[q] = 0.0f;
  float2 za[kL], ha[kL], zn[kL], hn[kL];
  auto load = [&](float2 (&z)[kL], float2 (&h)[kL], int64_t p) {
    const float2 *zp = zb - p * REVERB_FFT, *hp = hb + p * REVERB_FFT;
#pragma unroll
    for (int q = 0; q < kL; ++q) z[q] = zp[q * kL];
#pragma unroll
    for (int q = 0; q < kL; ++q) h[q] = hp[q * kL];
  };
  auto mac = [&](const float2 (&z)[kL], const float2 (&h)[kL]) {
#pragma unroll
    for (int q = 0; q < kL; ++q) {
      accr[q] = fmaf(-z[q].y, h[q].y, fmaf(z[q].x, h[q].x, accr[q]));
      acci[q] = fmaf(z[q].y, h[q].x, fmaf(z[q].x, h[q].y, acci[q]));
    }
  };
  if (p_lo <= p_hi) load(za, ha, p_lo);
#pragma unroll 1
  for (int64_t p = p_lo; p <= p_hi; p += 2) {
    const bool second = p + 1 <= p_hi;
    if (second) load(zn, hn, p + 1);
    mac(za, ha);
    if (second) {
      if (p + 2 <= p_hi) load(za, ha, p + 2);
      mac(zn, hn);
    }
  }
  // the inverse transform: conj(FFT(conj(Y))), 1 / 1024 at the store (a power of two)
#pragma unroll
  for (int q = 0; q < kL; ++q) acci[q] = -acci[q];
  fft1024(accr, acci, lds.xch + half * kL * kRow, lds.tw, l);
  int64_t b0, e0, b1, e1;
  reverb_block_out(k, n, d, b0, e0);
  reverb_block_out(k + 1, n, d, b1, e1);
  const float scale = 1.0f / 1024.0f;
  // element 512 + 32 q + l: tau = 512 k + 32 q + l (real part), 512 (k + 1) + 32 q + l (imaginary part)
  const int64_t t0 = k * REVERB_BLOCK - d + l;
#pragma unroll
  for (int q = 0; q < kL / 2; ++q) {
    const int64_t t = t0 + kL * q;
    if (t >= b0 && t < e0) ys[t] = accr[q + kL / 2] * scale;
  }
#pragma unroll
  for (int q = 0; q < kL / 2; ++q) {
    const int64_t t = t0 + REVERB_BLOCK + kL * q;
    if (t >= b1 && t < e1) ys[t] = -acci[q + kL / 2] * scale;
  }
}

// ---- scale ----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(REVERB_SCALE_THREADS) void reverb_scale_kernel(
    float *__restrict__ out, const int64_t *__restrict__ offs, const int64_t *__restrict__ lens,
    const double *__restrict__ gain, int wide) {
  typedef float V4 __attribute__((ext_vector_type(REVERB_SCALE_VEC)));
  const int b = blockIdx.y;
  const double c = gain[b];
  if (c == 0.0) return;  // "leave" (the utterance's: wave-uniform)
  const int64_t off = offs[b], n = lens[b];
  int64_t t = (off & ~(int64_t)(REVERB_SCALE_VEC - 1)) - off + (int64_t)blockIdx.x * REVERB_SCALE_TILE +
              (int64_t)threadIdx.x * REVERB_SCALE_VEC;
  float *ys = out + off;
#pragma unroll 1
  for (int k = 0; k < REVERB_SCALE_ITERS; ++k, t += REVERB_SCALE_STRIDE) {
    if (t >= n) return;
    if (wide && t >= 0 && t + REVERB_SCALE_VEC <= n) {
      V4 v = *(const V4 *)(ys + t);
#pragma unroll
      for (int e = 0; e < REVERB_SCALE_VEC; ++e) v[e] = (float)__dmul_rn((double)v[e], c);
      *(V4 *)(ys + t) = v;
    } else {
#pragma unroll
      for (int e = 0; e < REVERB_SCALE_VEC; ++e)
        if (t + e >= 0 && t + e < n) ys[t + e] = (float)__dmul_rn((double)ys[t + e], c);
    }
  }
}

}  // namespace

}  // namespace pds

extern "C" {

int32_t pds_stages6_version(void) { return 100; }

const char *pds_stages6_last_error(void) { return pds::g_stages6_error.c_str(); }

int64_t pds_reverb_block_samples(void) { return pds::REVERB_BLOCK; }

int64_t pds_reverb_max_taps(void) { return pds::REVERB_MAX_TAPS; }

int64_t pds_reverb_partitions(int64_t L) {
  if (L < 1 || L > pds::REVERB_MAX_TAPS) {
    pds::stages6_invalid("reverb_partitions: a response has 1 to 2^20 taps");
    return -1;
  }
  return pds::reverb_partitions(L);
}

int64_t pds_reverb_spectra_units(int64_t n) { return pds::reverb_spectra_units(n, true); }

int64_t pds_reverb_convolve_units(int64_t n, int64_t d, int32_t transformed) {
  return pds::reverb_convolve_units(n, d < 0 ? 0 : d, transformed != 0);
}

int64_t pds_reverb_workspace_bytes(int64_t units) { return pds::reverb_workspace_bytes(units); }

int32_t pds_reverb_twiddles(float *host_out) {
  if (!host_out) return pds::stages6_invalid("reverb_twiddles: null pointer");
  for (int q = 0; q < 32; ++q)
    for (int l = 0; l < 32; ++l) {
      const double a = -2.0 * M_PI * (double)(q * l) / 1024.0;
      host_out[2 * (q * 32 + l)] = (float)cos(a);
      host_out[2 * (q * 32 + l) + 1] = (float)sin(a);
    }
  return PDS_STAGES6_OK;
}

#define PDS_REVERB_SPECTRA(SUFFIX, T)                                                                                  \
  int32_t pds_reverb_spectra_##SUFFIX(const T *d_x, const int64_t *d_off, const int64_t *d_len, const int64_t *d_rir,  \
                                      const int64_t *d_spec_base, int32_t B, int64_t total_units,                      \
                                      const float *d_twiddle, float *d_workspace, void *stream) {                      \
    return pds::launch_spectra<T>(d_x, d_off, d_len, d_rir, d_spec_base, B, total_units, d_twiddle, d_workspace,       \
                                  stream);                                                                             \
  }
PDS_REVERB_SPECTRA(f32, float)
PDS_REVERB_SPECTRA(f64, double)
PDS_REVERB_SPECTRA(i16, int16_t)

int32_t pds_reverb_convolve(const void *d_x, int32_t xtype, const int64_t *d_off, const int64_t *d_len,
                            const int64_t *d_rir, const int64_t *d_spec_base, const int64_t *d_unit_base, int32_t B,
                            int64_t total_units, const float *d_workspace, const float *d_h, const int64_t *d_rir_base,
                            const int64_t *d_rir_parts, const int64_t *d_rir_peak, const int64_t *d_rir_tap,
                            const float *d_rir_gain, int32_t K, const float *d_twiddle, float *d_out, void *stream) {
  using namespace pds;
  if (B < 0 || total_units < 0 || K < 0) return stages6_invalid("reverb_convolve: bad size");
  if (xtype < 0 || xtype > 2) return stages6_invalid("reverb_convolve: xtype must be 0 (f32), 1 (f64) or 2 (i16)");
  const int64_t blocks = reverb_blocks(total_units);
  if (blocks < 0) return stages6_invalid("reverb_convolve: more than 2^31 - 1 blocks in one call (split the batch)");
  if (B == 0 || total_units == 0) return PDS_STAGES6_OK;
  if (!d_x || !d_off || !d_len || !d_rir || !d_spec_base || !d_unit_base || !d_twiddle || !d_out)
    return stages6_invalid("reverb_convolve: null pointer");
  if (K > 0 && (!d_h || !d_rir_base || !d_rir_parts || !d_rir_peak || !d_rir_tap || !d_rir_gain))
    return stages6_invalid("reverb_convolve: null pointer");
  ReverbConvArgs a;
  a.x = d_x; a.xtype = xtype; a.offs = d_off; a.lens = d_len; a.rir = d_rir; a.spec_base = d_spec_base;
  a.unit_base = d_unit_base; a.B = B; a.total = total_units; a.ws = (const float2 *)d_workspace;
  a.h = (const float2 *)d_h; a.rir_base = d_rir_base; a.rir_parts = d_rir_parts; a.rir_peak = d_rir_peak; a.rir_tap = d_rir_tap;
  a.rir_gain = d_rir_gain; a.K = K;
  a.twiddle = (const float2 *)d_twiddle; a.out = d_out;
  hipLaunchKernelGGL(reverb_convolve_kernel, dim3((unsigned)blocks), dim3(REVERB_THREADS), 0, (hipStream_t)stream, a);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return stages6_hip_fail(err, "reverb_convolve launch");
  return PDS_STAGES6_OK;
}

int32_t pds_reverb_scale(float *d_out, const int64_t *d_off, const int64_t *d_len, const double *d_gain, int32_t B,
                         int64_t max_len, void *stream) {
  using namespace pds;
  if (B < 0 || max_len < 0) return stages6_invalid("reverb_scale: bad size");
  if (B > REVERB_MAX_UTTS) return stages6_invalid("reverb_scale: more than 65535 utterances in one call (split the batch)");
  if (reverb_scale_blocks(max_len, B) < 0)
    return stages6_invalid("reverb_scale: more than 2^31 - 1 blocks in one call (split the batch)");
  if (B == 0 || max_len == 0) return PDS_STAGES6_OK;
  if (!d_out || !d_off || !d_len || !d_gain) return stages6_invalid("reverb_scale: null pointer");
  const int wide = (uintptr_t)d_out % (REVERB_SCALE_VEC * sizeof(float)) == 0;
  hipLaunchKernelGGL(reverb_scale_kernel, dim3((unsigned)reverb_scale_blocks_x(max_len), (unsigned)B),
                     dim3(REVERB_SCALE_THREADS), 0, (hipStream_t)stream, d_out, d_off, d_len, d_gain, wide);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return stages6_hip_fail(err, "reverb_scale launch");
  return PDS_STAGES6_OK;
}

}  // extern "C"
