// libpds_amd_stages5.so: noise mixing at a drawn signal-to-noise ratio (pre.AddNoise) for gfx950, three kernel families
// over packed utterances.  Declarations and the definition of the arithmetic: include/pds_amd_stages5.h.  Built without
// contraction (Makefile): every float64 operation is rounded separately, as the definition says.  The library stands
// alone: its own version, its own error string, no header shared with the other five libraries.
//
// The forms.  mix_chunk_energy_kernel: one wave per chunk of 16384 samples of one segment, found by a binary search of
// the wave's number in the segments' chunk bases (wave-uniform); lane l adds the squares of samples l, l + 64, ... with
// MIX_AHEAD loads in flight, then the 64 partial sums fold by cross-lane moves in the definition's tree order.
// mix_gain_kernel: one lane per segment folds its chunk sums in order and writes E, P or the gain.  mix_apply_kernel: a
// bandwidth kernel, grid (sample blocks, utterances); a lane takes groups of MIX_VEC consecutive samples that stand on
// multiples of MIX_VEC of the buffer, so that where the buffers are aligned a group is one wide load and one wide
// store whatever the utterance's offset; adjacent lanes take adjacent groups, so a wave reads whole lines of the
// signal and (between wraps) of the noise.  The wrapped position is found once per lane and stepped from there.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/pds_amd_stages5.h"
#include "mix_rule.h"

namespace pds {

static thread_local std::string g_stages5_error;

static int32_t stages5_invalid(const char *msg) {
  g_stages5_error = msg;
  return PDS_STAGES5_ERR_INVALID;
}

static int32_t stages5_hip_fail(hipError_t err, const char *what) {
  g_stages5_error = std::string(what) + ": " + hipGetErrorString(err);
  return PDS_STAGES5_ERR_HIP;
}

// ---- segment energy -------------------------------------------------------------------------------------------------

template <typename T>
__global__ __launch_bounds__(MIX_ENERGY_WAVES *MIX_WAVE) void mix_chunk_energy_kernel(
    const T *__restrict__ x, const int64_t *__restrict__ offs, const int64_t *__restrict__ lens,
    const int64_t *__restrict__ chunk_base, int B, int64_t total_chunks, double *__restrict__ partials) {
  const int lane = threadIdx.x & (MIX_WAVE - 1);
  const int64_t w = (int64_t)blockIdx.x * MIX_ENERGY_WAVES + (threadIdx.x >> 6);
  if (w >= total_chunks) return;
  // the last segment whose base is not above w: the one with chunks there (empty segments share the base of the next)
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (chunk_base[mid] <= w) lo = mid; else hi = mid - 1;
  }
  const int64_t n = lens[lo];
  const int64_t c = w - chunk_base[lo];
  if (c < 0 || c >= mix_chunks(n)) return;  // (a table that does not go with the lengths: nothing is read)
  const T *seg = x + offs[lo];
  int64_t begin, end;
  mix_chunk_span(c, n, begin, end);
  double p = mix_lane_sum_ahead<T>([&](int64_t i) { return seg[i]; }, [](T v) { return (double)v; }, begin, end, lane);
  // the tree of the definition: p_l = p_l + p_{l + s} for l < s (the lanes at and above s add what nobody reads)
#pragma unroll
  for (int s = MIX_WAVE / 2; s >= 1; s >>= 1) p = p + __shfl_down(p, s, MIX_WAVE);
  if (lane == 0) partials[w] = p;
}

template <typename T>
static int32_t launch_chunk_energy(const T *d_x, const int64_t *d_off, const int64_t *d_len, const int64_t *d_chunk_base,
                                   int32_t B, int64_t total_chunks, double *d_partials, void *stream) {
  if (B < 0 || total_chunks < 0) return stages5_invalid("mix_chunk_energy: bad size");
  const int64_t blocks = mix_energy_blocks(total_chunks);
  if (blocks < 0) return stages5_invalid("mix_chunk_energy: more than 2^31 - 1 blocks in one call (split the batch)");
  if (B == 0 || total_chunks == 0) return PDS_STAGES5_OK;
  if (!d_x || !d_off || !d_len || !d_chunk_base || !d_partials) return stages5_invalid("mix_chunk_energy: null pointer");
  hipLaunchKernelGGL(mix_chunk_energy_kernel<T>, dim3((unsigned)blocks), dim3(MIX_ENERGY_WAVES * MIX_WAVE), 0,
                     (hipStream_t)stream, d_x, d_off, d_len, d_chunk_base, (int)B, total_chunks, d_partials);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return stages5_hip_fail(err, "mix_chunk_energy launch");
  return PDS_STAGES5_OK;
}

// ---- gain -----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(MIX_THREADS) void mix_gain_kernel(
    const double *__restrict__ partials, const int64_t *__restrict__ chunk_base, const int64_t *__restrict__ lens, int B,
    int mode, const int64_t *__restrict__ clip, const double *__restrict__ ratio, const int64_t *__restrict__ applied,
    const double *__restrict__ pn, int K, double *__restrict__ out) {
  const int64_t b = (int64_t)blockIdx.x * MIX_THREADS + threadIdx.x;
  if (b >= B) return;
  const int64_t n = lens[b];
  const double e = mix_fold(partials + chunk_base[b], mix_chunks(n));
  if (mode == 0) {
    out[b] = e;
  } else if (mode == 1) {
    out[b] = mix_power(e, n);
  } else {
    const int64_t j = clip[b];
    const bool known = j >= 0 && j < K;
    out[b] = mix_gain(known && applied[b] != 0, mix_power(e, n), known ? pn[j] : 0.0, ratio[b],
                      [](double q) { return __dsqrt_rn(q); });
  }
}

// ---- mix ------------------------------------------------------------------------------------------------------------

template <typename T>
struct MixVec {
  typedef T type __attribute__((ext_vector_type(MIX_VEC)));
};

template <typename TX> struct MixOut { typedef float type; };
template <> struct MixOut<double> { typedef double type; };

// one sample of the definition's sum: product and sum rounded separately, one rounding to TO
template <typename TX, typename TO>
__device__ __forceinline__ TO mix_one(TX x, double g, double z) {
  return (TO)__dadd_rn((double)x, __dmul_rn(g, z));
}

template <typename TX, typename TZ>
__global__ __launch_bounds__(MIX_THREADS) void mix_apply_kernel(
    const TX *__restrict__ x, const int64_t *__restrict__ offs, const int64_t *__restrict__ lens,
    const TZ *__restrict__ bank, const int64_t *__restrict__ clip_off, const int64_t *__restrict__ clip_len,
    const int64_t *__restrict__ start, const double *__restrict__ gain, int wide,
    typename MixOut<TX>::type *__restrict__ out) {
  typedef typename MixOut<TX>::type TO;
  typedef typename MixVec<TX>::type VX;
  typedef typename MixVec<TO>::type VO;
  const int b = blockIdx.y;
  const int64_t off = offs[b], n = lens[b];
  // the lane's first group: on a multiple of MIX_VEC of the buffer, at or up to MIX_VEC - 1 samples before the utterance
  int64_t t = (off & ~(int64_t)(MIX_VEC - 1)) - off + (int64_t)blockIdx.x * MIX_TILE + (int64_t)threadIdx.x * MIX_VEC;
  if (t >= n) return;
  const int64_t L = clip_len[b];
  const double g = L >= 1 ? gain[b] : 0.0;
  const TX *xs = x + off;
  TO *ys = out + off;
  if (g == 0.0) {  // copied (wave-uniform: g is the utterance's)
#pragma unroll 1
    for (int k = 0; k < MIX_ITERS; ++k, t += MIX_STRIDE) {
      if (t >= n) return;
      if (wide && t >= 0 && t + MIX_VEC <= n) {
        const VX v = *(const VX *)(xs + t);
        VO y;
#pragma unroll
        for (int e = 0; e < MIX_VEC; ++e) y[e] = (TO)v[e];
        *(VO *)(ys + t) = y;
      } else {
#pragma unroll
        for (int e = 0; e < MIX_VEC; ++e)
          if (t + e >= 0 && t + e < n) ys[t + e] = (TO)xs[t + e];
      }
    }
    return;
  }
  const TZ *z = bank + clip_off[b];
  // the one modulo of the lane (t >= -(MIX_VEC - 1), so MIX_VEC clip lengths keep the sum above zero), then steps
  // (whatever start holds, the position lies in [0, L): nothing is read outside the clip)
  int64_t pos = mix_wrap_first(start[b], t + MIX_VEC * L, L);
  const int64_t one = mix_wrap_stride(1, L), step = mix_wrap_stride(MIX_STRIDE, L);
#pragma unroll 1
  for (int k = 0; k < MIX_ITERS; ++k, t += MIX_STRIDE, pos = mix_wrap_step(pos, step, L)) {
    if (t >= n) return;
    int64_t p = pos;
    if (wide && t >= 0 && t + MIX_VEC <= n) {
      const VX v = *(const VX *)(xs + t);
      double zs[MIX_VEC];
#pragma unroll
      for (int e = 0; e < MIX_VEC; ++e, p = mix_wrap_step(p, one, L)) zs[e] = (double)z[p];
      VO y;
#pragma unroll
      for (int e = 0; e < MIX_VEC; ++e) y[e] = mix_one<TX, TO>(v[e], g, zs[e]);
      *(VO *)(ys + t) = y;
    } else {
#pragma unroll
      for (int e = 0; e < MIX_VEC; ++e, p = mix_wrap_step(p, one, L))
        if (t + e >= 0 && t + e < n) ys[t + e] = mix_one<TX, TO>(xs[t + e], g, (double)z[p]);
    }
  }
}

template <typename TX, typename TZ>
static int32_t launch_apply(const TX *d_x, const int64_t *d_off, const int64_t *d_len, const TZ *d_bank,
                            const int64_t *d_clip_off, const int64_t *d_clip_len, const int64_t *d_start,
                            const double *d_gain, int32_t B, int64_t max_len, typename MixOut<TX>::type *d_out,
                            void *stream) {
  typedef typename MixOut<TX>::type TO;
  if (B < 0 || max_len < 0) return stages5_invalid("mix_apply: bad size");
  if (B > MIX_MAX_UTTS) return stages5_invalid("mix_apply: more than 65535 utterances in one call (split the batch)");
  if (mix_apply_blocks(max_len, B) < 0)
    return stages5_invalid("mix_apply: more than 2^31 - 1 blocks in one call (split the batch)");
  if (B == 0 || max_len == 0) return PDS_STAGES5_OK;
  if (!d_x || !d_off || !d_len || !d_bank || !d_clip_off || !d_clip_len || !d_start || !d_gain || !d_out)
    return stages5_invalid("mix_apply: null pointer");
  // a group is one wide access where both buffers are aligned to it; else sample by sample
  const int wide = ((uintptr_t)d_x % (MIX_VEC * sizeof(TX)) == 0) && ((uintptr_t)d_out % (MIX_VEC * sizeof(TO)) == 0);
  hipLaunchKernelGGL((mix_apply_kernel<TX, TZ>), dim3((unsigned)mix_apply_blocks_x(max_len), (unsigned)B),
                     dim3(MIX_THREADS), 0, (hipStream_t)stream, d_x, d_off, d_len, d_bank, d_clip_off, d_clip_len,
                     d_start, d_gain, wide, d_out);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return stages5_hip_fail(err, "mix_apply launch");
  return PDS_STAGES5_OK;
}

}  // namespace pds

extern "C" {

int32_t pds_stages5_version(void) { return 100; }

const char *pds_stages5_last_error(void) { return pds::g_stages5_error.c_str(); }

int64_t pds_mix_chunk_samples(void) { return pds::MIX_CHUNK; }

int64_t pds_mix_chunk_count(int64_t n) { return pds::mix_chunks(n); }

int64_t pds_mix_tile_samples(void) { return pds::MIX_TILE; }

#define PDS_MIX_ENERGY(SUFFIX, T)                                                                                      \
  int32_t pds_mix_chunk_energy_##SUFFIX(const T *d_x, const int64_t *d_off, const int64_t *d_len,                      \
                                        const int64_t *d_chunk_base, int32_t B, int64_t total_chunks,                  \
                                        double *d_partials, void *stream) {                                            \
    return pds::launch_chunk_energy<T>(d_x, d_off, d_len, d_chunk_base, B, total_chunks, d_partials, stream);          \
  }
PDS_MIX_ENERGY(f32, float)
PDS_MIX_ENERGY(f64, double)
PDS_MIX_ENERGY(i16, int16_t)

int32_t pds_mix_gain(const double *d_partials, const int64_t *d_chunk_base, const int64_t *d_len, int32_t B,
                     int32_t mode, const int64_t *d_clip, const double *d_ratio, const int64_t *d_applied,
                     const double *d_pn, int32_t K, double *d_out, void *stream) {
  if (B < 0 || K < 0) return pds::stages5_invalid("mix_gain: bad size");
  if (mode < 0 || mode > 2) return pds::stages5_invalid("mix_gain: mode must be 0 (E), 1 (P) or 2 (gain)");
  if (B == 0) return PDS_STAGES5_OK;
  if (!d_partials || !d_chunk_base || !d_len || !d_out) return pds::stages5_invalid("mix_gain: null pointer");
  if (mode == 2 && (!d_clip || !d_ratio || !d_applied || !d_pn)) return pds::stages5_invalid("mix_gain: null pointer");
  hipLaunchKernelGGL(pds::mix_gain_kernel, dim3((unsigned)pds::mix_gain_blocks(B)), dim3(pds::MIX_THREADS), 0,
                     (hipStream_t)stream, d_partials, d_chunk_base, d_len, (int)B, (int)mode, d_clip, d_ratio, d_applied,
                     d_pn, (int)K, d_out);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return pds::stages5_hip_fail(err, "mix_gain launch");
  return PDS_STAGES5_OK;
}

#define PDS_MIX_APPLY(XS, TX, ZS, TZ, TO)                                                                              \
  int32_t pds_mix_apply_##XS##_##ZS(const TX *d_x, const int64_t *d_off, const int64_t *d_len, const TZ *d_bank,       \
                                    const int64_t *d_clip_off, const int64_t *d_clip_len, const int64_t *d_start,      \
                                    const double *d_gain, int32_t B, int64_t max_len, TO *d_out, void *stream) {       \
    return pds::launch_apply<TX, TZ>(d_x, d_off, d_len, d_bank, d_clip_off, d_clip_len, d_start, d_gain, B, max_len,   \
                                     d_out, stream);                                                                   \
  }
PDS_MIX_APPLY(f32, float, f32, float, float)
PDS_MIX_APPLY(f32, float, f64, double, float)
PDS_MIX_APPLY(f32, float, i16, int16_t, float)
PDS_MIX_APPLY(f64, double, f32, float, double)
PDS_MIX_APPLY(f64, double, f64, double, double)
PDS_MIX_APPLY(f64, double, i16, int16_t, double)
PDS_MIX_APPLY(i16, int16_t, f32, float, float)
PDS_MIX_APPLY(i16, int16_t, f64, double, float)
PDS_MIX_APPLY(i16, int16_t, i16, int16_t, float)

}  // extern "C"
