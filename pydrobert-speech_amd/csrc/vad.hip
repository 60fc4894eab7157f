// libpds_amd_stages.so: the energy VAD for gfx950 over packed ragged batches -- Kaldi's voiced-frame decision
// (compute-vad-energy) and the order-preserving selection of the kept rows (select-voiced-frames).
// Declarations and the definition of the arithmetic: include/pds_amd_stages.h; the rule itself: vad_rule.h.
// Built without contraction (Makefile): every float64 operation is rounded separately, as the definition says.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pds_amd_stages.h"
#include "stages_internal.h"
#include "vad_rule.h"

namespace pds {

constexpr int VD_WAVE = 64;
constexpr int VD_THREADS = 256;                    // the decision: four waves, each with an utterance of its own
constexpr int VD_WAVES = VD_THREADS / VD_WAVE;
constexpr int VD_AHEAD = 4;                        // loads in flight per lane (sums and ballots are sequential, loads are not)
constexpr int SEL_THREADS = 256;                   // the selection: a block takes a tile of this many rows
constexpr int SEL_WAVES = SEL_THREADS / VD_WAVE;
constexpr int64_t SEL_COLS = (int64_t)1 << 20;     // words of a row copied per pass: rows x words of a pass fit 32 bits

// the float64 `v` of lane j (j the same in every lane), in every lane
__device__ __forceinline__ double lane_value(double v, int j) {
  const uint64_t bits = (uint64_t)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)bits, j);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(bits >> 32), j);
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// ---- the decision: one wave per utterance ---------------------------------------------------------------------------
//
// Lane j owns partial sum j (its energies are those a wave loads together), the 64 partials are added in lane order by
// every lane alike, and the vote goes over the utterance in chunks of 64 frames, lane l taking frame t = t0 + l.  The
// number of frames above the threshold in t's window [lo, hi] is a difference of two running counts,
//     above[0, hi] - above[0, lo),
// and both ends move with t: the chunk's lanes look at the 64 frames t + context (past the end: nothing) and at the 64
// frames t - context (before the start: nothing), a ballot of each gives the counts inside the chunk and two wave-wide
// bases carry them from chunk to chunk.  Two loads per frame whatever the context.

template <typename T>
__global__ __launch_bounds__(VD_THREADS) void vad_energy_kernel(
    const T *__restrict__ energy, int64_t stride, const int64_t *__restrict__ row_off,
    const int64_t *__restrict__ nrows, int32_t B, double energy_threshold, double energy_mean_scale, int64_t context,
    double proportion, uint8_t *__restrict__ voiced, int64_t *__restrict__ count) {
  const int lane = threadIdx.x & (VD_WAVE - 1);
  const int64_t b = (int64_t)blockIdx.x * VD_WAVES + (threadIdx.x >> 6);
  if (b >= B) return;
  const int64_t Tn = nrows[b];
  if (Tn <= 0) {
    if (lane == 0) count[b] = 0;
    return;
  }
  const int64_t r0 = row_off[b];
  const T *e = energy + r0 * stride;
  const int64_t last = Tn - 1;
  double thr = energy_threshold;
  if (energy_mean_scale != 0.0) {
    // (vad_partial_sum with VD_AHEAD loads in flight: a row index past the end repeats the last row and is not added)
    double p = 0.0;
    for (int64_t t = lane; t < Tn; t += (int64_t)VD_AHEAD * VAD_PARTIALS) {
      double v[VD_AHEAD];
#pragma unroll
      for (int u = 0; u < VD_AHEAD; ++u) {
        const int64_t tt = t + (int64_t)u * VAD_PARTIALS;
        v[u] = (double)e[(tt < Tn ? tt : last) * stride];
      }
#pragma unroll
      for (int u = 0; u < VD_AHEAD; ++u)
        if (t + (int64_t)u * VAD_PARTIALS < Tn) p = p + v[u];
    }
    const double s = vad_combine(Tn, [&](int j) { return lane_value(p, j); });
    thr = vad_threshold(energy_threshold, energy_mean_scale, s, Tn);
  }
  const uint64_t below = ((uint64_t)1 << lane) - 1;  // the lanes in front of this one
  const uint64_t upto = below | ((uint64_t)1 << lane);
  // frames above the threshold among the first min(context, Tn): they lie in front of the first chunk's leading ends
  int64_t lead = 0, lag = 0, total = 0;
  const int64_t pre = context < Tn ? context : Tn;
  for (int64_t u0 = 0; u0 < pre; u0 += VD_WAVE) {
    const int64_t u = u0 + lane;
    const double v = (double)e[(u < pre ? u : pre - 1) * stride];
    lead += __popcll(__ballot(u < pre && vad_above(v, thr)));
  }
  for (int64_t t0 = 0; t0 < Tn; t0 += (int64_t)VD_AHEAD * VD_WAVE) {
    double hv[VD_AHEAD], lv[VD_AHEAD];
#pragma unroll
    for (int u = 0; u < VD_AHEAD; ++u) {
      const int64_t t = t0 + u * VD_WAVE + lane;
      const int64_t h = t + context, l = t - context;
      hv[u] = (double)e[(h < Tn ? h : last) * stride];
      lv[u] = context == 0 ? hv[u] : (double)e[(l < 0 ? 0 : l < Tn ? l : last) * stride];
    }
#pragma unroll
    for (int u = 0; u < VD_AHEAD; ++u) {
      const int64_t t = t0 + u * VD_WAVE + lane;
      if (t0 + u * VD_WAVE >= Tn) break;  // (the same in every lane)
      const int64_t h = t + context, l = t - context;
      const uint64_t hm = __ballot(h < Tn && vad_above(hv[u], thr));
      const uint64_t lm = __ballot(l >= 0 && l < Tn && vad_above(lv[u], thr));
      const int64_t upto_hi = lead + __popcll(hm & upto);     // above in [0, hi]
      const int64_t before_lo = lag + __popcll(lm & below);   // above in [0, lo)
      lead += __popcll(hm);
      lag += __popcll(lm);
      bool is_voiced = false;
      if (t < Tn) {
        int64_t lo, hi;
        vad_window(t, Tn, context, lo, hi);
        is_voiced = vad_vote(upto_hi - before_lo, hi - lo + 1, proportion);
        voiced[r0 + t] = is_voiced ? 1 : 0;
      }
      total += __popcll(__ballot(is_voiced));
    }
  }
  if (lane == 0) count[b] = total;
}

template <typename T>
static int32_t launch_vad_energy(const T *d_energy, int64_t stride, const int64_t *d_row_off, const int64_t *d_nrows,
                                 int32_t B, int64_t max_rows, double energy_threshold, double energy_mean_scale,
                                 int32_t frames_context, double proportion_threshold, uint8_t *d_voiced,
                                 int64_t *d_count, void *stream) {
  if (B < 0 || max_rows < 0) return stages_invalid("vad_energy_rows: bad size");
  if (!(energy_mean_scale >= 0.0) || frames_context < 0)
    return stages_invalid("vad_energy_rows: energy_mean_scale and frames_context must not be negative");
  if (!(proportion_threshold > 0.0 && proportion_threshold < 1.0))
    return stages_invalid("vad_energy_rows: proportion_threshold must lie strictly between 0 and 1");
  if (B == 0 || max_rows == 0) return PDS_STAGES_OK;
  if (stride < 1) return stages_invalid("vad_energy_rows: the row stride must be positive");
  if (!d_energy || !d_row_off || !d_nrows || !d_voiced || !d_count) return stages_invalid("vad_energy_rows: null pointer");
  const int64_t blocks = ((int64_t)B + VD_WAVES - 1) / VD_WAVES;  // (B < 2^31: always a grid)
  hipLaunchKernelGGL(vad_energy_kernel<T>, dim3((unsigned)blocks), dim3(VD_THREADS), 0, (hipStream_t)stream, d_energy,
                     stride, d_row_off, d_nrows, B, energy_threshold, energy_mean_scale, (int64_t)frames_context,
                     proportion_threshold, d_voiced, d_count);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return stages_hip_fail(err, "vad_energy_rows launch");
  return PDS_STAGES_OK;
}

// ---- the selection: one block per (utterance, tile of 256 rows) -----------------------------------------------------
//
// The block counts the kept rows in front of its tile (all its lanes, 256 flags at a time: the flags of an utterance
// of T rows are read T / 512 times over, a byte each), ranks the tile's own kept rows by a ballot per wave and the
// waves' counts, leaves their row numbers in rank order in LDS, and then all its lanes copy the kept rows word by
// word: adjacent lanes adjacent words of a row, and on from the end of one kept row to the start of the next, so that
// short rows fill a wave too.

__global__ __launch_bounds__(SEL_THREADS) void select_rows_kernel(
    const uint32_t *__restrict__ in, int64_t in_stride, int32_t words, const int64_t *__restrict__ row_off,
    const int64_t *__restrict__ nrows, int64_t tiles, const uint8_t *__restrict__ keep,
    const int64_t *__restrict__ out_row_off, uint32_t *__restrict__ out, int64_t out_stride) {
  __shared__ int64_t s_front[SEL_WAVES];
  __shared__ int32_t s_kept[SEL_WAVES];
  __shared__ int32_t s_rows[SEL_THREADS];
  const int64_t b = (int64_t)blockIdx.x / tiles, tile = (int64_t)blockIdx.x - b * tiles;
  const int64_t Tn = nrows[b];
  const int64_t t0 = tile * SEL_THREADS;
  if (t0 >= Tn) return;  // (a shorter utterance of the batch, or an empty one: the same in the whole block)
  const int64_t r0 = row_off[b];
  const uint8_t *k = keep + r0;
  const int lane = threadIdx.x & (VD_WAVE - 1), w = threadIdx.x >> 6;
  int64_t front = 0;
  for (int64_t t = threadIdx.x; t < t0; t += SEL_THREADS) front += k[t] != 0;
  const int64_t t = t0 + threadIdx.x;
  const bool mine = t < Tn && k[t] != 0;
  const uint64_t m = __ballot(mine);
#pragma unroll
  for (int off = VD_WAVE / 2; off; off >>= 1) front += __shfl_xor(front, off);
  if (lane == 0) {
    s_front[w] = front;
    s_kept[w] = __popcll(m);
  }
  __syncthreads();
  int64_t base = 0;
  int32_t kept = 0, rank = 0;
#pragma unroll
  for (int j = 0; j < SEL_WAVES; ++j) {
    base += s_front[j];
    if (j < w) rank += s_kept[j];
    kept += s_kept[j];
  }
  if (mine) s_rows[rank + __popcll(m & (((uint64_t)1 << lane) - 1))] = threadIdx.x;
  __syncthreads();
  if (kept == 0) return;
  const uint32_t *src = in + (r0 + t0) * in_stride;
  uint32_t *dst = out + (out_row_off[b] + base) * out_stride;
  for (int64_t c0 = 0; c0 < words; c0 += SEL_COLS) {
    const uint32_t cols = (uint32_t)(words - c0 < SEL_COLS ? words - c0 : SEL_COLS);
    const uint32_t n = (uint32_t)kept * cols;  // (at most 2^8 * 2^20)
#pragma unroll 4
    for (uint32_t i = threadIdx.x; i < n; i += SEL_THREADS) {
      const uint32_t q = i / cols, c = i - q * cols;
      dst[q * out_stride + c0 + c] = src[s_rows[q] * in_stride + c0 + c];
    }
  }
}

static int32_t launch_select_rows(const void *d_in, int64_t in_stride, int32_t words, const int64_t *d_row_off,
                                  const int64_t *d_nrows, int32_t B, int64_t max_rows, const uint8_t *d_keep,
                                  const int64_t *d_out_row_off, void *d_out, int64_t out_stride, void *stream) {
  if (B < 0 || max_rows < 0 || words <= 0) return stages_invalid("select_rows: bad size");
  if (B == 0 || max_rows == 0) return PDS_STAGES_OK;
  if (in_stride < words || out_stride < words) return stages_invalid("select_rows: a row stride is below the row's words");
  const int64_t tiles = max_rows / SEL_THREADS + (max_rows % SEL_THREADS != 0);
  if (tiles > (int64_t)0x7fffffff / B) return stages_invalid("select_rows: too many blocks in one call (split the batch)");
  if (!d_in || !d_out || !d_row_off || !d_nrows || !d_keep || !d_out_row_off)
    return stages_invalid("select_rows: null pointer");
  hipLaunchKernelGGL(select_rows_kernel, dim3((unsigned)((int64_t)B * tiles)), dim3(SEL_THREADS), 0,
                     (hipStream_t)stream, (const uint32_t *)d_in, in_stride, words, d_row_off, d_nrows, tiles, d_keep,
                     d_out_row_off, (uint32_t *)d_out, out_stride);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return stages_hip_fail(err, "select_rows launch");
  return PDS_STAGES_OK;
}

}  // namespace pds

extern "C" {

int32_t pds_vad_energy_rows_f32(const float *d_energy, int64_t stride, const int64_t *d_row_off,
                                const int64_t *d_nrows, int32_t B, int64_t max_rows, double energy_threshold,
                                double energy_mean_scale, int32_t frames_context, double proportion_threshold,
                                uint8_t *d_voiced, int64_t *d_count, void *stream) {
  return pds::launch_vad_energy<float>(d_energy, stride, d_row_off, d_nrows, B, max_rows, energy_threshold,
                                       energy_mean_scale, frames_context, proportion_threshold, d_voiced, d_count,
                                       stream);
}
int32_t pds_vad_energy_rows_f64(const double *d_energy, int64_t stride, const int64_t *d_row_off,
                                const int64_t *d_nrows, int32_t B, int64_t max_rows, double energy_threshold,
                                double energy_mean_scale, int32_t frames_context, double proportion_threshold,
                                uint8_t *d_voiced, int64_t *d_count, void *stream) {
  return pds::launch_vad_energy<double>(d_energy, stride, d_row_off, d_nrows, B, max_rows, energy_threshold,
                                        energy_mean_scale, frames_context, proportion_threshold, d_voiced, d_count,
                                        stream);
}

int32_t pds_select_rows_w32(const void *d_in, int64_t in_stride, int32_t words, const int64_t *d_row_off,
                            const int64_t *d_nrows, int32_t B, int64_t max_rows, const uint8_t *d_keep,
                            const int64_t *d_out_row_off, void *d_out, int64_t out_stride, void *stream) {
  return pds::launch_select_rows(d_in, in_stride, words, d_row_off, d_nrows, B, max_rows, d_keep, d_out_row_off, d_out,
                                 out_stride, stream);
}

}  // extern "C"
