// The rule of the energy VAD (include/pds_amd_stages.h, post.EnergyVAD): host and device, no dependencies.
// Shared by the kernels of vad.hip and by tests/csrc/test_vad_rule.cpp, which sweeps it on the CPU.
// Every float64 operation here is rounded by itself: a translation unit that includes this is built without
// contraction (the threshold is a product, a quotient and a sum, in that order).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PDS_VR_HD __host__ __device__ __forceinline__
#else
#define PDS_VR_HD inline
#endif

namespace pds {

constexpr int VAD_PARTIALS = 64;  // interleaved partial sums of an utterance's energies: one per lane of a wave

// Partial sum j (0 <= j < 64) of the T energies load(0) .. load(T - 1), already widened to float64: the energies
// t = j, j + 64, j + 128, .. in ascending order, starting from +0.0.  No energy (j >= T): +0.0.
template <typename Load>
PDS_VR_HD double vad_partial_sum(int64_t T, int j, Load load) {
  double p = 0.0;
  for (int64_t t = j; t < T; t += VAD_PARTIALS) p = p + load(t);
  return p;
}

// How many of the 64 partial sums of T energies have to be added: partial j >= T is +0.0, and s + (+0.0) has the
// bits of s for every s but -0.0, which a sum that started from +0.0 never is (x + y is -0.0 only if both are).
PDS_VR_HD int vad_partials_used(int64_t T) { return T < VAD_PARTIALS ? (int)(T < 0 ? 0 : T) : VAD_PARTIALS; }

// The sum of an utterance's energies: s = +0.0, then s += partial(j) for j = 0 .. 63 in order (the partials past
// vad_partials_used(T) are left out: see there)
template <typename Partial>
PDS_VR_HD double vad_combine(int64_t T, Partial partial) {
  double s = 0.0;
  const int n = vad_partials_used(T);
  for (int j = 0; j < n; ++j) s = s + partial(j);
  return s;
}

// energy_threshold + (energy_mean_scale * s) / T, each operation rounded once (T >= 1, energy_mean_scale != 0)
PDS_VR_HD double vad_threshold(double energy_threshold, double energy_mean_scale, double s, int64_t T) {
  const double scaled = energy_mean_scale * s;
  const double mean = scaled / (double)T;
  return energy_threshold + mean;
}

// A NaN energy is never above the threshold, nor is anything above a NaN threshold
PDS_VR_HD bool vad_above(double e, double thr) { return e > thr; }

// Frames [lo, hi] that vote on frame t of an utterance of T frames (0 <= t < T, frames_context >= 0)
PDS_VR_HD void vad_window(int64_t t, int64_t T, int64_t frames_context, int64_t &lo, int64_t &hi) {
  lo = t > frames_context ? t - frames_context : 0;
  hi = frames_context < T - 1 - t ? t + frames_context : T - 1;
}

// num of the den frames of a window lie above the threshold: is the frame voiced
PDS_VR_HD bool vad_vote(int64_t num, int64_t den, double proportion_threshold) {
  return (double)num >= (double)den * proportion_threshold;
}

}  // namespace pds
