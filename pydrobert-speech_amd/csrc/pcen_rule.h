// The rule of per-channel energy normalisation (include/pds_amd_stages2.h, post.PCEN): host and device, no
// dependencies but <math.h>.  Shared by the kernels of pcen.hip and by tests/csrc/test_pcen_rule.cpp, which sweeps it
// on the CPU.  Every float64 operation here is rounded by itself: a translation unit that includes this is built
// without contraction (the smoother is two products and a sum, in that order).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PDS_PR_HD __host__ __device__ __forceinline__
#else
#define PDS_PR_HD inline
#endif

namespace pds {

constexpr int PCEN_THREADS = 256;                    // lanes of a block of every PCEN kernel
constexpr int64_t PCEN_MAX_BLOCKS = 0x7fffffff;      // blocks one launch may have: 2^31 - 1
constexpr int PCEN_AHEAD = 4;  // row loads in flight per lane of the smoother (the chain is sequential, the loads are not)

// One step of the smoother: M[t] = (oms * M[t-1]) + (smooth * E[t]), two products and one sum, each rounded once.
// `oms` is 1 - smooth as the host rounded it; it is never recomputed here.
PDS_PR_HD double pcen_smooth_step(double oms, double smooth, double m_prev, double e) {
  const double kept = oms * m_prev;
  const double fresh = smooth * e;
  return kept + fresh;
}

// The smoother's value at a row: the first row of an utterance starts it (M = E, widened exactly), every other row
// takes a step from the row before
PDS_PR_HD double pcen_smooth_row(bool first, double oms, double smooth, double m_prev, double e) {
  return first ? e : pcen_smooth_step(oms, smooth, m_prev, e);
}

// One lane's walk over its utterance of Tn rows: M of every row, in order.  load(t) gives E[t] widened (0 <= t < Tn),
// store(t, m) takes M[t].  PCEN_AHEAD rows at a time: their loads first, without a condition (a row past the end
// repeats the last one, so every index given to load lies in [0, Tn)) and so in flight together, then the chain and
// the stores in row order.  The loads are unrolled, not the arithmetic chain: each step waits for the one before.
template <typename Load, typename Store>
PDS_PR_HD void pcen_smooth_walk(int64_t Tn, double oms, double smooth, Load load, Store store) {
  double prev = 0.0;
  for (int64_t t = 0; t < Tn; t += PCEN_AHEAD) {
    double v[PCEN_AHEAD];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int u = 0; u < PCEN_AHEAD; ++u) {
      const int64_t tt = t + u < Tn ? t + u : Tn - 1;
      v[u] = load(tt);
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int u = 0; u < PCEN_AHEAD; ++u) {
      if (t + u >= Tn) continue;
      prev = pcen_smooth_row(t + u == 0, oms, smooth, prev, v[u]);
      store(t + u, prev);
    }
  }
}

// Lanes of a launch with one lane per (item, column): `items` utterances or streams of C columns each, in 64 bits.
// -1 if a count is negative or the product does not fit (items * C >= 2^63)
PDS_PR_HD int64_t pcen_lane_count(int64_t items, int64_t C) {
  if (items < 0 || C < 0) return -1;
  if (items == 0 || C == 0) return 0;
  if (items > INT64_MAX / C) return -1;
  return items * C;
}

// Blocks of PCEN_THREADS lanes that cover `lanes` lanes; -1 above 2^31 - 1 blocks (the caller refuses the launch) and
// for a negative count
PDS_PR_HD int64_t pcen_block_count(int64_t lanes) {
  if (lanes < 0) return -1;
  const int64_t blocks = lanes / PCEN_THREADS + (lanes % PCEN_THREADS != 0);
  return blocks > PCEN_MAX_BLOCKS ? -1 : blocks;
}

// Lane g of block `block`, thread `thread`
PDS_PR_HD int64_t pcen_lane(int64_t block, int thread) { return block * PCEN_THREADS + thread; }

// Lane g -> (item, column): adjacent lanes sit on adjacent columns of one item, so a wave reads contiguous runs of a row
PDS_PR_HD void pcen_lane_map(int64_t g, int64_t C, int64_t &item, int64_t &column) {
  item = g / C;
  column = g - item * C;
}

// y = pow(E / pow(eps + M, gain) + bias, power) - bp with bp = bias ** power from the host: every operation float64, no
// special case for an exponent
PDS_PR_HD double pcen_compress(double e, double m, double gain, double bias, double power, double eps, double bp) {
  const double floor_m = eps + m;
  const double agc = pow(floor_m, gain);
  const double ratio = e / agc;
  const double biased = ratio + bias;
  const double root = pow(biased, power);
  return root - bp;
}

}  // namespace pds
