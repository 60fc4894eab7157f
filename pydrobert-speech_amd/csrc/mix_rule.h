// The rule of noise mixing (include/pds_amd_stages5.h, pre.AddNoise): host and device, no dependencies but <math.h>.
// Shared by the kernels of mix.hip and by tests/csrc/test_mix_rule.cpp, which sweeps it on the CPU.  Every float64
// operation here is rounded by itself: a translation unit that includes this is built without contraction.  The
// library shares no header with the other five, so Philox4x32-10 is restated here (the round function is the one of
// dither_noise.h), host-callable.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PDS_MX_HD __host__ __device__ __forceinline__
#else
#define PDS_MX_HD inline
#endif

namespace pds {

constexpr int MIX_WAVE = 64;                     // lanes of a wave: the lanes of a chunk's sum
constexpr int64_t MIX_CHUNK = 16384;             // samples of a chunk of the segment energy
constexpr int MIX_ENERGY_WAVES = 4;              // waves (chunks) of a block of the energy kernel
constexpr int MIX_AHEAD = 8;                     // loads in flight per lane of the energy kernel
constexpr int MIX_THREADS = 256;                 // lanes of a block of the gain and apply kernels
constexpr int MIX_VEC = 4;                       // consecutive samples of a lane: one wide access
constexpr int MIX_ITERS = 4;                     // groups of a lane, MIX_THREADS * MIX_VEC samples apart
constexpr int64_t MIX_STRIDE = (int64_t)MIX_THREADS * MIX_VEC;  // samples between a lane's groups
constexpr int64_t MIX_TILE = MIX_STRIDE * MIX_ITERS;            // samples of a block of the apply kernel
constexpr int MIX_MAX_UTTS = 65535;              // utterances of one launch of the apply kernel (grid.y)
constexpr int64_t MIX_MAX_BLOCKS = 0x7fffffff;   // blocks one launch may have: 2^31 - 1

// The counter of the plan's one Philox block.  dither_noise.h forms (q_lo, q_hi, 0, 0) and specaug_rule.h
// (i, 0, d, 0): both leave the fourth word zero, so a counter whose fourth word is not zero differs from all of them.
constexpr uint32_t MIX_COUNTER_0 = 0u, MIX_COUNTER_1 = 0u, MIX_COUNTER_2 = 0u, MIX_COUNTER_3 = 0x4D495831u;  // "MIX1"

// ---- the generator --------------------------------------------------------------------------------------------------

// Philox4x32-10 (Salmon et al., SC'11) on counter c under key (k0, k1), in place
PDS_MX_HD void mix_philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// x0..x3 of the utterance with `key` (split as dither_noise.h splits it: low word, high word)
PDS_MX_HD void mix_draw(uint64_t key, uint32_t x[4]) {
  x[0] = MIX_COUNTER_0; x[1] = MIX_COUNTER_1; x[2] = MIX_COUNTER_2; x[3] = MIX_COUNTER_3;
  mix_philox(x, (uint32_t)key, (uint32_t)(key >> 32));
}

// ---- the plan's draws -----------------------------------------------------------------------------------------------

// (x * n) >> 32 for 0 <= n < 2^63, an integer in [0, n): the 96-bit product is taken in two halves
PDS_MX_HD int64_t mix_pick(uint32_t x, int64_t n) {
  const uint64_t un = (uint64_t)n;
  const uint64_t lo = (uint64_t)x * (un & 0xffffffffu);  // x * low word, below 2^64
  const uint64_t hi = (uint64_t)x * (un >> 32);          // x * high word, weighs 2^32
  return (int64_t)(hi + (lo >> 32));                     // ((hi << 32) + lo) >> 32, exact: the low 32 bits of lo fall off
}

// snr = lo + (hi - lo) * (x2 * 2^-32), each operation rounded by itself; exactly lo where lo == hi
PDS_MX_HD double mix_snr(double lo, double hi, uint32_t x2) {
  const double u = (double)x2 * (1.0 / 4294967296.0);  // exact
  const double d = hi - lo;
  const double m = d * u;
  return lo + m;
}

PDS_MX_HD bool mix_applied(uint32_t x3, double prob) { return (double)x3 * (1.0 / 4294967296.0) < prob; }

// ---- the segment energy ---------------------------------------------------------------------------------------------

// chunks of a segment of n samples
PDS_MX_HD int64_t mix_chunks(int64_t n) { return n <= 0 ? 0 : (n + MIX_CHUNK - 1) / MIX_CHUNK; }

// samples [begin, end) of chunk c of a segment of n samples
PDS_MX_HD void mix_chunk_span(int64_t c, int64_t n, int64_t &begin, int64_t &end) {
  begin = c * MIX_CHUNK;
  end = begin + MIX_CHUNK < n ? begin + MIX_CHUNK : n;
}

// lane's partial sum of [begin, end): i = begin + lane, begin + lane + 64, ... in that order from +0.0; `load(i)` is
// sample i widened to float64; the product is rounded by itself
template <typename Load>
PDS_MX_HD double mix_lane_sum(Load load, int64_t begin, int64_t end, int lane) {
  double p = 0.0;
  for (int64_t i = begin + lane; i < end; i += MIX_WAVE) {
    const double v = load(i);
    const double sq = v * v;
    p = p + sq;
  }
  return p;
}

// the same sum with MIX_AHEAD loads issued before the adds that depend on them (the kernel's form): the adds keep their
// order, so the value is mix_lane_sum's bit for bit; `Raw` is what `fetch(i)` gives and `widen` makes float64 of it
template <typename Raw, typename Fetch, typename Widen>
PDS_MX_HD double mix_lane_sum_ahead(Fetch fetch, Widen widen, int64_t begin, int64_t end, int lane) {
  double p = 0.0;
  int64_t i = begin + lane;
  for (; i + (int64_t)(MIX_AHEAD - 1) * MIX_WAVE < end; i += (int64_t)MIX_AHEAD * MIX_WAVE) {
    Raw raw[MIX_AHEAD];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < MIX_AHEAD; ++k) raw[k] = fetch(i + (int64_t)k * MIX_WAVE);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < MIX_AHEAD; ++k) {
      const double v = widen(raw[k]);
      const double sq = v * v;
      p = p + sq;
    }
  }
  for (; i < end; i += MIX_WAVE) {
    const double v = widen(fetch(i));
    const double sq = v * v;
    p = p + sq;
  }
  return p;
}

// the fixed tree over the 64 partial sums, in place: for s = 32, 16, .., 1: p[l] += p[l + s] for l < s; the sum is p[0]
PDS_MX_HD double mix_tree(double p[MIX_WAVE]) {
  for (int s = MIX_WAVE / 2; s >= 1; s >>= 1)
    for (int l = 0; l < s; ++l) p[l] = p[l] + p[l + s];
  return p[0];
}

// the sum of chunk c of a segment of n samples (what one wave of the energy kernel writes)
template <typename Load>
inline double mix_chunk_sum(Load load, int64_t c, int64_t n) {
  int64_t begin, end;
  mix_chunk_span(c, n, begin, end);
  double p[MIX_WAVE];
  for (int l = 0; l < MIX_WAVE; ++l) p[l] = mix_lane_sum(load, begin, end, l);
  return mix_tree(p);
}

// E of `count` chunk sums: from +0.0, in ascending order (what one lane of the gain kernel does)
PDS_MX_HD double mix_fold(const double *partials, int64_t count) {
  double e = 0.0;
  for (int64_t c = 0; c < count; ++c) e = e + partials[c];
  return e;
}

// mean power of a segment of n samples with energy e
PDS_MX_HD double mix_power(double e, int64_t n) { return n > 0 ? e / (double)n : 0.0; }

// ---- the gain -------------------------------------------------------------------------------------------------------

// g = sqrt(Ps / (Pn * r)) where applied, Ps > 0 and Pn > 0 (comparisons false for NaN), else 0.0; `root` is the square
// root (the device's correctly rounded one in the kernel, sqrt() on the host)
template <typename Root>
PDS_MX_HD double mix_gain(bool applied, double ps, double pn, double r, Root root) {
  if (!(applied && ps > 0.0 && pn > 0.0)) return 0.0;
  const double den = pn * r;
  const double q = ps / den;
  return root(q);
}

// ---- the wrapped index ----------------------------------------------------------------------------------------------

// position of sample t >= 0 in a clip of L >= 1 samples read from start s, 0 <= s < L: the one modulo of a lane
PDS_MX_HD int64_t mix_wrap_first(int64_t s, int64_t t, int64_t L) { return (int64_t)(((uint64_t)s + (uint64_t)t) % (uint64_t)L); }

// the step a stride makes in a clip of L samples: stride mod L, found once per utterance
// (a stride is below 2^31: where L is above it the stride itself, else a 32-bit modulo)
PDS_MX_HD int64_t mix_wrap_stride(int64_t stride, int64_t L) {
  return L > stride ? stride : (int64_t)((uint32_t)stride % (uint32_t)L);
}

// position after one more stride: pos + step, less L where that reaches L (0 <= pos < L, 0 <= step < L)
PDS_MX_HD int64_t mix_wrap_step(int64_t pos, int64_t step, int64_t L) {
  const int64_t next = pos + step;
  return next >= L ? next - L : next;
}

// ---- block counts ---------------------------------------------------------------------------------------------------

// blocks of the energy kernel over `total_chunks` chunks, or -1 above 2^31 - 1
PDS_MX_HD int64_t mix_energy_blocks(int64_t total_chunks) {
  if (total_chunks < 0) return -1;
  const int64_t blocks = (total_chunks + MIX_ENERGY_WAVES - 1) / MIX_ENERGY_WAVES;
  return blocks > MIX_MAX_BLOCKS ? -1 : blocks;
}

// blocks along x of the apply kernel for utterances of at most max_len samples: a lane's groups stand on multiples of
// MIX_VEC of the buffer, so an utterance may begin up to MIX_VEC - 1 samples into its first group
PDS_MX_HD int64_t mix_apply_blocks_x(int64_t max_len) {
  if (max_len <= 0) return 0;
  return (max_len + (MIX_VEC - 1) + MIX_TILE - 1) / MIX_TILE;
}

// blocks of one launch of the apply kernel over B utterances, or -1 above 2^31 - 1 (or B above MIX_MAX_UTTS)
PDS_MX_HD int64_t mix_apply_blocks(int64_t max_len, int64_t B) {
  if (B < 0 || B > MIX_MAX_UTTS || max_len < 0) return -1;
  const int64_t bx = mix_apply_blocks_x(max_len);
  if (bx > MIX_MAX_BLOCKS) return -1;
  const int64_t blocks = bx * B;  // below 2^31 * 2^16
  return blocks > MIX_MAX_BLOCKS ? -1 : blocks;
}

// blocks of the gain kernel: one lane per utterance
PDS_MX_HD int64_t mix_gain_blocks(int64_t B) { return B < 0 ? -1 : (B + MIX_THREADS - 1) / MIX_THREADS; }

}  // namespace pds
