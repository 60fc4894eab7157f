// The rule of reverberation (include/pds_amd_stages6.h, pre.Reverb): host and device, no dependencies.  Shared by the
// kernels of reverb.hip and by tests/csrc/test_reverb_rule.cpp, which sweeps it on the CPU.  Everything here is integer
// arithmetic but the one comparison of the plan.  The library shares no header with the other six, so Philox4x32-10 is
// restated here (the round function is the one of dither_noise.h), host-callable.
//
// The definition's text is in include/pds_amd_stages6.h.  The form the kernels take, which this header counts for:
//
// - y_full of an utterance is cut into blocks of 512 samples on multiples of 512 of tau; block k covers
//   [512 k, 512 k + 512).  Blocks 2 m and 2 m + 1 form pair m: one inverse transform yields both.
// - Spectrum k of an utterance, k = -1 .. reverb_last_spectrum(n), is the 1024-point transform of
//   z[s] = x[512 (k - 1) + s] + i x[512 k + s], 0 <= s < 1024 (x zero outside [0, n)): the stretch of block k in the real
//   part, the stretch of block k + 1 in the imaginary part.  Spectra below -1 and above the last are zero: not stored,
//   not added.
// - Pair m (k = 2 m) is sum_p Z_{k - p} H_p over p = reverb_first_part .. reverb_last_part in ascending order, one
//   inverse transform, elements 512 .. 1023: the real part is block k, the imaginary part block k + 1.
// - A unit is what one half wave does: one spectrum, one pair, or 1024 samples of a copied utterance.  An utterance's
//   units are rounded up to an even count, so that the two halves of a wave serve one utterance.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PDS_RV_HD __host__ __device__ __forceinline__
#else
#define PDS_RV_HD inline
#endif

namespace pds {

constexpr int64_t REVERB_BLOCK = 512;             // B: taps of a partition, samples of a block of y_full
constexpr int64_t REVERB_FFT = 1024;              // N: points of a transform
constexpr int64_t REVERB_MAX_TAPS = 1 << 20;      // taps a room impulse response may have
constexpr int REVERB_HALVES = 8;                  // half waves (units) of a block of the transform kernels
constexpr int REVERB_THREADS = REVERB_HALVES * 32;
constexpr int REVERB_ROW_STRIDE = 33;             // complex values between rows of a transposition area (no conflicts)
constexpr int REVERB_SCALE_THREADS = 256;         // lanes of a block of the scale kernel
constexpr int REVERB_SCALE_VEC = 4;               // consecutive samples of a lane: one wide access
constexpr int REVERB_SCALE_ITERS = 4;             // groups of a lane
constexpr int64_t REVERB_SCALE_STRIDE = (int64_t)REVERB_SCALE_THREADS * REVERB_SCALE_VEC;
constexpr int64_t REVERB_SCALE_TILE = REVERB_SCALE_STRIDE * REVERB_SCALE_ITERS;
constexpr int REVERB_MAX_UTTS = 65535;            // utterances of one launch of the scale kernel (grid.y)
constexpr int64_t REVERB_MAX_BLOCKS = 0x7fffffff;  // blocks one launch may have: 2^31 - 1

// The counter of the plan's one Philox block.  dither_noise.h forms (q_lo, q_hi, 0, 0), specaug_rule.h (i, 0, d, 0)
// and mix_rule.h (0, 0, 0, 0x4D495831): this fourth word differs from all of them.
constexpr uint32_t REVERB_COUNTER_0 = 0u, REVERB_COUNTER_1 = 0u, REVERB_COUNTER_2 = 0u,
                   REVERB_COUNTER_3 = 0x52495231u;  // "RIR1"

// ---- the generator --------------------------------------------------------------------------------------------------

// Philox4x32-10 (Salmon et al., SC'11) on counter c under key (k0, k1), in place
PDS_RV_HD void reverb_philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
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
PDS_RV_HD void reverb_draw(uint64_t key, uint32_t x[4]) {
  x[0] = REVERB_COUNTER_0; x[1] = REVERB_COUNTER_1; x[2] = REVERB_COUNTER_2; x[3] = REVERB_COUNTER_3;
  reverb_philox(x, (uint32_t)key, (uint32_t)(key >> 32));
}

// ---- the plan's draws -----------------------------------------------------------------------------------------------

// j = (x0 * K) >> 32 for 1 <= K < 2^31, an integer in [0, K)
PDS_RV_HD int64_t reverb_pick(uint32_t x0, int64_t K) { return (int64_t)(((uint64_t)x0 * (uint64_t)K) >> 32); }

PDS_RV_HD bool reverb_applied(uint32_t x3, double prob) { return (double)x3 * (1.0 / 4294967296.0) < prob; }

// ---- partitions, blocks, spectra ------------------------------------------------------------------------------------

// P: partitions of a response of L taps (0 for L <= 0)
PDS_RV_HD int64_t reverb_partitions(int64_t L) { return L <= 0 ? 0 : (L + REVERB_BLOCK - 1) / REVERB_BLOCK; }

// first and last block of y_full an utterance of n >= 1 samples with peak d >= 0 needs: tau in [d, d + n)
PDS_RV_HD int64_t reverb_first_block(int64_t d) { return d / REVERB_BLOCK; }
PDS_RV_HD int64_t reverb_last_block(int64_t n, int64_t d) { return (d + n - 1) / REVERB_BLOCK; }

// first pair, and the pairs of the utterance (0 for n <= 0)
PDS_RV_HD int64_t reverb_first_pair(int64_t d) { return d / REVERB_FFT; }
PDS_RV_HD int64_t reverb_pairs(int64_t n, int64_t d) {
  return n <= 0 ? 0 : (d + n - 1) / REVERB_FFT - d / REVERB_FFT + 1;
}

// output samples [begin, end) of the utterance that block k writes once shifted by -d and clipped to [0, n)
PDS_RV_HD void reverb_block_out(int64_t k, int64_t n, int64_t d, int64_t &begin, int64_t &end) {
  const int64_t lo = k * REVERB_BLOCK - d, hi = lo + REVERB_BLOCK;
  begin = lo < 0 ? 0 : lo > n ? n : lo;
  end = hi < 0 ? 0 : hi > n ? n : hi;  // (hi > lo, so end >= begin; a block outside the utterance gives begin == end)
}

// the last spectrum that is not zero: its real stretch begins at 512 (k - 1) <= n - 1 (n >= 1); the first is -1
PDS_RV_HD int64_t reverb_last_spectrum(int64_t n) { return (n - 1) / REVERB_BLOCK + 1; }

// spectra stored for an utterance of n samples: k = -1 .. last (0 for n <= 0); spectrum k lies in slot k + 1
PDS_RV_HD int64_t reverb_spectra(int64_t n) { return n <= 0 ? 0 : reverb_last_spectrum(n) + 2; }

// sample index of element s of spectrum k: real part and imaginary part; zero fill where outside [0, n)
PDS_RV_HD int64_t reverb_stretch_re(int64_t k, int64_t s) { return (k - 1) * REVERB_BLOCK + s; }
PDS_RV_HD int64_t reverb_stretch_im(int64_t k, int64_t s) { return k * REVERB_BLOCK + s; }
PDS_RV_HD bool reverb_inside(int64_t i, int64_t n) { return i >= 0 && i < n; }

// partitions p of the sum of the pair at block k (even): -1 <= k - p <= last spectrum, 0 <= p < P; empty if first > last
PDS_RV_HD int64_t reverb_first_part(int64_t k, int64_t n) {
  const int64_t lo = k - reverb_last_spectrum(n);
  return lo < 0 ? 0 : lo;
}
PDS_RV_HD int64_t reverb_last_part(int64_t k, int64_t P) { return k + 1 < P - 1 ? k + 1 : P - 1; }

// ---- units, grids, workspace ------------------------------------------------------------------------------------------

PDS_RV_HD int64_t reverb_even(int64_t units) { return (units + 1) & ~(int64_t)1; }

// An utterance is `transformed` where it is applied and its response has more than one non-zero tap; else it is copied
// (not applied) or delayed and scaled (one tap), 1024 samples a unit, and needs no spectra.

// units of the spectra kernel for an utterance: its spectra where transformed, else none
PDS_RV_HD int64_t reverb_spectra_units(int64_t n, bool transformed) {
  return transformed ? reverb_even(reverb_spectra(n)) : 0;
}

// units of the convolve kernel: pairs where transformed, else stretches of 1024 samples
PDS_RV_HD int64_t reverb_convolve_units(int64_t n, int64_t d, bool transformed) {
  if (n <= 0) return 0;
  return reverb_even(transformed ? reverb_pairs(n, d) : (n + REVERB_FFT - 1) / REVERB_FFT);
}

// blocks of a transform kernel over `units` units, or -1 above 2^31 - 1
PDS_RV_HD int64_t reverb_blocks(int64_t units) {
  if (units < 0) return -1;
  const int64_t blocks = (units + REVERB_HALVES - 1) / REVERB_HALVES;
  return blocks > REVERB_MAX_BLOCKS ? -1 : blocks;
}

// bytes of the workspace of `units` spectra slots (complex64, 1024 each), or -1 where the count is refused
PDS_RV_HD int64_t reverb_workspace_bytes(int64_t units) {
  if (reverb_blocks(units) < 0) return -1;
  return units * REVERB_FFT * 8;
}

// blocks along x of the scale kernel for utterances of at most max_len samples (groups stand on multiples of 4 of the
// buffer, so an utterance may begin up to 3 samples into its first group), and of one launch over B utterances
PDS_RV_HD int64_t reverb_scale_blocks_x(int64_t max_len) {
  if (max_len <= 0) return 0;
  return (max_len + (REVERB_SCALE_VEC - 1) + REVERB_SCALE_TILE - 1) / REVERB_SCALE_TILE;
}
PDS_RV_HD int64_t reverb_scale_blocks(int64_t max_len, int64_t B) {
  if (B < 0 || B > REVERB_MAX_UTTS || max_len < 0) return -1;
  const int64_t bx = reverb_scale_blocks_x(max_len);
  if (bx > REVERB_MAX_BLOCKS) return -1;
  const int64_t blocks = bx * B;
  return blocks > REVERB_MAX_BLOCKS ? -1 : blocks;
}

// the utterance of unit u: the last b of B with base[b] <= u (utterances without units share the base of the next)
PDS_RV_HD int reverb_find(const int64_t *base, int B, int64_t u) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (base[mid] <= u) lo = mid; else hi = mid - 1;
  }
  return lo;
}

}  // namespace pds
