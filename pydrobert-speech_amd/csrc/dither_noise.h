// The noise of Dither (pre.py), shared by every kernel that adds it: pre.hip's dither_kernel and dither_packed_kernel
// and multistream.hip's multistream_assemble_dither_kernel.
//
// Counter-based: the noise of sample t of an utterance depends on (key, t) alone.  Samples 2q and 2q + 1 share pair q:
// one Philox4x32-10 block (counter = q, key = the utterance's 64-bit key) gives two uniforms of 53 bits, Box-Muller two
// Gaussians; the even sample takes the cosine branch, the odd one the sine branch.  The result is
//   (T)((double)x + (coeff * rad) * trig)
// with the two multiplies and the add rounded separately -- written with __dmul_rn / __dadd_rn so that it is the same
// value in every kernel and under every -ffp-contract setting (pre.hip and multistream.hip are built with
// -ffp-contract=off; dither_kernel compiled to exactly these three operations before the arithmetic moved here).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pds {

// Philox4x32-10 (Salmon et al., SC'11): counter = element block, key = seed
__device__ __forceinline__ void philox4x32(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
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

// the noise of pair q under `key`, scaled by coeff: `even` for sample 2q, `odd` for sample 2q + 1
__device__ __forceinline__ void dither_pair(int64_t q, uint64_t key, double coeff, double &even, double &odd) {
  uint32_t c[4] = {(uint32_t)q, (uint32_t)((uint64_t)q >> 32), 0u, 0u};
  philox4x32(c, (uint32_t)key, (uint32_t)(key >> 32));
  // two uniforms in (0, 1] and [0, 1) (every operation here is exact: integers below 2^53 and a power of two)
  const double u1 = ((double)(((uint64_t)c[0] << 21) ^ (c[1] >> 11)) + 1.0) * (1.0 / 9007199254740992.0);
  const double u2 = (double)(((uint64_t)c[2] << 21) ^ (c[3] >> 11)) * (1.0 / 9007199254740992.0);
  const double rad = sqrt(-2.0 * log(u1));
  double s, co;
  sincospi(2.0 * u2, &s, &co);
  const double scaled = __dmul_rn(coeff, rad);
  even = __dmul_rn(scaled, co);
  odd = __dmul_rn(scaled, s);
}

// sample x (already widened exactly to float64) with its noise, rounded to T once
template <typename T>
__device__ __forceinline__ T dither_add(double x, double noise) {
  return (T)__dadd_rn(x, noise);
}

// the noise of the single sample at position t (a lane that needs one sample of a pair, not both)
__device__ __forceinline__ double dither_noise_at(int64_t t, uint64_t key, double coeff) {
  double even, odd;
  dither_pair(t >> 1, key, coeff, even, odd);
  return (t & 1) ? odd : even;
}

}  // namespace pds
