// The rule of perceptual linear prediction cepstra (include/pds_amd_stages4.h, post.PLP): host and device, no
// dependencies but <math.h>.  Included by plp.hip, whose every kernel inlines plp_row, and by
// tests/csrc/test_plp_rule.cpp, which sweeps it on the CPU.  Every float64 operation here is rounded by itself: a
// translation unit that includes this is built without contraction.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PDS_PL_HD __host__ __device__ __forceinline__
#else
#define PDS_PL_HD inline
#endif

namespace pds {

constexpr int PLP_THREADS = 64;                 // lanes of a block = rows of a block: one wave, a row per lane
constexpr int64_t PLP_MAX_BLOCKS = 0x7fffffff;  // blocks one launch may have: 2^31 - 1
constexpr int PLP_MAX_WIDTH = 256;              // columns of an input row
constexpr int PLP_MAX_ORDER = 32;               // the LPC order p
constexpr double PLP_CLAMP = 1e-5;              // the least 1 - k^2 of a Durbin step

// Blocks of PLP_THREADS rows that cover `rows` rows; -1 above 2^31 - 1 blocks (the caller refuses the launch) and for
// a negative count
PDS_PL_HD int64_t plp_block_count(int64_t rows) {
  if (rows < 0) return -1;
  const int64_t blocks = rows / PLP_THREADS + (rows % PLP_THREADS != 0);
  return blocks > PLP_MAX_BLOCKS ? -1 : blocks;
}

// The row of lane `thread` of block `block`: adjacent lanes on adjacent rows
PDS_PL_HD int64_t plp_lane_row(int64_t block, int thread) { return block * PLP_THREADS + thread; }

// float64 words of working storage a row needs: r[0..p] (which q[0..p-1] takes over once Durbin is through) and
// a[0..p-1]
PDS_PL_HD int plp_work_words(int p) { return 2 * p + 1; }

// ... and the bytes of LDS of a block of PLP_THREADS rows
PDS_PL_HD int64_t plp_block_lds_bytes(int p) { return (int64_t)plp_work_words(p) * PLP_THREADS * 8; }

// 1 if (F, copy, p, K) is a shape the definition serves: 1 <= F, F + copy <= 256, 1 <= p <= min(F + 1, 32),
// 1 <= K <= p + 1
PDS_PL_HD int plp_shape_ok(int64_t F, int64_t copy, int64_t p, int64_t K) {
  if (copy != 0 && copy != 1) return 0;
  if (F < 1 || F + copy > PLP_MAX_WIDTH) return 0;
  if (p < 1 || p > PLP_MAX_ORDER || p > F + 1) return 0;
  return K >= 1 && K <= p + 1;
}

// Steps 2 and 3 of the definition for one widened energy: the floor (a NaN passes), the weight, the root
template <typename Pow>
PDS_PL_HD double plp_compress(double e, double w, double compress_factor, double floor, Pow pow_fn) {
  const double g = (e < floor) ? floor : e;
  const double weighted = g * w;
  return pow_fn(weighted, compress_factor);
}

// One column of the spectrum d[j] = v into the autocorrelations: r[i] = r[i] + B[i][j] * v for every i
PDS_PL_HD void plp_accumulate(double *work, int64_t stride, const double *B, int D, int p, int j, double v) {
  for (int i = 0; i <= p; ++i) {
    const double prod = B[(int64_t)i * D + j] * v;
    work[i * stride] = work[i * stride] + prod;
  }
}

// Steps 6 and 7 over r = work[0..p] and a = work[p+1..2p], elements `stride` words apart: Durbin's recursion, then the
// cepstrum, which is written over r (dead by then): q[i] is work[i] on return.  Returns the final E.
//
// The t of step 6.5 is not stored: t[j] and t[i - 1 - j] need a[j] and a[i - 1 - j] and nothing else, so the pair is
// read, both values are formed -- the very products and differences of the definition -- and written back.
PDS_PL_HD double plp_recursions(double *work, int64_t stride, int p) {
  double *r = work;
  double *a = work + (int64_t)(p + 1) * stride;
  double E = r[0];
  for (int i = 0; i < p; ++i) {
    double k = r[(i + 1) * stride];
    for (int j = 0; j < i; ++j) {
      const double prod = a[j * stride] * r[(i - j) * stride];
      k = k + prod;
    }
    k = k / E;
    const double kk = k * k;
    double c = 1.0 - kk;
    c = (c < PLP_CLAMP) ? PLP_CLAMP : c;  // (a NaN passes)
    E = E * c;
    for (int j = 0; 2 * j < i - 1; ++j) {
      const int m = i - 1 - j;
      const double lo = a[j * stride], hi = a[m * stride];
      const double from_hi = k * hi;
      const double from_lo = k * lo;
      a[j * stride] = lo - from_hi;
      a[m * stride] = hi - from_lo;
    }
    if (i & 1) {  // (i elements, i odd: the middle one pairs with itself)
      const int m = (i - 1) / 2;
      const double mid = a[m * stride];
      const double prod = k * mid;
      a[m * stride] = mid - prod;
    }
    a[i * stride] = -k;
  }
  double *q = work;
  for (int i = 0; i < p; ++i) {
    double s = 0.0;
    for (int j = 0; j < i; ++j) {
      const double scaled = (double)(i - j) * a[j * stride];
      const double prod = scaled * q[(i - j - 1) * stride];
      s = s + prod;
    }
    const double mean = s / (double)(i + 1);
    q[i * stride] = -a[i * stride] - mean;
  }
  return E;
}

// Steps 1 to 8 for one row.  load(c) gives column c of the row widened (0 <= c < copy + F); `work` is
// plp_work_words(p) float64 words `stride` apart, the row's own; w[F], B[p+1][D] and L[K] are the host's tables;
// pow_fn and log_fn are the two calls that are not plain IEEE arithmetic; store(k, v) takes output column k, still
// float64 (the caller rounds it once to the row's type); aux(j, v) takes d[j] for j < D and E as j = D, and is
// called only if `want_aux`.
//
// The row streams through: h[f] is computed, goes into all p + 1 sums as d[1 + f] (and as d[0] or d[D - 1] at the
// edges, in the order of j) and is dropped, so d is never stored.
template <typename Load, typename Pow, typename Log, typename Store, typename Aux>
PDS_PL_HD void plp_row(Load load, int F, int copy, const double *w, const double *B, const double *L, int p, int K,
                       double compress_factor, double floor, double *work, int64_t stride, Pow pow_fn, Log log_fn,
                       Store store, bool want_aux, Aux aux) {
  const int D = F + 2;
  for (int i = 0; i <= p; ++i) work[i * stride] = 0.0;
  for (int f = 0; f < F; ++f) {
    const double h = plp_compress(load(copy + f), w[f], compress_factor, floor, pow_fn);
    if (f == 0) {
      plp_accumulate(work, stride, B, D, p, 0, h);
      if (want_aux) aux(0, h);
    }
    plp_accumulate(work, stride, B, D, p, 1 + f, h);
    if (want_aux) aux(1 + f, h);
    if (f == F - 1) {
      plp_accumulate(work, stride, B, D, p, D - 1, h);
      if (want_aux) aux(D - 1, h);
    }
  }
  const double E = plp_recursions(work, stride, p);
  if (want_aux) aux(D, E);
  if (copy) {
    const double e0 = load(0);
    store(0, log_fn((e0 < floor) ? floor : e0));
  } else {
    store(0, L[0] * log_fn(E));
  }
  for (int k = 1; k < K; ++k) store(k, L[k] * work[(k - 1) * stride]);
}

}  // namespace pds
