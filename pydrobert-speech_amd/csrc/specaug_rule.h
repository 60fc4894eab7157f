// The rule of SpecAugment (include/pds_amd_stages3.h, post.SpecAugment): host and device, no dependencies but <math.h>.
// Shared by the kernels of specaug.hip and by tests/csrc/test_specaug_rule.cpp, which sweeps it on the CPU.  Every
// float64 operation here is rounded by itself: a translation unit that includes this is built without contraction.
// The library shares no header with the other three, so Philox4x32-10 is restated here (the round function is the one
// of dither_noise.h).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PDS_SA_HD __host__ __device__ __forceinline__
#else
#define PDS_SA_HD inline
#endif

namespace pds {

constexpr int SPECAUG_THREADS = 256;                 // lanes of a block of every kernel of the library
constexpr int SPECAUG_WAVE = 64;                     // lanes of a wave: the partial sums of the mean
constexpr int SPECAUG_ROWS = 32;                     // rows of a block's tile of the apply kernel
constexpr int SPECAUG_MAX_MASKS = 16;                // frequency masks, and time masks, at the most
constexpr int SPECAUG_PLAN_MAX = 2 + 4 * SPECAUG_MAX_MASKS;  // int64 words of the longest plan row
constexpr int SPECAUG_AHEAD = 16;                    // loads in flight per lane of the mean
constexpr int64_t SPECAUG_MAX_BLOCKS = 0x7fffffff;   // blocks one launch may have: 2^31 - 1
constexpr int64_t SPECAUG_MAX_T = 0x7fffffff;        // rows of an utterance the draws are defined for: U takes n < 2^31
constexpr int64_t SPECAUG_MAX_WIDTH = 0x7ffffffe;    // freq_width and time_width at the most: 2^31 - 2
constexpr int64_t SPECAUG_MAX_WARP = (int64_t)1 << 29;

// ---- step 0: the generator ------------------------------------------------------------------------------------------

// Philox4x32-10 (Salmon et al., SC'11) on counter c under key (k0, k1), in place
PDS_SA_HD void specaug_philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
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

// P(i, d): the block with counter words (i, 0, d, 0) under the utterance's key; r[0..3] are its output words
PDS_SA_HD void specaug_draw(uint32_t i, uint32_t d, uint64_t key, uint32_t r[4]) {
  r[0] = i; r[1] = 0u; r[2] = d; r[3] = 0u;
  specaug_philox(r, (uint32_t)key, (uint32_t)(key >> 32));
}

// U(r, n) = (r * (n + 1)) >> 32 for 0 <= n < 2^31: an integer in [0, n]
PDS_SA_HD int64_t specaug_uniform(uint32_t r, int64_t n) { return (int64_t)(((uint64_t)r * (uint64_t)(n + 1)) >> 32); }

// ---- steps 1 to 3: the plan of one utterance ------------------------------------------------------------------------

// int64 words of a plan row: w0, w1, (f0, f) per frequency mask, (t0, t) per time mask
PDS_SA_HD int32_t specaug_plan_words(int32_t freq_masks, int32_t time_masks) { return 2 + 2 * freq_masks + 2 * time_masks; }

// The plan of an utterance of T rows and C columns under `key` into plan[0 .. specaug_plan_words).  T == 0, and a T the
// draws are not defined for (above SPECAUG_MAX_T: the Python layer refuses it), give -1, -1 and zeros: nothing changes
PDS_SA_HD void specaug_plan_one(int64_t T, int64_t C, uint64_t key, int32_t freq_masks, int64_t freq_width,
                                int32_t time_masks, int64_t time_width, double time_ratio, int64_t W, int64_t *plan) {
  const int32_t words = specaug_plan_words(freq_masks, time_masks);
  plan[0] = plan[1] = -1;
  for (int32_t k = 2; k < words; ++k) plan[k] = 0;
  if (T <= 0 || T > SPECAUG_MAX_T || C <= 0) return;
  uint32_t r[4];
  if (W >= 1 && T >= 2 * W + 3) {
    specaug_draw(0u, 1u, key, r);
    const int64_t w0 = W + 1 + specaug_uniform(r[0], T - 3 - 2 * W);
    plan[0] = w0;
    plan[1] = w0 - W + specaug_uniform(r[1], 2 * W);
  }
  for (int32_t j = 0; j < freq_masks; ++j) {
    specaug_draw((uint32_t)j, 2u, key, r);
    const int64_t f = specaug_uniform(r[0], freq_width < C ? freq_width : C);
    plan[2 + 2 * j] = specaug_uniform(r[1], C - f);
    plan[3 + 2 * j] = f;
  }
  const double scaled = time_ratio * (double)T;  // the product rounded once
  int64_t bound = (int64_t)floor(scaled);
  if (time_width < bound) bound = time_width;
  int64_t *tm = plan + 2 + 2 * freq_masks;
  for (int32_t j = 0; j < time_masks; ++j) {
    specaug_draw((uint32_t)j, 3u, key, r);
    const int64_t t = specaug_uniform(r[0], bound);
    tm[2 * j] = specaug_uniform(r[1], T - t);
    tm[2 * j + 1] = t;
  }
}

// ---- step 4: the source position ------------------------------------------------------------------------------------

// A plan's warp is taken only where it keeps every source row inside the utterance: 1 <= w0, w1 <= T - 2.  Drawn plans
// always are (or are -1, -1); a plan a caller wrote by hand that is not is treated as no warp
PDS_SA_HD bool specaug_warps(int64_t T, int64_t w0, int64_t w1) {
  return T <= SPECAUG_MAX_T && w0 >= 1 && w1 >= 1 && w0 <= T - 2 && w1 <= T - 2;
}

// s of row t: a product, a quotient and (behind the centre) a sum, each rounded once; i = floor(s), a = s - i
PDS_SA_HD void specaug_source(int64_t t, int64_t T, int64_t w0, int64_t w1, int64_t &i, double &a) {
  double s;
  if (t <= w1) {
    const double num = (double)t * (double)w0;
    s = num / (double)w1;
  } else {
    const double num = (double)(t - w1) * (double)(T - 1 - w0);
    const double q = num / (double)(T - 1 - w1);
    s = (double)w0 + q;
  }
  const double fl = floor(s);
  i = (int64_t)fl;
  a = s - fl;
}

// row t lies in [t0, t0 + n): written so that no plan word, however wrong, overflows
PDS_SA_HD bool specaug_in_span(int64_t x, int64_t x0, int64_t n) {
  return n > 0 && x >= x0 && (uint64_t)x - (uint64_t)x0 < (uint64_t)n;
}

struct SpecaugRow {
  int64_t i;    // the source row
  double a;     // the weight of row i + 1 (0: row i is copied)
  bool masked;  // the row lies in a time mask
};

// What row t of an utterance of T rows needs of its plan.  The source row is kept inside the utterance whatever the
// plan says (i + 1 <= T - 1 whenever a > 0 is a property of the definition, swept on the CPU; the guard never acts on
// a plan that specaug_warps admits)
PDS_SA_HD SpecaugRow specaug_row(int64_t t, int64_t T, const int64_t *plan, int32_t freq_masks, int32_t time_masks) {
  SpecaugRow row;
  row.i = t;
  row.a = 0.0;
  row.masked = false;
  const int64_t *tm = plan + 2 + 2 * freq_masks;
  for (int32_t j = 0; j < time_masks; ++j) row.masked = row.masked || specaug_in_span(t, tm[2 * j], tm[2 * j + 1]);
  if (!row.masked && specaug_warps(T, plan[0], plan[1])) {
    specaug_source(t, T, plan[0], plan[1], row.i, row.a);
    if (row.i < 0) { row.i = 0; row.a = 0.0; }
    if (row.i >= T - 1) { row.i = T - 1; row.a = 0.0; }
  }
  return row;
}

// column c lies in a frequency mask of the plan
PDS_SA_HD bool specaug_column_masked(int64_t c, const int64_t *plan, int32_t freq_masks) {
  bool masked = false;
  for (int32_t j = 0; j < freq_masks; ++j) masked = masked || specaug_in_span(c, plan[2 + 2 * j], plan[3 + 2 * j]);
  return masked;
}

// x0 + a * (x1 - x0): the samples widened exactly, the difference, the product and the sum each rounded once
PDS_SA_HD double specaug_mix(double x0, double x1, double a) {
  const double diff = x1 - x0;
  const double part = a * diff;
  return x0 + part;
}

// ---- the walk of a block of the apply kernel over its tile ----------------------------------------------------------

// Lane `thread` of a block over a tile of `rows` rows of C columns: visit(r, c) for the elements it owns, 0 <= r <
// rows, 0 <= c < C.  The tile's elements are dealt in row-major order, SPECAUG_THREADS at a time: adjacent lanes take
// adjacent columns and go on from the end of one row to the start of the next, so narrow rows fill a wave too.  One
// division at the start; every step after it is additions (no product rows * C is formed, whatever C).  (A form that
// took four elements' loads before their stores was measured 6 to 24 % slower: DESIGN.md section 4.10.)
template <typename Visit>
PDS_SA_HD void specaug_tile_walk(int thread, int32_t rows, int64_t C, Visit visit) {
  int64_t r, c, dr, dc;
  if (C > SPECAUG_THREADS) {
    r = 0; c = thread; dr = 0; dc = SPECAUG_THREADS;
  } else {
    const int32_t Cn = (int32_t)C;
    r = thread / Cn; c = thread % Cn; dr = SPECAUG_THREADS / Cn; dc = SPECAUG_THREADS % Cn;
  }
  while (r < rows) {
    visit((int32_t)r, c);
    c += dc;
    r += dr;
    if (c >= C) { c -= C; ++r; }
  }
}

// ---- step 5: the mean -----------------------------------------------------------------------------------------------

// the partial sum that owns flat element e = t * C + c
PDS_SA_HD int32_t specaug_sum_owner(int64_t e) { return (int32_t)(e & (SPECAUG_WAVE - 1)); }

// p_lane of an utterance of T rows and C columns: its elements in ascending e from +0.0.  load(t, c) gives x[t][c]
// widened.  SPECAUG_AHEAD loads at a time, without a condition (a position past the end repeats the group's first,
// which is not added) and so in flight together, then the additions in order
template <typename Load>
PDS_SA_HD double specaug_lane_sum(int lane, int64_t T, int64_t C, Load load) {
  int64_t t, c, dr, dc;
  if (C > SPECAUG_WAVE) {
    t = 0; c = lane; dr = 0; dc = SPECAUG_WAVE;
  } else {
    const int32_t Cn = (int32_t)C;
    t = lane / Cn; c = lane % Cn; dr = SPECAUG_WAVE / Cn; dc = SPECAUG_WAVE % Cn;
  }
  double p = 0.0;
  while (t < T) {
    double v[SPECAUG_AHEAD];
    int n = 0;
    const int64_t t_first = t, c_first = c;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int u = 0; u < SPECAUG_AHEAD; ++u) {
      const bool in = t < T;
      v[u] = load(in ? t : t_first, in ? c : c_first);
      n += in;
      c += dc;
      t += dr;
      if (c >= C) { c -= C; ++t; }
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int u = 0; u < SPECAUG_AHEAD; ++u)
      if (u < n) p = p + v[u];
  }
  return p;
}

// m = (((+0.0 + p_0) + p_1) + ... + p_63) / (T * C); NaN for T * C == 0
PDS_SA_HD double specaug_combine(const double *p, int64_t T, int64_t C) {
  double s = 0.0;
  for (int j = 0; j < SPECAUG_WAVE; ++j) s = s + p[j];
  return s / (double)(T * C);
}

// ---- grids, in 64 bits ----------------------------------------------------------------------------------------------

// blocks of SPECAUG_THREADS lanes with one lane per utterance (the plan); -1 for a negative count
PDS_SA_HD int64_t specaug_plan_blocks(int64_t B) {
  if (B < 0) return -1;
  return B / SPECAUG_THREADS + (B % SPECAUG_THREADS != 0);
}

// blocks with one wave per utterance (the mean); -1 for a negative count
PDS_SA_HD int64_t specaug_mean_blocks(int64_t B) {
  constexpr int waves = SPECAUG_THREADS / SPECAUG_WAVE;
  if (B < 0) return -1;
  return B / waves + (B % waves != 0);
}

// tiles of SPECAUG_ROWS rows that cover the longest utterance; -1 for a negative count
PDS_SA_HD int64_t specaug_tiles(int64_t max_rows) {
  if (max_rows < 0) return -1;
  return max_rows / SPECAUG_ROWS + (max_rows % SPECAUG_ROWS != 0);
}

// blocks of the apply kernel, one per (utterance, tile); -1 above 2^31 - 1 blocks (the caller refuses the launch: the
// batch is split) and for a negative count
PDS_SA_HD int64_t specaug_apply_blocks(int64_t B, int64_t tiles) {
  if (B < 0 || tiles < 0) return -1;
  if (B == 0 || tiles == 0) return 0;
  if (tiles > SPECAUG_MAX_BLOCKS / B) return -1;
  return B * tiles;
}

}  // namespace pds
