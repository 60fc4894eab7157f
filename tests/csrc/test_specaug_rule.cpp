// Sweep of the rule the SpecAugment kernels share (pydrobert-speech_amd/csrc/specaug_rule.h) on the CPU: Philox known
// answers, U's range, the plan's invariants, the source position's properties, a block's walk over its tile and a
// wave's partial sums, lane by lane through bounds-checked vectors against brute force, and the grid arithmetic at its
// refusal bounds.  Stand-alone: g++ -std=c++17 -ffp-contract=off, plain and under the address and undefined-behaviour
// sanitizers (tests/test_specaug_rule.py).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../pydrobert-speech_amd/csrc/specaug_rule.h"

using namespace pds;

static long g_checks = 0;

#define CHECK(cond)                                                       \
  do {                                                                    \
    ++g_checks;                                                           \
    if (!(cond)) {                                                        \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
      exit(1);                                                            \
    }                                                                     \
  } while (0)

static uint64_t mix64(uint64_t &state) {  // splitmix64: the sweep's own source of keys and data
  uint64_t z = (state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static void known_answers() {
  // Random123's known answers for philox4x32-10: counter, key -> output
  uint32_t a[4] = {0, 0, 0, 0};
  specaug_philox(a, 0u, 0u);
  CHECK(a[0] == 0x6627e8d5u && a[1] == 0xe169c58du && a[2] == 0xbc57ac4cu && a[3] == 0x9b00dbd8u);
  uint32_t b[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  specaug_philox(b, 0xffffffffu, 0xffffffffu);
  CHECK(b[0] == 0x408f276du && b[1] == 0x41c83b0eu && b[2] == 0xa20bc7c6u && b[3] == 0x6d5451fdu);
  uint32_t c[4] = {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u};
  specaug_philox(c, 0xa4093822u, 0x299f31d0u);
  CHECK(c[0] == 0xd16cfe09u && c[1] == 0x94fdccebu && c[2] == 0x5001e420u && c[3] == 0x24126ea1u);
  // P(i, d) is the block with counter (i, 0, d, 0) and key (k mod 2^32, k >> 32)
  uint32_t r[4], want[4] = {5u, 0u, 3u, 0u};
  specaug_draw(5u, 3u, 0x299f31d0a4093822ull, r);
  specaug_philox(want, 0xa4093822u, 0x299f31d0u);
  CHECK(memcmp(r, want, sizeof r) == 0);
}

static void uniform_range() {
  const uint32_t rs[] = {0u, 1u, 0x7fffffffu, 0x80000000u, 0xffffffffu};
  const int64_t ns[] = {0, 1, 7, 0x7ffffffe, 0x7fffffff};
  for (uint32_t r : rs)
    for (int64_t n : ns) {
      const int64_t u = specaug_uniform(r, n);
      CHECK(u >= 0 && u <= n);
    }
  CHECK(specaug_uniform(0u, 0x7fffffff) == 0 && specaug_uniform(0xffffffffu, 0x7fffffff) == 0x7fffffff);
  CHECK(specaug_uniform(0xffffffffu, 0) == 0 && specaug_uniform(0xffffffffu, 7) == 7);
}

static long plan_invariants() {
  uint64_t state = 1;
  long plans = 0;
  const int64_t widths[] = {1, 13, 40, 65};
  int64_t plan[SPECAUG_PLAN_MAX];
  for (int64_t T = 0; T <= 300; ++T)
    for (int64_t W = 0; W <= 8; ++W)
      for (int k = 0; k < 6; ++k) {
        const uint64_t key = mix64(state);
        const int64_t C = widths[(T + W + k) % 4];
        const int32_t F = (int32_t)(mix64(state) % 17), N = (int32_t)(mix64(state) % 17);
        const int64_t fw = (k & 1) ? 2 * C + 3 : (int64_t)(mix64(state) % (uint64_t)(C + 1));
        const int64_t tw = (k & 2) ? SPECAUG_MAX_WIDTH : (int64_t)(mix64(state) % 60);
        const double ratio = k == 5 ? 1e-3 : (k == 4 ? 0.2 : 1.0);
        for (int j = 0; j < SPECAUG_PLAN_MAX; ++j) plan[j] = 0x5555555555555555ll;
        specaug_plan_one(T, C, key, F, fw, N, tw, ratio, W, plan);
        ++plans;
        const int32_t words = specaug_plan_words(F, N);
        CHECK(words == 2 + 2 * F + 2 * N && words <= SPECAUG_PLAN_MAX);
        for (int j = words; j < SPECAUG_PLAN_MAX; ++j) CHECK(plan[j] == 0x5555555555555555ll);  // nothing past the row
        if (T == 0) {
          CHECK(plan[0] == -1 && plan[1] == -1);
          for (int j = 2; j < words; ++j) CHECK(plan[j] == 0);
          continue;
        }
        if (W >= 1 && T >= 2 * W + 3) {
          CHECK(plan[0] >= W + 1 && plan[0] <= T - 2 - W && plan[1] >= 1 && plan[1] <= T - 2);
          CHECK(plan[1] >= plan[0] - W && plan[1] <= plan[0] + W && specaug_warps(T, plan[0], plan[1]));
        } else {
          CHECK(plan[0] == -1 && plan[1] == -1 && !specaug_warps(T, plan[0], plan[1]));
        }
        for (int j = 0; j < F; ++j) {
          const int64_t f0 = plan[2 + 2 * j], f = plan[3 + 2 * j];
          CHECK(f >= 0 && f <= fw && f <= C && f0 >= 0 && f0 + f <= C);
        }
        const int64_t bound = (int64_t)floor(ratio * (double)T) < tw ? (int64_t)floor(ratio * (double)T) : tw;
        for (int j = 0; j < N; ++j) {
          const int64_t t0 = plan[2 + 2 * F + 2 * j], t = plan[3 + 2 * F + 2 * j];
          CHECK(t >= 0 && t <= bound && t0 >= 0 && t0 + t <= T);
        }
      }
  // an utterance the draws are not defined for gets the plan of an empty one
  specaug_plan_one(SPECAUG_MAX_T + 1, 40, 7, 2, 10, 2, 50, 1.0, 5, plan);
  CHECK(plan[0] == -1 && plan[1] == -1 && plan[2] == 0 && plan[9] == 0);
  specaug_plan_one(SPECAUG_MAX_T, 40, 7, 2, 10, 2, SPECAUG_MAX_WIDTH, 1.0, SPECAUG_MAX_WARP, plan);
  CHECK(plan[0] >= SPECAUG_MAX_WARP + 1 && plan[0] <= SPECAUG_MAX_T - 2 - SPECAUG_MAX_WARP && plan[6] + plan[7] <= SPECAUG_MAX_T);
  return plans;
}

static long source_positions() {
  long positions = 0;
  for (int64_t T = 3; T <= 64; ++T)
    // every centre specaug_warps admits: the drawn ones (|w1 - w0| <= W) and every plan a caller may write
    for (int64_t w0 = 1; w0 <= T - 2; ++w0)
      for (int64_t w1 = 1; w1 <= T - 2; ++w1) {
        CHECK(specaug_warps(T, w0, w1));
        double prev = -1.0;
        for (int64_t t = 0; t < T; ++t) {
          int64_t i;
          double a;
          specaug_source(t, T, w0, w1, i, a);
          const double s = (double)i + a;
          ++positions;
          CHECK(s > prev);  // strictly increasing
          prev = s;
          CHECK(a >= 0.0 && a < 1.0 && i >= 0 && i <= T - 1);
          if (a > 0.0) CHECK(i + 1 <= T - 1);
          if (t == 0) CHECK(i == 0 && a == 0.0);
          if (t == w1) CHECK(i == w0 && a == 0.0);
          if (t == T - 1) CHECK(i == T - 1 && a == 0.0);
          if (w0 == w1) CHECK(i == t && a == 0.0);  // the identity
          // the guard of specaug_row never acts
          int64_t plan[2] = {w0, w1};
          const SpecaugRow row = specaug_row(t, T, plan, 0, 0);
          CHECK(row.i == i && row.a == a && !row.masked);
        }
      }
  // at the size limits the arithmetic stays exact at the fixed points
  const int64_t T = SPECAUG_MAX_T, w0 = T - 2, w1 = 1;
  int64_t i;
  double a;
  specaug_source(0, T, w0, w1, i, a);
  CHECK(i == 0 && a == 0.0);
  specaug_source(w1, T, w0, w1, i, a);
  CHECK(i == w0 && a == 0.0);
  specaug_source(T - 1, T, w0, w1, i, a);
  CHECK(i == T - 1 && a == 0.0);
  // what is no warp: a centre outside [1, T - 2], any T
  CHECK(!specaug_warps(5, 0, 1) && !specaug_warps(5, 1, 4) && !specaug_warps(5, -1, -1) && !specaug_warps(2, 1, 1));
  CHECK(!specaug_warps(5, INT64_MAX, 1) && !specaug_warps(5, 1, INT64_MIN) && !specaug_warps(SPECAUG_MAX_T + 1, 1, 1));
  // mask words, however wrong, only compare
  CHECK(!specaug_in_span(3, INT64_MIN, INT64_MAX) && specaug_in_span(-5, INT64_MIN, INT64_MAX));
  CHECK(specaug_in_span(3, 3, 1) && !specaug_in_span(4, 3, 1) && !specaug_in_span(2, 3, 1) && !specaug_in_span(3, 3, 0));
  CHECK(!specaug_in_span(3, 3, -5) && specaug_in_span(3, -4, INT64_MAX) && !specaug_in_span(3, INT64_MAX, INT64_MAX));
  return positions;
}

// one block of the apply kernel over its tile, as specaug.hip runs it, through bounds-checked vectors
static void block_apply(const std::vector<float> &in, int64_t in_stride, int64_t r0, int64_t Tn, int64_t tile, int64_t C,
                        const std::vector<int64_t> &plan, int32_t F, int32_t N, float fill, std::vector<float> &out,
                        int64_t out_stride, std::vector<int> &visits) {
  const int64_t t0 = tile * SPECAUG_ROWS;
  if (t0 >= Tn) return;
  const int32_t rows = (int32_t)(Tn - t0 < SPECAUG_ROWS ? Tn - t0 : SPECAUG_ROWS);
  std::vector<SpecaugRow> info;
  for (int32_t r = 0; r < rows; ++r) info.push_back(specaug_row(t0 + r, Tn, plan.data(), F, N));
  for (int thread = 0; thread < SPECAUG_THREADS; ++thread)
    specaug_tile_walk(thread, rows, C, [&](int32_t r, int64_t c) {
      CHECK(r >= 0 && r < rows && c >= 0 && c < C);
      float v = fill;
      const SpecaugRow &row = info.at(r);
      if (!row.masked && !specaug_column_masked(c, plan.data(), F)) {
        v = in.at((r0 + row.i) * in_stride + c);
        if (row.a != 0.0)
          v = (float)specaug_mix((double)v, (double)in.at((r0 + row.i + 1) * in_stride + c), row.a);
      }
      out.at((r0 + t0 + r) * out_stride + c) = v;
      ++visits.at((r0 + t0 + r) * out_stride + c);
    });
}

// x in [x0, x0 + n) in arithmetic wide enough for any plan word
static bool in_wide(int64_t x, int64_t x0, int64_t n) { return (__int128)x >= x0 && (__int128)x < (__int128)x0 + n; }

static long tile_walks() {
  uint64_t state = 2;
  long walks = 0;
  const int64_t widths[] = {1, 2, 3, 40, 63, 64, 65, 255, 256, 257, 700};
  const int64_t lengths[] = {1, 2, SPECAUG_ROWS - 1, SPECAUG_ROWS, SPECAUG_ROWS + 1, 2 * SPECAUG_ROWS + 1};
  for (int64_t C : widths)
    for (int64_t Tn : lengths)
      for (int variant = 0; variant < 4; ++variant) {
        const int64_t pad = variant & 1 ? 5 : 0, r0 = 3;
        const int64_t in_stride = C + pad, out_stride = C + (variant & 2 ? 2 : 0);
        const int32_t F = 2, N = 2;
        std::vector<int64_t> plan(specaug_plan_words(F, N));
        specaug_plan_one(Tn, C, mix64(state), F, 10, N, 20, 1.0, variant >= 2 ? 3 : 0, plan.data());
        if (variant == 3 && Tn >= 3) { plan[0] = Tn - 2; plan[1] = 1; }  // a plan written by hand, at an extreme
        if (variant == 1) { plan[0] = INT64_MAX; plan[1] = INT64_MIN; plan[2] = INT64_MIN; plan[3] = INT64_MAX; }
        std::vector<float> in((r0 + Tn + 2) * in_stride), out((r0 + Tn + 2) * out_stride, -77.0f), want(out);
        for (float &x : in) x = (float)((double)(int64_t)(mix64(state) % 2001) - 1000.0) / 8.0f;
        std::vector<int> visits(out.size(), 0);
        const int64_t tiles = specaug_tiles(Tn + 40);  // (a longer utterance in the batch: more tiles than this one has)
        for (int64_t tile = 0; tile < tiles; ++tile)
          block_apply(in, in_stride, r0, Tn, tile, C, plan, F, N, 0.5f, out, out_stride, visits);
        ++walks;
        // brute force: the definition element by element
        for (int64_t t = 0; t < Tn; ++t)
          for (int64_t c = 0; c < C; ++c) {
            bool masked = false;
            for (int j = 0; j < F; ++j) masked |= in_wide(c, plan[2 + 2 * j], plan[3 + 2 * j]);
            for (int j = 0; j < N; ++j) masked |= in_wide(t, plan[2 + 2 * F + 2 * j], plan[3 + 2 * F + 2 * j]);
            float v = 0.5f;
            if (!masked) {
              v = in[(r0 + t) * in_stride + c];
              if (plan[0] >= 1 && plan[0] <= Tn - 2 && plan[1] >= 1 && plan[1] <= Tn - 2) {
                int64_t i;
                double a;
                specaug_source(t, Tn, plan[0], plan[1], i, a);
                const double x0 = in[(r0 + i) * in_stride + c];
                v = a == 0.0 ? (float)x0 : (float)(x0 + a * ((double)in[(r0 + i + 1) * in_stride + c] - x0));
              }
            }
            want[(r0 + t) * out_stride + c] = v;
          }
        for (size_t k = 0; k < out.size(); ++k) {
          const int64_t row = (int64_t)k / out_stride, col = (int64_t)k % out_stride;
          const bool inside = row >= r0 && row < r0 + Tn && col < C;
          CHECK(visits[k] == (inside ? 1 : 0));  // every element once, nothing else touched
          CHECK(memcmp(&out[k], &want[k], sizeof(float)) == 0);
        }
      }
  return walks;
}

static long partial_sums() {
  uint64_t state = 3;
  long sums = 0;
  const int64_t shapes[][2] = {{1, 1}, {1, 63}, {63, 1}, {1, 64}, {64, 1}, {5, 13}, {65, 1}, {1, 65}, {17, 241},
                               {3, 64}, {7, 32}, {100, 40}, {9, 700}};
  for (const auto &shape : shapes)
    for (int pad = 0; pad < 2; ++pad) {
      const int64_t T = shape[0], C = shape[1], stride = C + 3 * pad;
      std::vector<double> x(T * stride);
      for (double &v : x) v = ldexp((double)(int64_t)(mix64(state) % 200001) - 100000.0, (int)(mix64(state) % 40) - 20);
      double want[SPECAUG_WAVE], got[SPECAUG_WAVE];
      for (int j = 0; j < SPECAUG_WAVE; ++j) want[j] = 0.0;
      for (int64_t e = 0; e < T * C; ++e) {
        const int j = specaug_sum_owner(e);
        CHECK(j == (int)(e % 64));
        want[j] = want[j] + x[(e / C) * stride + e % C];
      }
      std::vector<int> reads(x.size(), 0);
      for (int lane = 0; lane < SPECAUG_WAVE; ++lane)
        got[lane] = specaug_lane_sum(lane, T, C, [&](int64_t t, int64_t c) {
          CHECK(t >= 0 && t < T && c >= 0 && c < C);
          ++reads.at(t * stride + c);
          return x.at(t * stride + c);
        });
      CHECK(memcmp(want, got, sizeof want) == 0);
      double s = 0.0;
      for (int j = 0; j < SPECAUG_WAVE; ++j) s = s + want[j];
      const double m = specaug_combine(got, T, C), ref = s / (double)(T * C);
      CHECK(memcmp(&m, &ref, sizeof m) == 0);
      ++sums;
    }
  double zeros[SPECAUG_WAVE] = {0};
  CHECK(isnan(specaug_combine(zeros, 0, 40)));
  return sums;
}

static void grids() {
  CHECK(specaug_plan_blocks(-1) == -1 && specaug_plan_blocks(0) == 0 && specaug_plan_blocks(1) == 1);
  CHECK(specaug_plan_blocks(256) == 1 && specaug_plan_blocks(257) == 2 && specaug_plan_blocks(0x7fffffff) == 8388608);
  CHECK(specaug_mean_blocks(-1) == -1 && specaug_mean_blocks(0) == 0 && specaug_mean_blocks(4) == 1);
  CHECK(specaug_mean_blocks(5) == 2 && specaug_mean_blocks(0x7fffffff) == 536870912);
  CHECK(specaug_tiles(-1) == -1 && specaug_tiles(0) == 0 && specaug_tiles(1) == 1 && specaug_tiles(SPECAUG_ROWS) == 1);
  CHECK(specaug_tiles(SPECAUG_ROWS + 1) == 2 && specaug_tiles(SPECAUG_MAX_T) == (SPECAUG_MAX_T + SPECAUG_ROWS - 1) / SPECAUG_ROWS);
  CHECK(specaug_tiles(INT64_MAX) > 0);
  CHECK(specaug_apply_blocks(-1, 1) == -1 && specaug_apply_blocks(1, -1) == -1 && specaug_apply_blocks(0, 5) == 0);
  CHECK(specaug_apply_blocks(5, 0) == 0 && specaug_apply_blocks(3, 7) == 21);
  CHECK(specaug_apply_blocks(1, SPECAUG_MAX_BLOCKS) == SPECAUG_MAX_BLOCKS && specaug_apply_blocks(1, SPECAUG_MAX_BLOCKS + 1) == -1);
  CHECK(specaug_apply_blocks(SPECAUG_MAX_BLOCKS, 1) == SPECAUG_MAX_BLOCKS && specaug_apply_blocks(SPECAUG_MAX_BLOCKS, 2) == -1);
  CHECK(specaug_apply_blocks(65536, 32767) == (int64_t)65536 * 32767 && specaug_apply_blocks(65536, 32768) == -1);
  CHECK(specaug_apply_blocks(0x7fffffff, INT64_MAX) == -1 && specaug_apply_blocks(2, INT64_MAX) == -1);
  // the longest utterance always fits a launch of its own
  CHECK(specaug_apply_blocks(1, specaug_tiles(SPECAUG_MAX_T)) > 0);
}

int main() {
  known_answers();
  uniform_range();
  const long plans = plan_invariants();
  const long positions = source_positions();
  const long walks = tile_walks();
  const long sums = partial_sums();
  grids();
  printf("%ld plans, %ld source positions, %ld tile walks and %ld means of the SpecAugment rule checked\n", plans,
         positions, walks, sums);
  printf("%ld checks of the SpecAugment rule passed\n", g_checks);
  return 0;
}
