// CPU sweep of csrc/vad_rule.h, the rule the kernels of vad.hip share: the interleaved partial sums and their
// combination against the plain 64-term form bit for bit, the window and the vote against brute force, and the
// decision kernel's walk over an utterance -- chunks of 64 frames, two running counts, every load without a condition
// (through a bounds-checked vector) -- against a count over each frame's window.
// Built plain and with -fsanitize=address,undefined by tests/test_vad_rule.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../pydrobert-speech_amd/csrc/vad_rule.h"

static long failures = 0;
#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) {                        \
      if (failures < 20) {                \
        printf("FAILED %s: ", #cond);     \
        printf(__VA_ARGS__);              \
        printf("\n");                     \
      }                                   \
      ++failures;                         \
    }                                     \
  } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t next_u64() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
static double next_unit() { return (double)(next_u64() >> 11) / 9007199254740992.0; }

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// the definition, literally: 64 partials from +0.0, all 64 added in order from +0.0
static double plain_sum(const std::vector<double> &e) {
  double p[64];
  for (int j = 0; j < 64; ++j) p[j] = 0.0;
  for (size_t t = 0; t < e.size(); ++t) p[t % 64] = p[t % 64] + e[t];
  double s = 0.0;
  for (int j = 0; j < 64; ++j) s = s + p[j];
  return s;
}

static int popcount(uint64_t m) { return __builtin_popcountll(m); }

// the kernel's vote over one utterance: lanes 0 .. 63 of a wave in a loop, ballots as 64-bit masks
static void kernel_walk(const std::vector<double> &e, double thr, int64_t context, double proportion,
                        std::vector<int> &voiced, int64_t &total) {
  const int AHEAD = 4, WAVE = 64;
  const int64_t Tn = (int64_t)e.size(), last = Tn - 1;
  voiced.assign(Tn, -1);
  total = 0;
  int64_t lead = 0, lag = 0;
  const int64_t pre = context < Tn ? context : Tn;
  for (int64_t u0 = 0; u0 < pre; u0 += WAVE) {
    uint64_t m = 0;
    for (int lane = 0; lane < WAVE; ++lane) {
      const int64_t u = u0 + lane;
      const double v = e.at(u < pre ? u : pre - 1);
      if (u < pre && pds::vad_above(v, thr)) m |= (uint64_t)1 << lane;
    }
    lead += popcount(m);
  }
  for (int64_t t0 = 0; t0 < Tn; t0 += (int64_t)AHEAD * WAVE) {
    double hv[AHEAD][WAVE], lv[AHEAD][WAVE];
    for (int u = 0; u < AHEAD; ++u)
      for (int lane = 0; lane < WAVE; ++lane) {
        const int64_t t = t0 + u * WAVE + lane;
        const int64_t h = t + context, l = t - context;
        hv[u][lane] = e.at(h < Tn ? h : last);
        lv[u][lane] = context == 0 ? hv[u][lane] : e.at(l < 0 ? 0 : l < Tn ? l : last);
      }
    for (int u = 0; u < AHEAD; ++u) {
      if (t0 + u * WAVE >= Tn) break;
      uint64_t hm = 0, lm = 0, vm = 0;
      for (int lane = 0; lane < WAVE; ++lane) {
        const int64_t t = t0 + u * WAVE + lane;
        const int64_t h = t + context, l = t - context;
        if (h < Tn && pds::vad_above(hv[u][lane], thr)) hm |= (uint64_t)1 << lane;
        if (l >= 0 && l < Tn && pds::vad_above(lv[u][lane], thr)) lm |= (uint64_t)1 << lane;
      }
      for (int lane = 0; lane < WAVE; ++lane) {
        const int64_t t = t0 + u * WAVE + lane;
        const uint64_t below = ((uint64_t)1 << lane) - 1, upto = below | ((uint64_t)1 << lane);
        const int64_t upto_hi = lead + popcount(hm & upto), before_lo = lag + popcount(lm & below);
        if (t < Tn) {
          int64_t lo, hi;
          pds::vad_window(t, Tn, context, lo, hi);
          const bool v = pds::vad_vote(upto_hi - before_lo, hi - lo + 1, proportion);
          CHECK(voiced.at(t) == -1, "frame %lld written twice", (long long)t);
          voiced.at(t) = v ? 1 : 0;
          if (v) vm |= (uint64_t)1 << lane;
        }
      }
      lead += popcount(hm);
      lag += popcount(lm);
      total += popcount(vm);
    }
  }
}

int main() {
  long sums = 0, walks = 0;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  // ---- the sum -------------------------------------------------------------------------------------------------------
  for (int64_t T = 0; T <= 300; ++T) {
    for (int kind = 0; kind < 4; ++kind) {
      std::vector<double> e(T);
      for (auto &v : e) {
        const double mag = std::ldexp(next_unit() - 0.5, (int)(next_u64() % 60) - 30);
        v = kind == 0 ? mag : kind == 1 ? 20.0 + 5.0 * (next_unit() - 0.5) : kind == 2 ? -0.0 : (next_u64() % 3 ? mag : -0.0);
      }
      double p[64];
      for (int j = 0; j < 64; ++j) p[j] = pds::vad_partial_sum(T, j, [&](int64_t t) { return e.at(t); });
      for (int j = (int)std::min<int64_t>(T, 64); j < 64; ++j)
        CHECK(same_bits(p[j], 0.0), "partial %d of %lld energies is not +0.0", j, (long long)T);
      CHECK(pds::vad_partials_used(T) == std::min<int64_t>(T, 64), "T %lld", (long long)T);
      const double s = pds::vad_combine(T, [&](int j) { return p[j]; });
      CHECK(same_bits(s, plain_sum(e)), "T %lld kind %d: %a != %a", (long long)T, kind, s, plain_sum(e));
      CHECK(!std::signbit(s) || s != 0.0, "T %lld kind %d: the sum is -0.0", (long long)T, kind);
      ++sums;
    }
  }
  CHECK(pds::vad_partials_used(-5) == 0 && pds::vad_partials_used((int64_t)1 << 40) == 64, "vad_partials_used");
  // ---- the threshold: three roundings ---------------------------------------------------------------------------------
  {
    const double s = 1.0 + std::ldexp(1.0, -52), scale = 1.0 + std::ldexp(1.0, -30);
    volatile double prod = scale * s;
    volatile double mean = prod / 3.0;
    volatile double want = 5.0 + mean;
    CHECK(same_bits(pds::vad_threshold(5.0, scale, s, 3), want), "threshold");
    CHECK(std::isnan(pds::vad_threshold(5.0, 0.5, nan, 7)) && pds::vad_threshold(5.0, 0.5, inf, 7) == inf &&
              pds::vad_threshold(5.0, 0.5, -inf, 7) == -inf, "non-finite sums");
    CHECK(!pds::vad_above(nan, 1.0) && !pds::vad_above(1.0, nan) && !pds::vad_above(inf, inf) &&
              pds::vad_above(inf, 1.0) && !pds::vad_above(2.0, 2.0) && pds::vad_above(std::nextafter(2.0, 3.0), 2.0),
          "vad_above");
  }
  // ---- ties of the vote -------------------------------------------------------------------------------------------------
  CHECK(pds::vad_vote(1, 2, 0.5) && !pds::vad_vote(1, 2, std::nextafter(0.5, 1.0)) && pds::vad_vote(0, 1, 0.0) &&
            !pds::vad_vote(0, 1, 0.6) && pds::vad_vote(3, 5, 0.6) && !pds::vad_vote(2, 5, 0.6), "vad_vote");
  // ---- the window and the kernel's walk -----------------------------------------------------------------------------------
  for (int64_t T = 1; T <= 300; T += (T < 70 ? 1 : T < 140 ? 3 : 17)) {
    std::vector<double> e(T);
    std::vector<int64_t> contexts;
    for (int64_t c = 0; c <= 9; ++c) contexts.push_back(c);
    for (int64_t c : {(int64_t)63, (int64_t)64, (int64_t)65, (int64_t)130, T - 2, T - 1, T, T + 1, T + 3, T + 200,
                      (int64_t)0x7fffffff})
      if (c > 9) contexts.push_back(c);
    for (int64_t context : contexts) {
      for (int density = 0; density < 3; ++density) {
        for (auto &v : e) v = next_unit() < 0.15 + 0.35 * density ? 10.0 : (next_u64() % 9 ? 0.0 : nan);
        if (T > 2 && density == 1) e[T / 2] = 5.0;  // (equal to the threshold: not above it)
        const double thr = 5.0, proportion = density == 2 ? 0.5 : 0.6;
        std::vector<int> got;
        int64_t total;
        kernel_walk(e, thr, context, proportion, got, total);
        int64_t want_total = 0;
        for (int64_t t = 0; t < T; ++t) {
          int64_t lo, hi;
          pds::vad_window(t, T, context, lo, hi);
          const int64_t blo = std::max<int64_t>(0, t - context), bhi = std::min<int64_t>(T - 1, t + context);
          CHECK(lo == blo && hi == bhi, "window T %lld t %lld context %lld: [%lld, %lld]", (long long)T, (long long)t,
                (long long)context, (long long)lo, (long long)hi);
          int64_t num = 0, den = 0;
          for (int64_t u = t - std::min<int64_t>(context, T); u <= t + std::min<int64_t>(context, T); ++u)
            if (u >= 0 && u < T) {
              ++den;
              num += e[u] > thr;
            }
          const int want = (double)num >= (double)den * proportion;
          CHECK(got.at(t) == want, "T %lld t %lld context %lld: %d, %lld of %lld", (long long)T, (long long)t,
                (long long)context, got.at(t), (long long)num, (long long)den);
          want_total += want;
        }
        CHECK(total == want_total, "T %lld context %lld: count %lld != %lld", (long long)T, (long long)context,
              (long long)total, (long long)want_total);
        ++walks;
      }
    }
  }
  if (failures) {
    printf("%ld checks failed\n", failures);
    return 1;
  }
  printf("%ld sums and %ld walks of the VAD rule checked\n", sums, walks);
  return 0;
}
