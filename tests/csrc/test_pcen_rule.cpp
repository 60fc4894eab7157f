// Sweep of csrc/pcen_rule.h on the CPU: what the PCEN kernels share with the host.  Stand-alone (its own main), run
// plain and under the address and undefined-behaviour sanitizers by tests/test_pcen_rule.py.
//   - the lane -> (item, column) mapping and the lane and block counts against brute force, for item * column counts
//     around 255 / 256 / 257 and at counts past 2^32, and the refusal above 2^31 - 1 blocks;
//   - the smoother step and a lane's walk over an utterance (four loads ahead) against the plain recurrence, bit for
//     bit, with every load index checked to lie inside the utterance;
//   - pcen_compress runs with the host's pow here: it is compared with the formula written out, within a tolerance.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../pydrobert-speech_amd/csrc/pcen_rule.h"

using namespace pds;

static long g_checks = 0;

#define CHECK(cond)                                                      \
  do {                                                                   \
    ++g_checks;                                                          \
    if (!(cond)) {                                                       \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

static uint64_t bits(double x) {
  uint64_t u;
  std::memcpy(&u, &x, sizeof u);
  return u;
}

static bool same(double a, double b) { return (std::isnan(a) && std::isnan(b)) || bits(a) == bits(b); }

// a small generator of its own: the sweep must not depend on the C library's
static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t next_u64() {
  g_state ^= g_state << 13;
  g_state ^= g_state >> 7;
  g_state ^= g_state << 17;
  return g_state;
}
static double next_unit() { return (double)(next_u64() >> 11) / 9007199254740992.0; }

static void sweep_lane_mapping() {
  // every (items, C) whose product lies around a block's edge, and a few more: brute force walks items and columns in
  // the order the lanes must have
  for (int64_t items = 1; items <= 300; ++items) {
    for (int64_t C = 1; C <= 300; ++C) {
      const int64_t lanes = items * C;
      const bool edge = lanes >= 250 && lanes <= 262;
      if (!edge && !(items <= 7 && C <= 70) && !(lanes >= 505 && lanes <= 520)) continue;
      CHECK(pcen_lane_count(items, C) == lanes);
      const int64_t blocks = pcen_block_count(lanes);
      CHECK(blocks == (lanes + 255) / 256);
      CHECK(blocks * PCEN_THREADS >= lanes && (blocks - 1) * PCEN_THREADS < lanes);
      int64_t g = 0;
      for (int64_t b = 0; b < items; ++b) {
        for (int64_t c = 0; c < C; ++c, ++g) {
          int64_t item, column;
          pcen_lane_map(g, C, item, column);
          CHECK(item == b && column == c);
          CHECK(pcen_lane(g / PCEN_THREADS, (int)(g % PCEN_THREADS)) == g);
        }
      }
      CHECK(g == lanes);
      // the launch's last block: its lanes past `lanes` are the ones the kernels send away
      const int64_t last = pcen_lane(blocks - 1, PCEN_THREADS - 1);
      CHECK(last >= lanes - 1 && last < lanes - 1 + PCEN_THREADS);
    }
  }
  // B * C in {255, 256, 257} exactly, by every factorisation
  for (int64_t lanes = 255; lanes <= 257; ++lanes) {
    int seen = 0;
    for (int64_t C = 1; C <= lanes; ++C) {
      if (lanes % C) continue;
      ++seen;
      CHECK(pcen_lane_count(lanes / C, C) == lanes);
      CHECK(pcen_block_count(lanes) == (lanes == 257 ? 2 : 1));
    }
    CHECK(seen >= 2);
  }
}

static void sweep_large_counts() {
  // counts past 2^32: the mapping at lanes no 32-bit index reaches, against wider arithmetic
  const int64_t shapes[][2] = {{(int64_t)1 << 20, (int64_t)1 << 13}, {((int64_t)1 << 31) - 1, 5},
                               {3000000007ll, 3},                   {((int64_t)1 << 31) - 1, 255},
                               {123456789, 4099}};
  for (const auto &s : shapes) {
    const int64_t items = s[0], C = s[1];
    const __int128 wide = (__int128)items * C;
    const int64_t lanes = pcen_lane_count(items, C);
    CHECK((__int128)lanes == wide && lanes > ((int64_t)1 << 32));
    const __int128 wide_blocks = (wide + 255) / 256;
    const int64_t blocks = pcen_block_count(lanes);
    if (wide_blocks > PCEN_MAX_BLOCKS) {
      CHECK(blocks == -1);
    } else {
      CHECK((__int128)blocks == wide_blocks);
    }
    const int64_t probes[] = {0, 1, C - 1, C, C + 1, ((int64_t)1 << 32) - 1, (int64_t)1 << 32, ((int64_t)1 << 32) + 1,
                              lanes - C - 1, lanes - C, lanes - 2, lanes - 1};
    for (int64_t g : probes) {
      if (g < 0 || g >= lanes) continue;
      int64_t item, column;
      pcen_lane_map(g, C, item, column);
      CHECK(item >= 0 && item < items && column >= 0 && column < C);
      CHECK((__int128)item * C + column == (__int128)g);
      CHECK(pcen_lane(g / PCEN_THREADS, (int)(g % PCEN_THREADS)) == g);
    }
    for (int n = 0; n < 2000; ++n) {
      const int64_t g = (int64_t)(next_u64() % (uint64_t)lanes);
      int64_t item, column;
      pcen_lane_map(g, C, item, column);
      CHECK(column >= 0 && column < C && (__int128)item * C + column == (__int128)g);
    }
  }
  // the refusal: 2^31 - 1 blocks are launched, one lane more is not
  const int64_t most = PCEN_MAX_BLOCKS * PCEN_THREADS;
  CHECK(pcen_block_count(most) == PCEN_MAX_BLOCKS);
  CHECK(pcen_block_count(most - 255) == PCEN_MAX_BLOCKS);
  CHECK(pcen_block_count(most - 256) == PCEN_MAX_BLOCKS - 1);
  CHECK(pcen_block_count(most + 1) == -1);
  CHECK(pcen_block_count(std::numeric_limits<int64_t>::max()) == -1);
  CHECK(pcen_block_count(-1) == -1 && pcen_block_count(0) == 0 && pcen_block_count(1) == 1);
  // ... and the lane count that does not fit 64 bits
  CHECK(pcen_lane_count((int64_t)1 << 32, (int64_t)1 << 31) == -1);
  CHECK(pcen_lane_count(std::numeric_limits<int64_t>::max(), 2) == -1);
  CHECK(pcen_lane_count(std::numeric_limits<int64_t>::max(), 1) == std::numeric_limits<int64_t>::max());
  CHECK(pcen_lane_count(-1, 4) == -1 && pcen_lane_count(4, -1) == -1);
  CHECK(pcen_lane_count(0, 40) == 0 && pcen_lane_count(40, 0) == 0);
}

// the plain recurrence, written apart from the header: volatile keeps every operation a rounding of its own
static std::vector<double> plain_smoother(const std::vector<double> &e, double oms, double smooth) {
  std::vector<double> m(e.size());
  for (size_t t = 0; t < e.size(); ++t) {
    if (t == 0) {
      m[t] = e[t];
      continue;
    }
    volatile double kept = oms * m[t - 1];
    volatile double fresh = smooth * e[t];
    volatile double sum = kept + fresh;
    m[t] = sum;
  }
  return m;
}

static void sweep_smoother() {
  const double smooths[] = {0.025, 1.0, 0.5, 1e-3, 0.9999999, 0.024689453048712014};
  const int64_t lengths[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 257, 1000};
  long walks = 0;
  for (double smooth : smooths) {
    volatile double one = 1.0;
    const double oms = one - smooth;
    for (int64_t Tn : lengths) {
      for (int variant = 0; variant < 4; ++variant) {
        std::vector<double> e((size_t)Tn);
        for (auto &x : e) {
          const double mag = std::exp((next_unit() * 2 - 1) * 13.8);  // 1e-6 .. 1e6
          x = next_unit() < 0.1 ? 0.0 : (variant == 1 ? (double)(float)mag : mag);
        }
        if (variant == 2 && Tn > 2) e[(size_t)(Tn / 2)] = std::numeric_limits<double>::quiet_NaN();
        if (variant == 3 && Tn > 2) e[(size_t)(Tn / 3)] = std::numeric_limits<double>::infinity();
        const std::vector<double> want = plain_smoother(e, oms, smooth);
        std::vector<double> got((size_t)Tn, -1.0);
        std::vector<int> stored((size_t)Tn, 0);
        int64_t next_store = 0, loads = 0;
        pcen_smooth_walk(
            Tn, oms, smooth,
            [&](int64_t t) {
              CHECK(t >= 0 && t < Tn);  // no load outside the utterance, the tail of the unroll included
              ++loads;
              return e[(size_t)t];
            },
            [&](int64_t t, double m) {
              CHECK(t == next_store);  // in row order, every row once
              ++next_store;
              ++stored[(size_t)t];
              got[(size_t)t] = m;
            });
        CHECK(next_store == Tn);
        CHECK(loads == (Tn + PCEN_AHEAD - 1) / PCEN_AHEAD * PCEN_AHEAD);
        for (int64_t t = 0; t < Tn; ++t) {
          CHECK(stored[(size_t)t] == 1);
          CHECK(same(got[(size_t)t], want[(size_t)t]));
          if (smooth == 1.0 && variant < 2) CHECK(same(got[(size_t)t], e[(size_t)t]));  // oms = 0: M = E
        }
        if (variant == 2 && Tn > 2)
          for (int64_t t = Tn / 2; t < Tn; ++t) CHECK(std::isnan(got[(size_t)t]));  // a one-pole filter does not forget
        if (variant == 3 && Tn > 2 && smooth < 1.0)
          for (int64_t t = Tn / 3; t < Tn; ++t) CHECK(std::isinf(got[(size_t)t]) || std::isnan(got[(size_t)t]));
        ++walks;
      }
    }
    // the step and the first row
    CHECK(same(pcen_smooth_row(true, oms, smooth, 123.0, 7.5), 7.5));
    CHECK(same(pcen_smooth_row(false, oms, smooth, 123.0, 7.5), pcen_smooth_step(oms, smooth, 123.0, 7.5)));
    volatile double kept = oms * 123.0, fresh = smooth * 7.5;
    volatile double sum = kept + fresh;
    CHECK(same(pcen_smooth_step(oms, smooth, 123.0, 7.5), sum));
  }
  std::printf("%ld walks of the PCEN smoother checked\n", walks);
}

static void sweep_compress() {
  // (the host's pow: close to the formula written out, and exactly its closed forms where pow is exact)
  for (int n = 0; n < 20000; ++n) {
    const double e = std::exp((next_unit() * 2 - 1) * 13.8), m = std::exp((next_unit() * 2 - 1) * 13.8);
    const double gain = next_unit(), bias = next_unit() * 4, power = 0.05 + next_unit(), eps = 1e-6;
    const double bp = std::pow(bias, power);
    const double y = pcen_compress(e, m, gain, bias, power, eps, bp);
    const double want = std::pow(e / std::pow(eps + m, gain) + bias, power) - bp;
    CHECK(std::isfinite(y));
    CHECK(std::fabs(y - want) <= 1e-12 * (std::fabs(want) + 1.0));
  }
  CHECK(pcen_compress(0.0, 5.0, 0.98, 0.0, 0.5, 1e-6, 0.0) == 0.0);
  CHECK(pcen_compress(9.0, 1.0, 0.0, 0.0, 0.5, 1e-6, 0.0) == 3.0);  // gain 0: no gain control
  CHECK(std::isnan(pcen_compress(std::numeric_limits<double>::quiet_NaN(), 1.0, 0.98, 2.0, 0.5, 1e-6, std::sqrt(2.0))));
}

int main() {
  sweep_lane_mapping();
  sweep_large_counts();
  sweep_smoother();
  sweep_compress();
  std::printf("%ld checks of the PCEN rule passed\n", g_checks);
  return 0;
}
