// Sweep of csrc/plp_rule.h on the CPU: what the PLP kernel inlines.  Stand-alone (its own main), run plain and under
// the address and undefined-behaviour sanitizers by tests/test_plp_rule.py.
//   - plp_row (the row streamed through, t of Durbin's step never stored, q written over r) against the definition
//     written out plainly (d stored, the sums taken one r[i] at a time, t an array of its own), bit for bit, over
//     F in {1, 2, 23, 40, 254}, p in {1, 2, 12, min(F + 1, 32)}, K in {1, p + 1}, with and without the energy column and
//     the auxiliary output, with the working words 1 and 64 apart; every array is exactly as long as the rule may
//     touch, and the other lanes' words of the element-major storage must keep their values;
//   - the known answers: r[i] = 0.5^i gives a = (-0.5, 0, ...), E = 0.75 and q[n-1] = 0.5^n / n exactly; a row of
//     1 / w[f] gives |out| < 1e-12; r = (1, 1, ...) engages the clamp; a NaN row is NaN in every computed column; a
//     row of zeros is finite;
//   - the lane -> row mapping, the block count and its refusal above 2^31 - 1 blocks, the LDS bytes, the shape check.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../pydrobert-speech_amd/csrc/plp_rule.h"

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

static const double PI = 3.14159265358979323846;

struct Tables {
  std::vector<double> w, B, L;
};

static Tables tables(int F, int p, int K, double lifter, double scale, bool loud) {
  Tables t;
  const int D = F + 2;
  t.w.resize(F);
  for (int f = 0; f < F; ++f) {
    if (!loud) {
      t.w[f] = 1.0;
      continue;
    }
    const double c = 60.0 + 7900.0 * (f + 0.5) / F;
    const double fsq = c * c, fs = fsq / (fsq + 1.6e5);
    t.w[f] = fs * fs * ((fsq + 1.44e6) / (fsq + 9.61e6));
  }
  t.B.resize((size_t)(p + 1) * D);
  const double s = 1.0 / (2.0 * (D - 1)), theta = PI / (D - 1);
  for (int i = 0; i <= p; ++i) {
    t.B[(size_t)i * D] = s;
    for (int j = 1; j < D - 1; ++j) t.B[(size_t)i * D + j] = 2.0 * s * std::cos(theta * i * j);
    t.B[(size_t)i * D + D - 1] = s * std::cos(theta * i * (D - 1));
  }
  t.L.resize(K);
  for (int k = 0; k < K; ++k) t.L[k] = lifter > 0.0 ? scale * (1.0 + 0.5 * lifter * std::sin(PI * k / lifter)) : scale;
  return t;
}

// the definition written out plainly: out[K], d[D], E
static void plain(const std::vector<double> &x, int F, int copy, const Tables &t, int p, int K, double cf, double floor,
                  std::vector<double> &out, std::vector<double> &d, double &E) {
  const int D = F + 2;
  std::vector<double> h(F), r(p + 1), a(p, 0.0), tt(p, 0.0), q(p, 0.0);
  for (int f = 0; f < F; ++f) {
    const double e = x[copy + f];
    const double g = (e < floor) ? floor : e;
    const double prod = g * t.w[f];
    h[f] = std::pow(prod, cf);
  }
  d.assign(D, 0.0);
  d[0] = h[0];
  for (int f = 0; f < F; ++f) d[1 + f] = h[f];
  d[D - 1] = h[F - 1];
  for (int i = 0; i <= p; ++i) {
    double acc = 0.0;
    for (int j = 0; j < D; ++j) {
      const double prod = t.B[(size_t)i * D + j] * d[j];
      acc = acc + prod;
    }
    r[i] = acc;
  }
  E = r[0];
  for (int i = 0; i < p; ++i) {
    double k = r[i + 1];
    for (int j = 0; j < i; ++j) {
      const double prod = a[j] * r[i - j];
      k = k + prod;
    }
    k = k / E;
    const double kk = k * k;
    double c = 1.0 - kk;
    c = (c < 1e-5) ? 1e-5 : c;
    E = E * c;
    tt[i] = -k;
    for (int j = 0; j < i; ++j) {
      const double prod = k * a[i - j - 1];
      tt[j] = a[j] - prod;
    }
    for (int j = 0; j <= i; ++j) a[j] = tt[j];
  }
  for (int i = 0; i < p; ++i) {
    double s = 0.0;
    for (int j = 0; j < i; ++j) {
      const double scaled = (double)(i - j) * a[j];
      const double prod = scaled * q[i - j - 1];
      s = s + prod;
    }
    const double mean = s / (double)(i + 1);
    q[i] = -a[i] - mean;
  }
  out.assign(K, 0.0);
  if (copy) {
    const double e0 = x[0];
    out[0] = std::log((e0 < floor) ? floor : e0);
  } else {
    out[0] = t.L[0] * std::log(E);
  }
  for (int k = 1; k < K; ++k) out[k] = t.L[k] * q[k - 1];
}

// plp_row of one row in lane `lane` of storage `lanes` wide; every array exactly as long as the rule may touch
static void ruled(const std::vector<double> &x, int F, int copy, const Tables &t, int p, int K, double cf, double floor,
                  int lanes, int lane, bool want_aux, std::vector<double> &out, std::vector<double> &aux) {
  const int D = F + 2;
  const double guard = -12345.5;
  std::vector<double> work((size_t)plp_work_words(p) * lanes, guard);
  out.assign(K, guard);
  aux.assign(want_aux ? D + 1 : 0, guard);
  std::vector<int> stored(K, 0), auxed(D + 1, 0);
  int loads = 0;
  plp_row(
      [&](int c) {
        CHECK(c >= 0 && c < copy + F);
        ++loads;
        return x[c];
      },
      F, copy, t.w.data(), t.B.data(), t.L.data(), p, K, cf, floor, work.data() + lane, (int64_t)lanes,
      [](double b, double e) { return std::pow(b, e); }, [](double v) { return std::log(v); },
      [&](int k, double v) {
        CHECK(k >= 0 && k < K);
        ++stored[k];
        out[k] = v;
      },
      want_aux,
      [&](int j, double v) {
        CHECK(want_aux && j >= 0 && j <= D);
        ++auxed[j];
        aux[j] = v;
      });
  CHECK(loads == F + copy);  // every energy is loaded (and raised) once
  for (int k = 0; k < K; ++k) CHECK(stored[k] == 1);
  for (int j = 0; j <= D; ++j) CHECK(auxed[j] == (want_aux ? 1 : 0));
  for (size_t i = 0; i < work.size(); ++i)
    if ((int)(i % lanes) != lane) CHECK(same(work[i], guard));  // the other lanes' words
}

static std::vector<double> random_row(int W, double level) {
  std::vector<double> x(W);
  for (int c = 0; c < W; ++c) {
    // exp of a sum of uniforms: a wide spread of magnitudes, and now and then an exact zero
    const double n = (next_unit() + next_unit() + next_unit() + next_unit() - 2.0) * 3.5;
    x[c] = (next_u64() % 17 == 0) ? 0.0 : (double)(float)(level * std::exp(n));
  }
  return x;
}

static void sweep_rows() {
  long rows = 0;
  const int Fs[] = {1, 2, 23, 40, 254};
  const double floor = std::ldexp(1.0, -126);
  for (int F : Fs) {
    const int pmax = F + 1 < 32 ? F + 1 : 32;
    const int ps[] = {1, 2, 12, pmax};
    for (int p : ps) {
      if (p > pmax) continue;
      const int Ks[] = {1, p + 1};
      for (int K : Ks) {
        for (int copy = 0; copy <= 1; ++copy) {
          if (F + copy > PLP_MAX_WIDTH) continue;
          CHECK(plp_shape_ok(F, copy, p, K));
          for (int variant = 0; variant < 4; ++variant) {
            const bool loud = variant != 1;
            const double cf = variant == 2 ? 0.5 : 1.0 / 3.0;
            const Tables t = tables(F, p, K, variant == 3 ? 0.0 : 22.0, variant == 2 ? 0.1 : 1.0, loud);
            const double levels[] = {1e-8, 1.0, 1e6};
            for (double level : levels) {
              const std::vector<double> x = random_row(F + copy, level);
              std::vector<double> want, d, out, aux;
              double E;
              plain(x, F, copy, t, p, K, cf, floor, want, d, E);
              const int lanes = variant & 1 ? PLP_THREADS : 1;
              const int lane = lanes == 1 ? 0 : (int)(next_u64() % lanes);
              for (int want_aux = 0; want_aux <= 1; ++want_aux) {
                ruled(x, F, copy, t, p, K, cf, floor, lanes, lane, want_aux != 0, out, aux);
                for (int k = 0; k < K; ++k) CHECK(same(out[k], want[k]) && std::isfinite(out[k]));
                if (want_aux) {
                  for (int j = 0; j < F + 2; ++j) CHECK(same(aux[j], d[j]));
                  CHECK(same(aux[F + 2], E));
                }
              }
              ++rows;
            }
          }
        }
      }
    }
  }
  std::printf("%ld rows against the definition written out\n", rows);
}

static void known_answers() {
  // r[i] = alpha^i: an AR(1) spectrum.  Durbin finds a = (-alpha, 0, ...) and E = 1 - alpha^2 exactly, and the
  // cepstrum of 1 / (1 - alpha z^-1) is alpha^n / n
  const int p = 12;
  const double alpha = 0.5;
  for (int lanes : {1, PLP_THREADS}) {
    std::vector<double> work((size_t)plp_work_words(p) * lanes, 7.0);
    double *mine = work.data() + (lanes - 1);
    for (int i = 0; i <= p; ++i) mine[(size_t)i * lanes] = std::pow(alpha, i);
    const double E = plp_recursions(mine, lanes, p);
    CHECK(E == 0.75);
    CHECK(mine[(size_t)(p + 1) * lanes] == -alpha);
    for (int j = 1; j < p; ++j) CHECK(mine[(size_t)(p + 1 + j) * lanes] == 0.0);
    for (int n = 1; n <= p; ++n) CHECK(mine[(size_t)(n - 1) * lanes] == std::pow(alpha, n) / n);
    CHECK(mine[0] == 0.5 && mine[lanes] == 0.125 && mine[2 * lanes] == 1.0 / 24 && mine[3 * lanes] == 1.0 / 64);
  }
  // r = (1, 1, ...): k = 1 in the first step, 1 - k^2 = 0 is clamped to 1e-5; every later k is 0
  {
    std::vector<double> work(plp_work_words(p), 1.0);
    const double E = plp_recursions(work.data(), 1, p);
    CHECK(E == 1e-5);
    CHECK(work[p + 1] == -1.0);
    for (int j = 1; j < p; ++j) CHECK(work[p + 1 + j] == 0.0);
    for (int n = 1; n <= p; ++n) CHECK(work[n - 1] == 1.0 / n);
  }
  // a NaN anywhere in r is a NaN in E and in every q: the clamp lets it pass
  {
    std::vector<double> work(plp_work_words(p), 0.0);
    for (int i = 0; i <= p; ++i) work[i] = std::pow(0.3, i);
    work[0] = std::numeric_limits<double>::quiet_NaN();
    const double E = plp_recursions(work.data(), 1, p);
    CHECK(std::isnan(E));
    for (int n = 0; n < p; ++n) CHECK(std::isnan(work[n]));
  }
  const double floor = std::ldexp(1.0, -126);
  const int Fs[] = {1, 2, 23, 40, 254};
  for (int F : Fs) {
    const int p2 = F + 1 < 12 ? F + 1 : 12, K = p2 + 1;
    const Tables t = tables(F, p2, K, 22.0, 1.0, true);
    std::vector<double> x(F), out, aux;
    // a flat spectrum after the weighting: r = (1, ~0, ...), log E ~ 0, every cepstrum ~ 0
    for (int f = 0; f < F; ++f) x[f] = 1.0 / t.w[f];
    ruled(x, F, 0, t, p2, K, 1.0 / 3.0, floor, 1, 0, false, out, aux);
    for (int k = 0; k < K; ++k) CHECK(std::fabs(out[k]) < 1e-12);
    // a row of zeros is finite, because of the floor
    std::fill(x.begin(), x.end(), 0.0);
    ruled(x, F, 0, t, p2, K, 1.0 / 3.0, floor, 1, 0, true, out, aux);
    for (int k = 0; k < K; ++k) CHECK(std::isfinite(out[k]));
    for (double v : aux) CHECK(std::isfinite(v) && v > 0.0);
    // a NaN in the row is a NaN in every computed column
    for (int at : {0, F / 2, F - 1}) {
      for (int f = 0; f < F; ++f) x[f] = 1.0 + f;
      x[at] = std::numeric_limits<double>::quiet_NaN();
      ruled(x, F, 0, t, p2, K, 1.0 / 3.0, floor, 1, 0, false, out, aux);
      for (int k = 0; k < K; ++k) CHECK(std::isnan(out[k]));
    }
  }
  // with the energy column: column 0 is the floored log energy, whatever the lifter and the scale
  {
    const int F = 23;
    const Tables t = tables(F, 12, 13, 22.0, 0.1, true);
    std::vector<double> x = random_row(F + 1, 1.0), out, aux;
    x[0] = 7.5;
    ruled(x, F, 1, t, 12, 13, 1.0 / 3.0, floor, 1, 0, false, out, aux);
    CHECK(same(out[0], std::log(7.5)));
    x[0] = 0.0;
    ruled(x, F, 1, t, 12, 13, 1.0 / 3.0, floor, 1, 0, false, out, aux);
    CHECK(same(out[0], std::log(floor)));
  }
  std::printf("known answers\n");
}

static void sweep_mapping() {
  CHECK(PLP_THREADS == 64);
  for (int64_t rows = 0; rows <= 400; ++rows) {
    const int64_t blocks = plp_block_count(rows);
    CHECK(blocks == (rows + PLP_THREADS - 1) / PLP_THREADS);
    // every row has one lane, in order, adjacent lanes on adjacent rows
    int64_t next = 0;
    for (int64_t b = 0; b < blocks; ++b)
      for (int t = 0; t < PLP_THREADS; ++t) {
        const int64_t row = plp_lane_row(b, t);
        if (row < rows) CHECK(row == next++);
      }
    CHECK(next == rows);
  }
  const int64_t most = PLP_MAX_BLOCKS * PLP_THREADS;
  CHECK(PLP_MAX_BLOCKS == 2147483647);
  CHECK(plp_block_count(most) == PLP_MAX_BLOCKS);
  CHECK(plp_block_count(most - 1) == PLP_MAX_BLOCKS);
  CHECK(plp_block_count(most - PLP_THREADS) == PLP_MAX_BLOCKS - 1);
  CHECK(plp_block_count(most + 1) == -1);
  CHECK(plp_block_count(INT64_MAX) == -1);
  CHECK(plp_block_count(-1) == -1);
  CHECK(plp_lane_row(PLP_MAX_BLOCKS - 1, PLP_THREADS - 1) == most - 1);  // (64 bits: no wrap at 2^31 or 2^32 rows)
  CHECK(plp_lane_row((int64_t)1 << 26, 0) == (int64_t)1 << 32);
  for (int p = 1; p <= PLP_MAX_ORDER; ++p) {
    CHECK(plp_work_words(p) == 2 * p + 1);
    CHECK(plp_block_lds_bytes(p) == (2 * p + 1) * 64 * 8 && plp_block_lds_bytes(p) <= 65536);
  }
  // the shapes the definition serves
  CHECK(plp_shape_ok(1, 0, 1, 1) && plp_shape_ok(1, 0, 2, 3) && !plp_shape_ok(1, 0, 3, 1));
  CHECK(plp_shape_ok(256, 0, 32, 33) && plp_shape_ok(255, 1, 32, 33) && !plp_shape_ok(256, 1, 32, 33));
  CHECK(!plp_shape_ok(257, 0, 12, 13) && !plp_shape_ok(0, 0, 1, 1) && !plp_shape_ok(0, 1, 1, 1));
  CHECK(!plp_shape_ok(40, 0, 33, 13) && !plp_shape_ok(40, 0, 0, 1) && !plp_shape_ok(40, 2, 12, 13));
  CHECK(!plp_shape_ok(40, 0, 12, 14) && !plp_shape_ok(40, 0, 12, 0) && plp_shape_ok(40, 0, 12, 13));
  CHECK(plp_shape_ok(23, 1, 24, 25) && !plp_shape_ok(23, 1, 25, 13));
  std::printf("lane and block mapping\n");
}

int main() {
  sweep_mapping();
  known_answers();
  sweep_rows();
  std::printf("%ld checks of the PLP rule passed\n", g_checks);
  return 0;
}
