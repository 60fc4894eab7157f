// Sweep of csrc/reverb_rule.h on the CPU (tests/test_reverb_rule.py builds and runs it, plain and under sanitizers):
// the block, partition, pair and output-range arithmetic against the definition written out plainly; every output
// sample written exactly once; no input index outside the utterance; the partitioned sum, evaluated with the rule's
// index arithmetic on integers, equal to the direct convolution; the plan's draws; the refusal above 2^31 - 1 blocks.
// The arrays are exactly as long as the rule may touch, so that a sanitizer sees any step outside them.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pydrobert-speech_amd/csrc/reverb_rule.h"

using namespace pds;

static int g_checks = 0;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    ++g_checks;                                                                      \
    if (!(cond)) {                                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                  \
      std::exit(1);                                                                  \
    }                                                                                \
  } while (0)

static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// one utterance of n samples against L taps with peak d: the whole form on integers
static void sweep(int64_t n, int64_t L, int64_t d) {
  const int64_t P = reverb_partitions(L);
  CHECK(P == ceil_div(L, 512));
  std::vector<int64_t> x((size_t)n), h((size_t)L);  // exactly as long as the rule may touch
  for (int64_t i = 0; i < n; ++i) x[(size_t)i] = (i * 7 + 3) % 11 - 5;
  for (int64_t k = 0; k < L; ++k) h[(size_t)k] = (k * 5 + 1) % 7 - 3;
  if (n == 0) {
    CHECK(reverb_pairs(n, d) == 0 && reverb_spectra(n) == 0);
    CHECK(reverb_spectra_units(n, true) == 0 && reverb_convolve_units(n, d, true) == 0);
    CHECK(reverb_convolve_units(n, d, false) == 0);
    return;
  }
  // blocks and pairs against the definition: tau runs over [d, d + n)
  CHECK(reverb_first_block(d) == d / 512 && reverb_last_block(n, d) == (d + n - 1) / 512);
  const int64_t m_lo = reverb_first_pair(d), pairs = reverb_pairs(n, d);
  CHECK(2 * m_lo <= reverb_first_block(d) && reverb_first_block(d) <= 2 * m_lo + 1);
  CHECK(2 * (m_lo + pairs - 1) <= reverb_last_block(n, d) && reverb_last_block(n, d) <= 2 * (m_lo + pairs - 1) + 1);
  // spectra: the last one whose stretch still meets the utterance, the first that is all zero behind it
  const int64_t last = reverb_last_spectrum(n);
  CHECK(reverb_stretch_re(last, 0) <= n - 1 && reverb_stretch_re(last + 1, 0) > n - 1);
  CHECK(reverb_spectra(n) == last + 2);
  CHECK(reverb_spectra_units(n, true) % 2 == 0 && reverb_spectra_units(n, true) >= reverb_spectra(n));
  CHECK(reverb_spectra_units(n, true) <= reverb_spectra(n) + 1 && reverb_spectra_units(n, false) == 0);
  CHECK(reverb_convolve_units(n, d, true) % 2 == 0 && reverb_convolve_units(n, d, true) >= pairs);
  CHECK(reverb_convolve_units(n, d, false) % 2 == 0 && reverb_convolve_units(n, d, false) * 1024 >= n);
  // the stretches: element s of spectrum k, zero fill outside the utterance, never an index outside it
  std::vector<std::vector<int64_t>> zr((size_t)(last + 2)), zi((size_t)(last + 2));
  for (int64_t k = -1; k <= last; ++k) {
    auto &r = zr[(size_t)(k + 1)], &im = zi[(size_t)(k + 1)];
    r.assign(1024, 0);
    im.assign(1024, 0);
    bool any = false;
    for (int64_t s = 0; s < 1024; ++s) {
      const int64_t ir = reverb_stretch_re(k, s), ii = reverb_stretch_im(k, s);
      CHECK(ir == 512 * (k - 1) + s && ii == 512 * k + s);
      if (reverb_inside(ir, n)) { r[(size_t)s] = x[(size_t)ir]; any = true; }
      if (reverb_inside(ii, n)) { im[(size_t)s] = x[(size_t)ii]; any = true; }
    }
    CHECK(any);  // (every stored spectrum meets the utterance)
  }
  // every pair: the circular convolution of the stored stretches with the partitions, elements 512 .. 1023
  std::vector<int> written((size_t)n, 0);
  std::vector<int64_t> wet((size_t)n, 0);
  for (int64_t m = m_lo; m < m_lo + pairs; ++m) {
    const int64_t k = 2 * m;
    const int64_t p_lo = reverb_first_part(k, n), p_hi = reverb_last_part(k, P);
    for (int64_t p = 0; p < P; ++p) {  // the skipped partitions are those whose spectrum is not stored
      const bool stored = k - p >= -1 && k - p <= last;
      CHECK(stored == (p >= p_lo && p <= p_hi));
    }
    for (int half = 0; half < 2; ++half) {
      int64_t begin, end;
      reverb_block_out(k + half, n, d, begin, end);
      CHECK(begin >= 0 && end <= n && begin <= end);
      for (int64_t t = begin; t < end; ++t) {
        const int64_t e = t + d - 512 * (k + half);  // element 512 + e of the transform
        CHECK(e >= 0 && e < 512);
        int64_t sum = 0;
        for (int64_t p = p_lo; p <= p_hi; ++p) {
          const auto &src = half ? zi[(size_t)(k - p + 1)] : zr[(size_t)(k - p + 1)];
          for (int64_t j = 0; j < 512 && 512 * p + j < L; ++j) sum += h[(size_t)(512 * p + j)] * src[(size_t)(512 + e - j)];
        }
        wet[(size_t)t] = sum;
        ++written[(size_t)t];
      }
    }
  }
  for (int64_t t = 0; t < n; ++t) {
    CHECK(written[(size_t)t] == 1);  // every output sample exactly once
    int64_t want = 0;  // y_full[t + d] written out plainly
    for (int64_t k = 0; k < L; ++k) {
      const int64_t i = t + d - k;
      if (i >= 0 && i < n) want += h[(size_t)k] * x[(size_t)i];
    }
    CHECK(wet[(size_t)t] == want);
  }
  // blocks outside the needed range write nothing
  int64_t begin, end;
  reverb_block_out(reverb_first_block(d) - 1, n, d, begin, end);
  CHECK(begin == end);
  reverb_block_out(reverb_last_block(n, d) + 1, n, d, begin, end);
  CHECK(begin == end);
}

int main() {
  const int64_t ns[] = {0, 1, 2, 511, 512, 513, 1023, 1024, 1025, 2049};
  const int64_t Ls[] = {1, 2, 511, 512, 513, 1024, 1025, 1537};
  for (int64_t n : ns)
    for (int64_t L : Ls) {
      if (L <= 2) {
        for (int64_t d = 0; d < L; ++d) sweep(n, L, d);
      } else {
        const int64_t ds[] = {0, 1, 511, 512, L - 1};
        for (int64_t d : ds)
          if (d < L) sweep(n, L, d);
      }
    }
  for (int64_t L = 1; L <= 9; ++L)
    for (int64_t d = 0; d < L; ++d) sweep(5, L, d);
  std::printf("blocks, partitions, output ranges: %d checks\n", g_checks);

  // the plan's draws: Philox4x32-10's known answer (Random123: zero counter and key), the pick and the comparison
  {
    uint32_t c[4] = {0, 0, 0, 0};
    reverb_philox(c, 0, 0);
    CHECK(c[0] == 0x6627e8d5u && c[1] == 0xe169c58du && c[2] == 0xbc57ac4cu && c[3] == 0x9b00dbd8u);
    CHECK(REVERB_COUNTER_3 == 0x52495231u && REVERB_COUNTER_3 != 0x4D495831u && REVERB_COUNTER_3 != 0u);
    for (int64_t K : {(int64_t)1, (int64_t)2, (int64_t)64, (int64_t)1000003}) {
      CHECK(reverb_pick(0xffffffffu, K) == K - 1 && reverb_pick(0u, K) == 0);
    }
    CHECK(!reverb_applied(0u, 0.0) && !reverb_applied(0xffffffffu, 0.0));
    CHECK(reverb_applied(0u, 1.0) && reverb_applied(0xffffffffu, 1.0));
    CHECK(reverb_applied(0x7fffffffu, 0.5) && !reverb_applied(0x80000000u, 0.5));
    uint32_t x[4], y[4];
    reverb_draw(0x0123456789abcdefull, x);
    reverb_draw(0x0123456789abcdefull, y);
    CHECK(x[0] == y[0] && x[3] == y[3]);
    reverb_draw(0x0123456789abcdeeull, y);
    CHECK(x[0] != y[0] || x[1] != y[1] || x[2] != y[2] || x[3] != y[3]);
  }
  std::printf("plan draws: Philox, pick and probability\n");

  // the counts of a launch and the refusal above 2^31 - 1 blocks
  {
    CHECK(reverb_blocks(0) == 0 && reverb_blocks(1) == 1 && reverb_blocks(8) == 1 && reverb_blocks(9) == 2);
    CHECK(reverb_blocks(-1) == -1);
    const int64_t most = REVERB_MAX_BLOCKS * REVERB_HALVES;
    CHECK(reverb_blocks(most) == REVERB_MAX_BLOCKS && reverb_blocks(most + 1) == -1);
    CHECK(reverb_workspace_bytes(3) == 3 * 8192 && reverb_workspace_bytes(most + 1) == -1);
    CHECK(reverb_workspace_bytes(most) == most * 8192);  // (64-bit: no wrap)
    CHECK(reverb_scale_blocks_x(0) == 0 && reverb_scale_blocks_x(1) == 1 && reverb_scale_blocks_x(4093) == 1);
    CHECK(reverb_scale_blocks_x(4094) == 2);
    CHECK(reverb_scale_blocks(4096, 65535) == 2 * 65535 && reverb_scale_blocks(4096, 65536) == -1);
    CHECK(reverb_scale_blocks((int64_t)1 << 40, 65535) == -1 && reverb_scale_blocks(-1, 1) == -1);
    const int64_t base[] = {0, 0, 4, 4, 6};
    CHECK(reverb_find(base, 5, 0) == 1 && reverb_find(base, 5, 3) == 1 && reverb_find(base, 5, 4) == 3);
    CHECK(reverb_find(base, 5, 5) == 3 && reverb_find(base, 5, 6) == 4 && reverb_find(base, 1, 9) == 0);
  }
  std::printf("launch counts: the refusal above 2^31 - 1 blocks\n");
  std::printf("%d checks of the reverb rule passed\n", g_checks);
  return 0;
}
