// CPU sweep of csrc/sliding_window.h, the window arithmetic the kernels of sliding.hip share: the window's properties,
// the rows the offline kernel's segment walk reads (through a bounds-checked vector), and the ring walk of the
// streaming kernel against the offline walk on integer data (exact in double, so the sums must be equal).
// Built plain and with -fsanitize=address,undefined by tests/test_sliding_window.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pydrobert-speech_amd/csrc/sliding_window.h"

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

// the offline kernel's walk over one (utterance, segment): sums per frame
static void offline_walk(const std::vector<double> &x, int64_t W, int64_t min_window, bool center, int64_t refresh,
                         std::vector<double> &s1, std::vector<int64_t> &count) {
  const int64_t T = (int64_t)x.size();
  s1.assign(T, 0.0);
  count.assign(T, 0);
  for (int64_t seg = 0; seg < pds::sliding_segments(T, refresh); ++seg) {
    const int64_t t0 = seg * refresh, t1 = std::min(t0 + refresh, T);
    int64_t ws, we;
    pds::sliding_window(t0, T, W, min_window, center, ws, we);
    double s = 0.0;
    for (int64_t u = ws; u < we; ++u) s += x.at(u);
    // as the kernel: AHEAD frames at a time, every load without a condition (so each index must be a row of the
    // utterance whether its value is used or not: .at() checks it), a frame past the segment's end repeating the last
    const int AHEAD = 4;
    for (int64_t t = t0; t < t1; t += AHEAD) {
      double xv[AHEAD], ov[AHEAD], nv[AHEAD];
      int64_t cnt[AHEAD];
      bool left[AHEAD], entered[AHEAD];
      for (int u = 0; u < AHEAD; ++u) {
        const int64_t tt = t + u < t1 ? t + u : t1 - 1;
        int64_t nws, nwe;
        pds::sliding_window(tt, T, W, min_window, center, nws, nwe);
        left[u] = nws != ws;
        entered[u] = nwe != we;
        xv[u] = x.at(tt);
        ov[u] = x.at(ws);
        nv[u] = x.at(nwe - 1);
        cnt[u] = nwe - nws;
        ws = nws;
        we = nwe;
      }
      for (int u = 0; u < AHEAD; ++u) {
        if (t + u >= t1) continue;
        if (left[u]) s -= ov[u];
        if (entered[u]) s += nv[u];
        (void)xv[u];
        s1.at(t + u) = s;
        count.at(t + u) = cnt[u];
      }
    }
  }
}

int main() {
  long windows = 0, walks = 0;
  for (int64_t W = 1; W <= 8; ++W)
    for (int64_t mw = 1; mw <= 11; ++mw)
      for (int center = 0; center < 2; ++center)
        for (int64_t T = 1; T <= 29; ++T) {
          int64_t pws = 0, pwe = 0;
          for (int64_t t = 0; t < T; ++t) {
            int64_t ws, we;
            pds::sliding_window(t, T, W, mw, center != 0, ws, we);
            CHECK(0 <= ws && ws <= t && t < we && we <= T, "W %ld mw %ld c %d T %ld t %ld: [%ld, %ld)", (long)W,
                  (long)mw, center, (long)T, (long)t, (long)ws, (long)we);
            CHECK(we - ws <= std::max(W + 1, mw), "W %ld mw %ld c %d T %ld t %ld", (long)W, (long)mw, center, (long)T,
                  (long)t);
            if (t) {
              CHECK((ws == pws || ws == pws + 1) && (we == pwe || we == pwe + 1), "W %ld mw %ld c %d T %ld t %ld",
                    (long)W, (long)mw, center, (long)T, (long)t);
            }
            if (!center && mw == 1) CHECK(ws == std::max<int64_t>(0, t - W) && we == t + 1, "causal window");
            pws = ws;
            pwe = we;
            ++windows;
          }
        }
  CHECK(pds::sliding_segments(0, 3) == 0 && pds::sliding_segments(1, 3) == 1 && pds::sliding_segments(3, 3) == 1 &&
            pds::sliding_segments(4, 3) == 2,
        "segments");
  // the offline walk against direct sums, and the streaming ring walk against the offline walk
  uint64_t rnd = 12345;
  auto next = [&]() {
    rnd = rnd * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rnd >> 33);
  };
  for (int64_t W = 1; W <= 7; ++W)
    for (int64_t refresh : {1, 2, 3, 5, 8, 1000})
      for (int64_t T : {0, 1, 2, 5, 9, 17, 40}) {
        std::vector<double> x(T);
        for (auto &v : x) v = (double)(next() % 2001) - 1000.0;
        for (int64_t mw : {1, 3, 9})
          for (int center = 0; center < 2; ++center) {
            std::vector<double> s1;
            std::vector<int64_t> cnt;
            offline_walk(x, W, mw, center != 0, refresh, s1, cnt);
            for (int64_t t = 0; t < T; ++t) {
              int64_t ws, we;
              pds::sliding_window(t, T, W, mw, center != 0, ws, we);
              double direct = 0.0;
              for (int64_t u = ws; u < we; ++u) direct += x.at(u);
              CHECK(s1.at(t) == direct && cnt.at(t) == we - ws, "offline walk W %ld mw %ld c %d r %ld T %ld t %ld",
                    (long)W, (long)mw, center, (long)refresh, (long)T, (long)t);
            }
            ++walks;
          }
        // streaming: ticks of 0 .. 4 rows, a ring of W + 1 slots
        std::vector<double> want;
        std::vector<int64_t> cnt;
        offline_walk(x, W, 1, false, refresh, want, cnt);
        std::vector<double> ring(W + 1, 1e300);  // (a slot read before it is written would show)
        double s = 0.0;
        int64_t t = 0;
        while (t < T) {
          const int64_t k = std::min<int64_t>(T - t, next() % 5);
          int64_t slot = pds::sliding_ring_slot(t, W), phase = t % refresh;
          for (int64_t r = 0; r < k; ++r, ++t) {
            const double d = x.at(t);
            const int64_t n = std::min(t, W) + 1;
            if (phase == 0) {
              int64_t q0 = slot - (n - 1);
              if (q0 < 0) q0 += W + 1;
              s = 0.0;
              for (int64_t j = 0; j < n - 1; ++j) s += ring.at(q0 + j < W + 1 ? q0 + j : q0 + j - (W + 1));
              s += d;
            } else {
              if (t > W) s -= ring.at(slot);
              s += d;
            }
            ring.at(slot) = d;
            CHECK(s == want.at(t) && n == cnt.at(t), "ring walk W %ld r %ld T %ld t %ld", (long)W, (long)refresh,
                  (long)T, (long)t);
            if (++slot == W + 1) slot = 0;
            if (++phase == refresh) phase = 0;
          }
        }
        ++walks;
      }
  if (failures) {
    printf("%ld checks failed\n", failures);
    return 1;
  }
  printf("sliding windows checked: %ld windows, %ld walks\n", windows, walks);
  return 0;
}
