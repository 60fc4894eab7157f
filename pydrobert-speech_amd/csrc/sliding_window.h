// The window of sliding-window CMVN (include/pds_amd_stages.h, post.SlidingCMVN): host and device, no dependencies.
// Shared by the kernels of sliding.hip and by tests/csrc/test_sliding_window.cpp, which sweeps it on the CPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PDS_SW_HD __host__ __device__ __forceinline__
#else
#define PDS_SW_HD inline
#endif

namespace pds {

// Frames [ws, we) whose statistics normalise frame t of an utterance of T frames (0 <= t < T): Kaldi's rule
// (apply-cmvn-sliding), W = cmn_window >= 1, min_window >= 1.  The causal window holds W + 1 frames once it is full.
//   0 <= ws <= t < we <= T;  from t to t + 1, ws and we each move by 0 or 1;  we - ws <= max(W + 1, min_window)
PDS_SW_HD void sliding_window(int64_t t, int64_t T, int64_t W, int64_t min_window, bool center, int64_t &ws,
                              int64_t &we) {
  if (center) {
    ws = t - W / 2;
    we = ws + W;
  } else {
    ws = t - W;
    we = t + 1;
  }
  if (ws < 0) {
    we -= ws;
    ws = 0;
  }
  if (!center && we > t) we = t + 1 > min_window ? t + 1 : min_window;
  if (we > T) {
    ws -= we - T;
    we = T;
    if (ws < 0) ws = 0;
  }
}

// Segments of `refresh` frames an utterance of T frames falls into (the sums are rebuilt at every segment's first
// frame, so segments are independent)
PDS_SW_HD int64_t sliding_segments(int64_t T, int64_t refresh) { return T <= 0 ? 0 : (T + refresh - 1) / refresh; }

// Slot of the streaming ring (W + 1 rows) that holds frame t: the slot frame t overwrites held frame t - W - 1, the
// frame that leaves the causal window [max(0, t - W), t + 1) at t
PDS_SW_HD int64_t sliding_ring_slot(int64_t t, int64_t W) { return t % (W + 1); }

}  // namespace pds
