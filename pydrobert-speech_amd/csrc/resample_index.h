// The index arithmetic of windowed-sinc rate conversion (include/pds_amd_stages.h, pre.Resample): host and device, no
// dependencies.  Shared by the kernels of resample.hip and by tests/csrc/test_resample_index.cpp, which sweeps it on
// the CPU.  Output k of an utterance belongs to phase p = k mod out_unit of unit u = k div out_unit and reads the
// inputs first[p] + u * in_unit + j, j in [0, ntaps[p]).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PDS_RS_HD __host__ __device__ __forceinline__
#else
#define PDS_RS_HD inline
#endif

namespace pds {

// the largest weight table a call takes: out_unit * max_taps entries (8 MiB of float64), so that an index into it
// and a phase fit 32 bits with room to spare
constexpr int64_t RESAMPLE_MAX_TABLE = (int64_t)1 << 20;

// ceil(n * out_unit / in_unit) without forming n * out_unit (n up to 2^62; the units are below 2^31)
PDS_RS_HD int64_t resample_num_output_samples(int64_t n, int64_t in_unit, int64_t out_unit) {
  if (n <= 0) return 0;
  const int64_t q = n / in_unit, r = n - q * in_unit;
  return q * out_unit + (r * out_unit + in_unit - 1) / in_unit;
}

// k = u * out_unit + p with 0 <= p < out_unit, for k >= 0: in 32 bits where k fits them (the division every lane does)
PDS_RS_HD void resample_split(int64_t k, int32_t out_unit, int64_t &u, int32_t &p) {
  if (k <= (int64_t)0xffffffffu) {
    const uint32_t k32 = (uint32_t)k, q = k32 / (uint32_t)out_unit;
    u = (int64_t)q;
    p = (int32_t)(k32 - q * (uint32_t)out_unit);
  } else {
    u = k / out_unit;
    p = (int32_t)(k - u * out_unit);
  }
}

// the first input index of an output of unit u whose phase starts at first_p: a 64-bit product (u * in_unit passes
// 2^31 after a few hours of audio)
PDS_RS_HD int64_t resample_base(int64_t u, int32_t in_unit, int32_t first_p) {
  return u * (int64_t)in_unit + (int64_t)first_p;
}

// Outputs due once a stream has been given n samples: the k whose last input index, last[p] + u * in_unit, is at most
// n - 1.  `last` holds out_unit values, non-decreasing, with last[out_unit - 1] <= last[0] + in_unit (the last index is
// then non-decreasing in k, and the due outputs are the first so many).  Never more than
// resample_num_output_samples(n, ...) where last[p] >= floor(p * in_unit / out_unit), as the definition gives.
PDS_RS_HD int64_t resample_due(int64_t n, int64_t in_unit, int64_t out_unit, const int32_t *last) {
  if (n <= 0) return 0;
  const int64_t q = n - 1;
  // u0: the last unit all of whose phases are due (floor division; -1: none)
  const int64_t d = q - (int64_t)last[out_unit - 1];
  const int64_t u0 = d >= 0 ? d / in_unit : -((-d + in_unit - 1) / in_unit);
  if (u0 < -1) return 0;
  // ... and the phases of unit u0 + 1 with last[p] <= rest: a binary search over the non-decreasing table
  const int64_t rest = q - (u0 + 1) * in_unit;
  int64_t lo = 0, hi = out_unit;
  while (lo < hi) {
    const int64_t mid = (lo + hi) / 2;
    if ((int64_t)last[mid] <= rest) lo = mid + 1; else hi = mid;
  }
  return (u0 + 1) * out_unit + lo;
}

}  // namespace pds
