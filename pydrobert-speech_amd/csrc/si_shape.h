// Launch shapes of the short-integration kernels: every size the launchers of si.hip (direct form) and si_fft.hip
// (overlap-save form) derive from the plan and the batch -- which transform size serves a bank, how many shift-sized
// blocks a transform yields, how many window factors a lane keeps, how the filters are dealt to workgroups, the tile
// of the direct form -- in one place, so that the launchers, the scratch length and pds_si_launch_shape (through
// which the tests ask what a launch looked like) cannot disagree.
//
// FFT form: a transform of NT = 1024 or 2048 points yields `blocks` blocks of S filtered samples
// (blocks * S <= NT - (M - 1), at most kSiFftMaxBlocks); utterance b needs blocks 0 .. nframes[b], so the longest one
// needs transforms = ceil((max_frames + 1) / blocks); a workgroup of kSiFftWaves wavefronts takes per_wg of them
// (two 1024-point transforms per wavefront or one 2048-point one).  Few workgroups (one utterance, a streaming call)
// would leave most of the device idle: the C filters are then dealt to `groups` <= 8 workgroups per stretch
// (grid.z), c_per_group filters each, the last group possibly shorter.
//
// Direct form: a workgroup takes JB consecutive blocks of one utterance and writes JB - 1 frames (neighbouring
// workgroups overlap by one block); a tile longer than kSiThreads * kSiR samples takes several passes of the
// thread block.
//
// Host code only (plain C++): included by si.hip, si_fft.hip and tests/csrc/test_si_shape.cpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace pds {

// ---- FFT form (si_fft.hip) ----
constexpr int kSiFftN = 1024;           // points of the half-wave transform; the 2048-point form is radix 2 on top
constexpr int kSiFftL = 32;             // lanes = registers of a half-wave transform
constexpr int kSiFftRowStride = kSiFftL + 1;  // exchange row stride in float2
constexpr int kSiFftWaves = 8;          // wavefronts per workgroup
constexpr int kSiFftMaxBlocks = 8;      // shift-sized blocks a transform may yield (register budget)
constexpr int kSiFftMaxWindowRegs = 16;  // window factors a lane may keep per window half
constexpr int kSiFftMaxGroups = 8;      // workgroups the filters of one stretch are dealt to at most
constexpr int kSiCombineThreads = 256;  // threads per workgroup of the combine kernel

// blocks of S filtered samples one NT-point transform yields for supports of M taps (0: none)
inline int si_fft_blocks_for(int NT, int M, int S) {
  if (M > NT) return 0;
  const int blocks = std::min(kSiFftMaxBlocks, (NT - (M - 1)) / S);
  const int lanes = NT / kSiFftL;  // of one transform
  if (blocks < 1 || S > kSiFftMaxWindowRegs * lanes) return 0;
  // (the transposition area(s) of the transform -- 2.06 NT floats -- are reused for its NT squared
  // samples; the block sums read less than `lanes` floats past them, weighted by zero)
  return blocks;
}

struct SiFftForm {
  int blocks = 0;    // 0: supports too long for this form (direct kernel)
  bool big = false;  // 2048-point transforms
};

// 1024- or 2048-point transforms: whichever spends less of a transform on the overlap (the
// larger one pays ~20 % more per point for its extra radix-2 stage)
inline SiFftForm si_fft_form_for(int M, int S) {
  SiFftForm f;
  const int b1 = si_fft_blocks_for(kSiFftN, M, S), b2 = si_fft_blocks_for(2 * kSiFftN, M, S);
  if (b1 == 0 && b2 == 0) return f;
  const double eff1 = (double)b1 * S / kSiFftN, eff2 = (double)b2 * S / (2 * kSiFftN) / 1.2;
  f.big = eff2 > eff1;
  f.blocks = f.big ? b2 : b1;
  return f;
}

// transforms the longest utterance needs: frames 0 .. max_frames - 1 read blocks 0 .. max_frames
inline int64_t si_fft_transforms_for(int blocks, int64_t max_frames) { return (max_frames + 1 + blocks - 1) / blocks; }

struct SiFftShape {
  int NT = 0, lanes = 0;    // points and lanes of one transform
  int per_wg = 0;           // transforms per workgroup
  int nw = 0;               // window factors per lane and half: the smallest built count (3, 5, 8, 16) covering a block
  int want = 0;             // groups asked for (the filters may not split that many ways)
  int c_per_group = 0;      // filters a workgroup walks
  unsigned grid_x = 0, groups = 0;  // grid.x, grid.z (grid.y = B)
  unsigned combine_x = 0;   // grid.x of the combine kernel: a thread per (frame, filter) of the longest utterance
  int64_t transforms = 0;   // per utterance
  int64_t blocks_per_utt = 0;  // scratch rows (shift-sized blocks) reserved per utterance
  int64_t scratch_len = 0;  // floats: [B][blocks_per_utt][C][2]
  size_t smem = 0;          // dynamic LDS, bytes
};

inline SiFftShape si_fft_shape(bool big, int blocks, int S, int C, int32_t B, int64_t max_frames, int num_cus) {
  SiFftShape s;
  s.NT = big ? 2 * kSiFftN : kSiFftN;
  s.lanes = s.NT / kSiFftL;
  s.per_wg = big ? kSiFftWaves : 2 * kSiFftWaves;
  const int nw = (S + s.lanes - 1) / s.lanes;
  s.nw = nw <= 3 ? 3 : nw <= 5 ? 5 : nw <= 8 ? 8 : kSiFftMaxWindowRegs;
  s.transforms = si_fft_transforms_for(blocks, max_frames);
  s.blocks_per_utt = s.transforms * blocks;
  s.scratch_len = (int64_t)B * s.blocks_per_utt * C * 2;
  s.grid_x = (unsigned)((s.transforms + s.per_wg - 1) / s.per_wg);
  // few workgroups (one utterance, a streaming call): the filters are dealt to several workgroups per stretch, each
  // repeating the stretch's forward transform -- 1 / c_per_group more work for a pass of filters in parallel
  const int64_t wgs = (s.transforms + s.per_wg - 1) / s.per_wg * B;
  s.want = (int)std::min<int64_t>(kSiFftMaxGroups, std::max<int64_t>(1, 2 * (int64_t)num_cus / std::max<int64_t>(1, wgs)));
  s.c_per_group = (C + s.want - 1) / s.want;
  s.groups = (unsigned)((C + s.c_per_group - 1) / s.c_per_group);
  s.combine_x = (unsigned)((max_frames * C + kSiCombineThreads - 1) / kSiCombineThreads);
  s.smem = ((size_t)2 * kSiFftWaves * kSiFftL * kSiFftRowStride + (big ? 3 : 1) * (size_t)kSiFftL * kSiFftL) * 2 * sizeof(float);
  return s;
}

// ---- direct form (si.hip) ----
constexpr int kSiR = 9;          // consecutive samples per thread
constexpr int kSiThreads = 256;

// taps per filter padded to a multiple of the register block
inline int si_mpad(int M) { return (M + kSiR - 1) / kSiR * kSiR; }

struct SiDirectShape {
  int JB = 0;          // blocks per tile; a workgroup writes JB - 1 frames
  int tile = 0;        // JB * S samples
  int passes = 0;      // of the thread block over a tile
  unsigned grid_x = 0;  // (grid.y = B)
  size_t smem = 0;     // dynamic LDS, bytes: signal stretch, [2][tile] weighted samples, [2][JB] sums
};

inline SiDirectShape si_direct_shape(int S, int mpad, int64_t max_frames, size_t elem_size) {
  SiDirectShape s;
  int JB = (kSiThreads * kSiR) / S;
  if (JB < 2) JB = 2;  // long shifts: two blocks per tile, several passes of the thread block
  if ((int64_t)JB - 1 > max_frames) JB = (int)max_frames + 1;
  s.JB = JB;
  s.tile = JB * S;
  s.passes = (s.tile + kSiThreads * kSiR - 1) / (kSiThreads * kSiR);
  s.grid_x = (unsigned)((max_frames + JB - 2) / (JB - 1));
  s.smem = ((size_t)s.tile + mpad - 1 + kSiR + 2 * (size_t)s.tile + 2 * (size_t)JB) * elem_size;
  return s;
}

}  // namespace pds
