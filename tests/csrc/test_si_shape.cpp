// Sweep of the launch-shape arithmetic of the short-integration kernels (pydrobert-speech_amd/csrc/si_shape.h): every
// shape the launchers can be handed is checked against what the kernels rely on -- the filters' groups cover
// 0 .. C - 1 exactly with no empty group, a transform's blocks fit behind the overlap and in the register budget, the
// window factors cover a block, the transforms cover every block a frame reads, the grid covers the transforms; for
// the direct form the tiles cover every frame and the LDS size is the kernel's layout.  Built and run by
// tests/test_si_shape.py (CPU only).
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../pydrobert-speech_amd/csrc/si_shape.h"

static long failures = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (failures++ < 20) {                               \
        printf("FAILED %s: ", #cond);                      \
        printf(__VA_ARGS__);                               \
        printf("\n");                                      \
      }                                                    \
    }                                                      \
  } while (0)

static const int kB[] = {1, 2, 7, 64, 257, 513, 1024, 65535};
static const int64_t kFrames[] = {1, 2, 3, 41, 1000};
static const int kCus[] = {64, 256, 304};

int main() {
  long forms[3] = {0, 0, 0}, shapes = 0, splits[9] = {0}, ragged = 0, buckets[17] = {0};
  // which transform serves (M, S), and how many blocks it yields
  for (int S = 1; S <= 2400; ++S) {
    bool seen[2][9] = {{false}};
    for (int M = 1; M <= 2100; ++M) {
      const pds::SiFftForm f = pds::si_fft_form_for(M, S);
      const int b1 = pds::si_fft_blocks_for(1024, M, S), b2 = pds::si_fft_blocks_for(2048, M, S);
      for (int big = 0; big < 2; ++big) {
        const int NT = big ? 2048 : 1024, lanes = NT / 32, blocks = big ? b2 : b1;
        if (blocks == 0) continue;  // not offered
        CHECK(blocks >= 1 && blocks <= 8, "S %d M %d NT %d blocks %d", S, M, NT, blocks);
        CHECK(blocks * S <= NT - (M - 1), "S %d M %d NT %d blocks %d", S, M, NT, blocks);
        CHECK(S <= 16 * lanes, "S %d M %d NT %d", S, M, NT);
      }
      if (f.blocks == 0) {
        CHECK(b1 == 0 && b2 == 0, "S %d M %d: a form is offered and none chosen", S, M);
        ++forms[0];
        continue;
      }
      CHECK(f.blocks == (f.big ? b2 : b1), "S %d M %d blocks %d", S, M, f.blocks);
      ++forms[f.big ? 2 : 1];
      // the batch sweep: M acts on a launch through the form and its blocks alone
      if (seen[f.big][f.blocks]) continue;
      seen[f.big][f.blocks] = true;
      for (int B : kB)
        for (int64_t frames : kFrames) {
          // (C and the CU count act through want alone: the full sweep over them is below)
          const pds::SiFftShape s = pds::si_fft_shape(f.big, f.blocks, S, 41, B, frames, 256);
          const int NT = f.big ? 2048 : 1024, lanes = NT / 32;
          CHECK(s.NT == NT && s.lanes == lanes && s.per_wg == (f.big ? 8 : 16), "S %d M %d", S, M);
          CHECK(s.transforms * f.blocks >= frames + 1, "S %d M %d frames %ld transforms %ld", S, M, (long)frames, (long)s.transforms);
          CHECK((s.transforms - 1) * f.blocks < frames + 1, "S %d M %d frames %ld: an idle transform", S, M, (long)frames);
          CHECK((int64_t)s.grid_x * s.per_wg >= s.transforms && s.grid_x >= 1, "S %d M %d grid.x %u", S, M, s.grid_x);
          CHECK(((int64_t)s.grid_x - 1) * s.per_wg < s.transforms, "S %d M %d grid.x %u: an idle workgroup", S, M, s.grid_x);
          CHECK(s.nw == 3 || s.nw == 5 || s.nw == 8 || s.nw == 16, "S %d nw %d", S, s.nw);
          CHECK(s.nw >= (S + lanes - 1) / lanes, "S %d lanes %d nw %d", S, lanes, s.nw);
          CHECK(s.blocks_per_utt == s.transforms * f.blocks, "S %d M %d", S, M);
          CHECK(s.scratch_len == (int64_t)B * s.blocks_per_utt * 41 * 2, "S %d M %d B %d", S, M, B);
          // the kernel's LDS: 16 exchange areas of [32][33] float2, the [32][32] twiddles, [32][64] more for 2048 points
          CHECK(s.smem == (size_t)(16 * 32 * 33 + (f.big ? 3 : 1) * 1024) * 8 && s.smem <= 160 * 1024, "smem %zu", s.smem);
          // a lane's block sums read NW floats, `lanes` apart, from its sample of the block: the last block's stay inside
          // the transform's own exchange area(s) ([32][33] float2 per 1024 points)
          CHECK(NT - S + s.nw * lanes <= (NT / 1024) * 32 * 33 * 2, "S %d M %d nw %d", S, M, s.nw);
          CHECK((int64_t)s.combine_x * 256 >= frames * 41 && ((int64_t)s.combine_x - 1) * 256 < frames * 41, "frames %ld combine grid.x %u", (long)frames, s.combine_x);
          ++buckets[s.nw];
          ++shapes;
        }
    }
  }
  // how the filters are dealt to workgroups: want depends on the workgroups of a launch and the CU count alone
  for (int C = 1; C <= 130; ++C)
    for (int cus : kCus)
      for (int B : kB)
        for (int64_t frames : kFrames)
          for (int big = 0; big < 2; ++big)
            for (int blocks = 1; blocks <= 8; ++blocks) {
              const pds::SiFftShape s = pds::si_fft_shape(big, blocks, 160, C, B, frames, cus);
              const int64_t wgs = (int64_t)s.grid_x * B;
              CHECK(s.want >= 1 && s.want <= 8, "want %d", s.want);
              CHECK(s.want == 8 || (int64_t)(s.want + 1) * wgs > 2 * cus, "C %d B %d cus %d want %d: more groups fit", C, B, cus, s.want);
              CHECK(s.want == 1 || (int64_t)s.want * wgs <= 2 * cus, "C %d B %d cus %d want %d: too many groups", C, B, cus, s.want);
              CHECK(s.groups >= 1 && s.groups <= 8 && (int)s.groups <= s.want, "C %d want %d groups %u", C, s.want, s.groups);
              CHECK(s.c_per_group >= 1, "C %d want %d", C, s.want);
              CHECK((int64_t)(s.groups - 1) * s.c_per_group < C && C <= (int64_t)s.groups * s.c_per_group,
                    "C %d want %d c_per_group %d groups %u", C, s.want, s.c_per_group, s.groups);
              // no group is larger than an even deal needs
              CHECK((int64_t)(s.c_per_group - 1) * s.want < C, "C %d want %d c_per_group %d", C, s.want, s.c_per_group);
              ++splits[s.groups];
              ragged += C % s.c_per_group != 0;
              ++shapes;
            }
  // the direct form
  long passes[4] = {0, 0, 0, 0};
  for (int S = 1; S <= 2400; ++S)
    for (int M : {1, 8, 9, 10, 377, 754, 1037, 2100})
      for (int64_t frames : kFrames)
        for (size_t elem : {sizeof(float), sizeof(double)}) {
          const int mpad = pds::si_mpad(M);
          CHECK(mpad >= M && mpad < M + 9 && mpad % 9 == 0, "M %d mpad %d", M, mpad);
          const pds::SiDirectShape s = pds::si_direct_shape(S, mpad, frames, elem);
          CHECK(s.JB >= 2, "S %d frames %ld JB %d", S, (long)frames, s.JB);
          CHECK(s.JB <= frames + 1, "S %d frames %ld JB %d", S, (long)frames, s.JB);  // (frames >= 1: the floor of 2 fits)
          CHECK(s.JB == 2 || s.JB * S <= 256 * 9, "S %d JB %d: more than one pass without need", S, s.JB);
          CHECK(s.tile == s.JB * S, "S %d", S);
          CHECK((int64_t)s.grid_x * (s.JB - 1) >= frames && s.grid_x >= 1, "S %d frames %ld JB %d grid.x %u", S, (long)frames, s.JB, s.grid_x);
          CHECK(((int64_t)s.grid_x - 1) * (s.JB - 1) < frames, "S %d frames %ld JB %d grid.x %u: an idle workgroup", S, (long)frames, s.JB, s.grid_x);
          CHECK(s.passes >= 1 && (int64_t)s.passes * 256 * 9 >= s.tile && (int64_t)(s.passes - 1) * 256 * 9 < s.tile, "S %d JB %d passes %d", S, s.JB, s.passes);
          // si_conv_kernel's layout: seg[tile + mpad - 1 + R], zw[2][tile], red[2][JB]
          const size_t seglen = (size_t)s.tile + mpad - 1 + 9;
          CHECK(s.smem == (seglen + 2 * (size_t)s.tile + 2 * (size_t)s.JB) * elem, "S %d M %d smem %zu", S, M, s.smem);
          // the last thread of the last pass reads 17 samples from seg[base - kb - 8 ...], base <= mpad - 1 + tile - 1 + 8
          // rounded up to the thread's nine samples: inside seg
          const size_t last_first = (size_t)(s.tile - 1) / 9 * 9;
          CHECK(mpad - 1 + last_first + 8 < seglen, "S %d M %d JB %d: a thread reads past the stretch", S, M, s.JB);
          ++passes[s.passes < 3 ? s.passes : 3];
          ++shapes;
        }
  printf("forms: none %ld, 1024-point %ld, 2048-point %ld; window factors 3/5/8/16: %ld %ld %ld %ld\n", forms[0], forms[1],
         forms[2], buckets[3], buckets[5], buckets[8], buckets[16]);
  printf("groups 1..8:");
  for (int g = 1; g <= 8; ++g) printf(" %ld", splits[g]);
  printf("; short last group %ld; direct passes 1/2/3+: %ld %ld %ld\n", ragged, passes[1], passes[2], passes[3]);
  // the sweep reached what it is for
  CHECK(forms[0] > 0 && forms[1] > 0 && forms[2] > 0, "a form never occurred");
  CHECK(buckets[3] > 0 && buckets[5] > 0 && buckets[8] > 0 && buckets[16] > 0, "a window bucket never occurred");
  for (int g = 1; g <= 8; ++g) CHECK(splits[g] > 0, "groups == %d never occurred", g);
  CHECK(ragged > 0 && passes[1] > 0 && passes[2] > 0, "a short last group or a second pass never occurred");
  if (failures) {
    printf("%ld checks failed\n", failures);
    return 1;
  }
  printf("si shapes checked: %ld\n", shapes);
  return 0;
}
