// lvl_linear_wgrad's kernel (wgrad_kernel.h; design notes in wgrad_mfma.hip) for the 160-family: 5x5 MFMA tiles per wave
// (workgroup tiles 320x160, 160x320, 160x160: both sides of every Conv1D weight of a 1600-wide GPT-2 XL decoder -- 1600 /
// 3200 / 4800 / 6400 -- and of the 320-wide test layout) and 8x5 (256x320, 256x160: a vocabulary padded to 256s against
// such a width, the tied lm_head of a small-vocabulary decoder). make_plan (wgrad_mfma.hip) considers them only for shapes
// that none of the older configurations divides. What differs from the older instantiations, inside the kernel:
//   * TA = 5 is odd: the mid-step barrier splits the A tiles 2 + 3;
//   * ANY number of (split, tile) pairs is mapped onto the XCDs (4800 x 1600 is 150 tiles at S = 1), see the decode.
#include "wgrad_kernel.h"

int lvl_launch_wgrad_160(int cfg, int tiles_k, int ntiles, int S, const void* dy, const void* x, float* part, float* bpart,
                         int64_t M, int N, int K, unsigned* sched, hipStream_t st) {
  const Plan p{cfg, tiles_k, ntiles, S, true};
  switch (cfg) {
    case 0: return launch<4, 2, 5, 5>(p, dy, x, part, bpart, M, N, K, sched, st);
    case 1: return launch<2, 4, 5, 5>(p, dy, x, part, bpart, M, N, K, sched, st);
    case 2: return launch<2, 2, 5, 5>(p, dy, x, part, bpart, M, N, K, sched, st);
    case 3: return launch<2, 4, 8, 5>(p, dy, x, part, bpart, M, N, K, sched, st);
    case 4: return launch<2, 2, 8, 5>(p, dy, x, part, bpart, M, N, K, sched, st);
  }
  return lvl_fail(LVL_EINVAL, "linear_wgrad: unknown 160-family configuration %d", cfg);
}
