// Key visibility of one context for the MFMA rows attention (cross_attn_mfma.hip, cross_attn_bwd_mfma.hip; KEYMASK).
// In the score fragments a lane of group g = lane >> 4 holds keys k*16 + g*4 + r (k < 16, r < 4): bit 4 k + r of `bits` says
// whether that key takes part in the softmax. Keys >= Tk never do. A context whose mask hides every key is `uniform`: all
// its Tk keys take part with score 0 (what transformers' finite fill gives) and no gradient reaches the scores.
#pragma once
#include <stdint.h>

struct KeyVis {
  uint64_t bits;
  bool uniform;
};

template <bool KEYMASK>
__device__ __forceinline__ KeyVis key_visibility(const uint8_t* __restrict__ mask, size_t ctx_off, int Tk, int g) {
  KeyVis kv{0, false};
  if constexpr (KEYMASK) {
    uint64_t in_range = 0, vis = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = k * 16 + g * 4 + r;
        if (key < Tk) {
          in_range |= 1ull << (4 * k + r);
          if (mask == nullptr || mask[ctx_off + key] != 0) vis |= 1ull << (4 * k + r);
        }
      }
    }
    // the four lane groups of a wave hold disjoint keys: the context has a visible key iff some lane has one
    kv.uniform = __builtin_amdgcn_ballot_w64(vis != 0) == 0;
    kv.bits = kv.uniform ? in_range : vis;
  }
  return kv;
}
