// The ONE definition of the decoder's dropout mask (device + host inline): Philox4x32-10 (Salmon et al., SC'11) with the
// standard constants, counter-based, so that a forward kernel and its backward regenerate the same mask from
// (seed, site, element) and no mask tensor is ever stored.
//   g   = e >> 2                       four consecutive elements share one Philox call
//   ctr = (g & 0xffffffff, g >> 32, site, 0),  key = (seed & 0xffffffff, seed >> 32)
//   w   = philox4x32_10(ctr, key)[e & 3]
//   T   = min(2^32 - 1, floor(p * 2^32 + 0.5));  keep iff w >= T;  scale = 1 / (1 - p) in float32
// p = 0 keeps everything with scale == 1. Element index e: row sites over [rows, D] use row * D + col; attention sites
// (((b * H + h) * L + i) << 8) | j for query i and key j < 256. Sites are numbered in the reference's execution order
// (gpt2_gated.py:421-495): 0 = embedding, block i: 1 + 6 i + {0 cross-attention probabilities, 1 cross c_proj, 2
// mlp_crossattention, 3 self-attention probabilities, 4 self c_proj, 5 mlp}. tests/dropout_reference.py restates this in numpy.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LVL_DROP_HD __host__ __device__ __forceinline__
#else
#define LVL_DROP_HD inline
#endif

namespace lvl_drop {

struct U4 { uint32_t v[4]; };

LVL_DROP_HD void mulhilo(uint32_t a, uint32_t b, uint32_t& hi, uint32_t& lo) {
  const uint64_t p = (uint64_t)a * b;
  hi = (uint32_t)(p >> 32);
  lo = (uint32_t)p;
}

LVL_DROP_HD U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint32_t h0, l0, h1, l1;
    mulhilo(0xD2511F53u, c0, h0, l0);
    mulhilo(0xCD9E8D57u, c2, h1, l1);
    const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
    c0 = n0; c1 = l1; c2 = n2; c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  U4 o;
  o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
  return o;
}

// the four random words of element group g = e >> 2
LVL_DROP_HD U4 group_words(uint64_t seed, uint32_t site, uint64_t g) {
  return philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), site, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}

LVL_DROP_HD uint32_t threshold(float p) {
  const double t = (double)p * 4294967296.0 + 0.5;
  return t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;      // (uint32_t) of a non-negative double truncates = floor
}

LVL_DROP_HD float scale_of(float p) { return 1.0f / (1.0f - p); }

// keep bits of the four elements of group g: bit r = element 4 g + r
LVL_DROP_HD uint32_t group_keep(uint64_t seed, uint32_t site, uint64_t g, uint32_t thr) {
  const U4 w = group_words(seed, site, g);
  return (uint32_t)(w.v[0] >= thr) | ((uint32_t)(w.v[1] >= thr) << 1) | ((uint32_t)(w.v[2] >= thr) << 2) |
         ((uint32_t)(w.v[3] >= thr) << 3);
}

// keep bits of the 8 consecutive elements e0 .. e0 + 7 (e0 % 8 == 0): two Philox calls
LVL_DROP_HD uint32_t keep8(uint64_t seed, uint32_t site, uint64_t e0, uint32_t thr) {
  return group_keep(seed, site, e0 >> 2, thr) | (group_keep(seed, site, (e0 >> 2) + 1, thr) << 4);
}

LVL_DROP_HD bool keep1(uint64_t seed, uint32_t site, uint64_t e, uint32_t thr) {
  return (group_keep(seed, site, e >> 2, thr) >> (e & 3)) & 1u;
}

}  // namespace lvl_drop
