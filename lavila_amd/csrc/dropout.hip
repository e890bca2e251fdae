// Stand-alone forms of the decoder's dropout (dropout.h: Philox4x32-10 mask from (seed, site, element)), gfx950:
//   lvl_dropout_mask    the keep mask of a range of elements as bytes -- what the tests and the golden tool read to get the
//                       very masks the fused kernels apply (the same device function, lvl_drop::group_keep)
//   lvl_dropout_apply   out = keep ? x / (1 - p) : 0 over n elements (n % 8 == 0), in place or not: the embedding site
//                       (gpt2_gated.py:899), and its own backward when applied to the gradient
// One thread per 8 elements = two Philox calls; f32 arithmetic, bf16 or f32 storage, 16-byte accesses.
#include "common.h"
#include "dropout.h"

namespace {

__global__ __launch_bounds__(256) void dropout_mask_kernel(uint8_t* __restrict__ out, int64_t n, uint64_t elem0,
                                                           uint64_t seed, uint32_t site, uint32_t thr) {
  // one thread per element group of 4 that the range touches
  const uint64_t g0 = elem0 >> 2;
  const int64_t ngroups = (int64_t)(((elem0 + (uint64_t)n - 1) >> 2) - g0) + 1;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < ngroups; i += (int64_t)gridDim.x * 256) {
    const uint64_t g = g0 + (uint64_t)i;
    const uint32_t bits = lvl_drop::group_keep(seed, site, g, thr);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint64_t e = (g << 2) + r;
      if (e >= elem0 && e - elem0 < (uint64_t)n) out[e - elem0] = (bits >> r) & 1u;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void dropout_apply_kernel(const T* x, T* out, int64_t n8, uint64_t seed, uint32_t site,
                                                            uint32_t thr, float scale) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    float v[8];
    Elem<T>::load8(x + i * 8, v);
    const uint32_t bits = lvl_drop::keep8(seed, site, (uint64_t)i * 8, thr);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = ((bits >> k) & 1u) ? scale * v[k] : 0.f;
    Elem<T>::store8(out + i * 8, v);
  }
}

int grid_for(int64_t items) {
  const int64_t b = (items + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace

extern "C" int lvl_dropout_mask(uint8_t* out, int64_t n, uint64_t elem0, uint64_t seed, uint32_t site, float p,
                                void* stream) {
  LVL_REQUIRE(n >= 0 && (n == 0 || out), "dropout_mask: null pointer or negative count");
  LVL_REQUIRE(p >= 0.f && p < 1.f, "dropout_mask: p = %g must be in [0, 1)", (double)p);
  LVL_REQUIRE(n == 0 || elem0 + (uint64_t)(n - 1) >= elem0, "dropout_mask: element range wraps");
  if (n == 0) return LVL_OK;
  hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)grid_for(n / 4 + 2)), dim3(256), 0, (hipStream_t)stream, out, n,
                     elem0, seed, site, lvl_drop::threshold(p));
  LVL_CHECK_LAUNCH("dropout_mask");
  return LVL_OK;
}

extern "C" int lvl_dropout_apply(const void* x, void* out, int64_t n, uint64_t seed, uint32_t site, float p, int dtype,
                                 void* stream) {
  LVL_REQUIRE(n >= 0 && n % 8 == 0 && (n == 0 || (x && out)), "dropout_apply: n = %lld must be a multiple of 8, pointers non-null",
              (long long)n);
  LVL_REQUIRE(p >= 0.f && p < 1.f, "dropout_apply: p = %g must be in [0, 1)", (double)p);
  LVL_REQUIRE(lvl_aligned16(x) && lvl_aligned16(out), "dropout_apply: pointers must be 16-byte aligned");
  if (n == 0) return LVL_OK;
  const int64_t n8 = n / 8;
  LVL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((dropout_apply_kernel<T>), dim3((unsigned)grid_for(n8)), dim3(256), 0,
                                               (hipStream_t)stream, (const T*)x, (T*)out, n8, seed, site,
                                               lvl_drop::threshold(p), lvl_drop::scale_of(p)));
  LVL_CHECK_LAUNCH("dropout_apply");
  return LVL_OK;
}
