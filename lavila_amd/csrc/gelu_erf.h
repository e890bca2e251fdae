// The exact (erf) GELU, a = 0.5 u (1 + erf(u / sqrt 2)), and its derivative Phi(u) + u phi(u). One definition for the kernels
// that apply the activation to a stored pre-activation (decode.hip: lvl_act_fwd / lvl_act_bwd, LVL_ACT_GELU_ERF) and for the
// TN GEMM's epilogues 6-8 (gemm_tn_kernel.h, instantiated in gemm_tn_gelu.hip): what an epilogue writes and what
// lvl_act_fwd rebuilds from the kept pre-activation must agree to the bit (tests/test_gpu_gemm_gelu_epilogues.py).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.7071067811865476f)); }

__device__ __forceinline__ float gelu_erf_grad(float x) {       // Phi(u) + u phi(u)
  const float cdf = 0.5f * (1.f + erff(x * 0.7071067811865476f));
  return cdf + x * 0.3989422804014327f * __expf(-0.5f * x * x);
}

// both from one erf: y and g are the values of the two functions above (same expressions on the same erff result)
__device__ __forceinline__ void gelu_erf_pair(float x, float& y, float& g) {
  const float e = erff(x * 0.7071067811865476f);
  y = 0.5f * x * (1.f + e);
  const float cdf = 0.5f * (1.f + e);
  g = cdf + x * 0.3989422804014327f * __expf(-0.5f * x * x);
}
