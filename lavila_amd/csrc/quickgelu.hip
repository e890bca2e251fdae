// a = QuickGELU(u), rebuilt from the pre-activation that the TN GEMM's LVL_EPI_BIAS_QUICKGELU epilogue keeps. gfx950.
//
// Selective activation recompute does not keep the MLP's hidden activation: the weight-gradient GEMM of fc2 gets it back from
// here. The expression is the epilogue's own (common.h: qgelu1 on the bf16 value for bf16, quick_gelu for f32), so the rebuilt
// tensor equals the forward's to the bit. HBM-bound, one pass: 16 bytes per lane and access, consecutive lanes on consecutive
// vectors, kQgUnroll vectors per thread requested before the first one is used.
#include "common.h"

namespace {

constexpr int kQgThreads = 256;
constexpr int kQgUnroll = 4;          // 8-element vectors in flight per thread
constexpr int kQgBlocks = 8192;       // grid cap (a chunk of kQgThreads * kQgUnroll vectors per workgroup and step)

template <typename T> struct QgAct;
template <> struct QgAct<bf16_t> {
  static __device__ __forceinline__ float f(float u) {
    float y, r;
    qgelu1(u, y, r);
    return y;
  }
};
template <> struct QgAct<float> {
  static __device__ __forceinline__ float f(float u) { return quick_gelu(u); }
};

template <typename T>
__global__ __launch_bounds__(kQgThreads) void quickgelu_apply_kernel(const T* __restrict__ u, T* __restrict__ a, int64_t nvec) {
  constexpr int64_t kChunk = (int64_t)kQgThreads * kQgUnroll;
  const int64_t nfull = nvec / kChunk;
  for (int64_t ch = blockIdx.x; ch < nfull; ch += gridDim.x) {
    const int64_t v0 = ch * kChunk + threadIdx.x;
    float x[kQgUnroll][8];
#pragma unroll
    for (int k = 0; k < kQgUnroll; ++k) Elem<T>::load8(u + (v0 + k * kQgThreads) * 8, x[k]);
#pragma unroll
    for (int k = 0; k < kQgUnroll; ++k) {
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = QgAct<T>::f(x[k][j]);
      Elem<T>::store8(a + (v0 + k * kQgThreads) * 8, o);
    }
  }
  // the vectors behind the last whole chunk (fewer than kChunk): one per thread and step
  for (int64_t v = nfull * kChunk + (int64_t)blockIdx.x * kQgThreads + threadIdx.x; v < nvec;
       v += (int64_t)gridDim.x * kQgThreads) {
    float x[8], o[8];
    Elem<T>::load8(u + v * 8, x);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = QgAct<T>::f(x[j]);
    Elem<T>::store8(a + v * 8, o);
  }
}

}  // namespace

extern "C" int lvl_quickgelu_apply(const void* u, void* a, int64_t rows, int cols, int dtype, void* stream) {
  LVL_REQUIRE(rows == 0 || (u && a), "quickgelu_apply: null pointer");
  LVL_REQUIRE(rows >= 0 && cols > 0 && cols % 8 == 0, "quickgelu_apply: cols=%d must be a multiple of 8", cols);
  LVL_REQUIRE(lvl_aligned16(u) && lvl_aligned16(a), "quickgelu_apply: pointers must be 16-byte aligned");
  if (rows == 0) return LVL_OK;
  const int64_t nvec = rows * (cols / 8);
  int64_t blocks = (nvec + (int64_t)kQgThreads * kQgUnroll - 1) / ((int64_t)kQgThreads * kQgUnroll);
  if (blocks > kQgBlocks) blocks = kQgBlocks;
  LVL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((quickgelu_apply_kernel<T>), dim3((unsigned)blocks), dim3(kQgThreads), 0,
                                               (hipStream_t)stream, (const T*)u, (T*)a, nvec));
  LVL_CHECK_LAUNCH("quickgelu_apply");
  return LVL_OK;
}
