// Contrastive (InfoNCE) head in slab form, gfx950: shape-generic VALU kernels (any E % 8 == 0) and the backward.
// The forward for E in {64,128,256,512} runs on the matrix cores (clip_loss_mfma.hip).
//
// Each rank owns B rows of both logit matrices: direction 0 = logits_per_image rows
// (scale*img_local) @ txt_all^T, direction 1 = logits_per_text rows (scale*txt_local) @ img_all^T.
// One workgroup per (row, direction): the [B,G] logits slab is never written to HBM (optional debug
// output aside); the row statistics (log-sum-exp, diagonal, expectation, argmax) come out of one
// streaming pass, and backward recomputes the logits from the gathered embeddings + gathered LSEs,
// so no gradient collective is needed.
#include "clip_row_state.h"
#include "internal.h"

namespace {

// a_s[e] = k * A[gi][e]: the workgroup's own row, staged in LDS for the column sweep (visible after the barrier)
template <typename T>
__device__ __forceinline__ void stage_row(float* a_s, const T* A, int gi, int E, float k) {
  for (int e = threadIdx.x; e < E; e += blockDim.x) a_s[e] = k * Elem<T>::load(A + (int64_t)gi * E + e);
  __syncthreads();
}

// second half of both backwards: dst[e] = k * sum_j c[j] * Bm[j][e], the coefficient row c[G] resident in LDS
template <typename T>
__device__ __forceinline__ void contract_rows(float* dst, const float* c, const T* Bm, int G, int E, float k) {
  for (int e = threadIdx.x; e < E; e += blockDim.x) {
    float acc = 0.f;
    for (int j = 0; j < G; ++j) acc = fmaf(c[j], Elem<T>::load(Bm + (int64_t)j * E + e), acc);
    dst[e] = k * acc;
  }
}

template <typename T>
__device__ __forceinline__ float dot_row(const T* __restrict__ b, const float* __restrict__ a_s, int E) {
  float acc = 0.f;
  for (int e = 0; e < E; e += 8) {
    float v[8];
    Elem<T>::load8(b + e, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = fmaf(a_s[e + j], v[j], acc);
  }
  return acc;
}

template <typename T>
__global__ __launch_bounds__(256) void clip_fwd_kernel(const T* __restrict__ img_all, const T* __restrict__ txt_all,
                                                       const float* __restrict__ scale_p, int B, int G, int E, int row0,
                                                       float* __restrict__ stats, int32_t* __restrict__ argmax,
                                                       float* __restrict__ logits) {
  extern __shared__ __attribute__((aligned(16))) float smem[];   // a_s[E] then the 4 wave records
  using State = RowState<1, 1>;
  float* a_s = smem;
  float* red = smem + E;
  const int i = blockIdx.x, dir = blockIdx.y, gi = row0 + i;
  const T* A = dir == 0 ? img_all : txt_all;
  const T* Bm = dir == 0 ? txt_all : img_all;
  stage_row(a_s, A, gi, E, *scale_p);

  State s;
  for (int j = threadIdx.x; j < G; j += blockDim.x) {
    const float z = dot_row(Bm + (int64_t)j * E, a_s, E);
    if (logits) logits[((int64_t)dir * B + i) * G + j] = z;
    if (j == gi) s.dg[0] = z;
    s.update(j, z, z, 0);
  }
  s.wave_reduce();
  if ((threadIdx.x & 63) == 0) s.store(red + (threadIdx.x >> 6) * State::REC);
  __syncthreads();
  // stats row: {log-sum-exp, diagonal (target) logit, sum_j softmax_j * logit_j, max logit}
  if (threadIdx.x == 0)
    State::finish(red, State::REC, stats + ((int64_t)dir * B + i) * State::STATS, argmax + dir * B + i);
}

template <typename T>
__global__ __launch_bounds__(256) void clip_bwd_kernel(const T* __restrict__ img_all, const T* __restrict__ txt_all,
                                                       const float* __restrict__ lse_all,
                                                       const float* __restrict__ scale_p,
                                                       const float* __restrict__ upstream_p, float coef, int B,
                                                       int G, int E, int row0, int rows_only,
                                                       float* __restrict__ dimg, float* __restrict__ dtxt) {
  extern __shared__ __attribute__((aligned(16))) float smem[];   // a_s[E], c[G]
  float* a_s = smem;
  float* c = smem + E;
  const int i = blockIdx.x, dir = blockIdx.y, gi = row0 + i;
  const T* A = dir == 0 ? img_all : txt_all;
  const T* Bm = dir == 0 ? txt_all : img_all;
  const float scale = *scale_p;
  stage_row(a_s, A, gi, E, scale);
  const float L_own = lse_all[(int64_t)dir * G + gi];
  const float* L_other = lse_all + (int64_t)(1 - dir) * G;
  for (int j = threadIdx.x; j < G; j += blockDim.x) {
    const float z = dot_row(Bm + (int64_t)j * E, a_s, E);
    // rows_only (CLIPLoss(local_loss=True) without gather_with_grad, loss.py:86-88): the gathered partner rows carry
    // no gradient, so only this row's own cross-entropy contributes
    c[j] = rows_only ? __expf(z - L_own) - (j == gi ? 1.f : 0.f)
                     : __expf(z - L_own) + __expf(z - L_other[j]) - (j == gi ? 2.f : 0.f);
  }
  __syncthreads();
  float* dst = (dir == 0 ? dimg : dtxt) + (int64_t)i * E;
  const float k = coef * scale * (upstream_p ? *upstream_p : 1.0f);
  contract_rows(dst, c, Bm, G, E, k);
}

}  // namespace

extern "C" int lvl_clip_loss_fwd(const void* img_all, const void* txt_all, const float* scale, int B, int G, int E, int row0,
                                 float* stats, int32_t* argmax, float* logits, int dtype, void* stream) {
  LVL_REQUIRE(img_all && txt_all && scale && stats && argmax, "clip_loss_fwd: null pointer");
  LVL_REQUIRE(B >= 0 && G > 0 && E > 0 && E % 8 == 0 && row0 >= 0 && row0 + B <= G,
              "clip_loss_fwd: bad shape B=%d G=%d E=%d row0=%d", B, G, E, row0);
  LVL_REQUIRE(lvl_aligned16(img_all) && lvl_aligned16(txt_all), "clip_loss_fwd: pointers must be 16-byte aligned");
  if (B == 0) return LVL_OK;
  if (lvl_clip_mfma_supported(E) && (dtype == LVL_F32 || dtype == LVL_BF16))
    return lvl_clip_fwd_mfma(img_all, txt_all, scale, B, G, E, row0, stats, argmax, logits, dtype, (hipStream_t)stream);
  const size_t shmem = (size_t)(E + 32) * sizeof(float);
  LVL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((clip_fwd_kernel<T>), dim3(B, 2), dim3(256), shmem, (hipStream_t)stream,
                                               (const T*)img_all, (const T*)txt_all, scale, B, G, E, row0, stats,
                                               argmax, logits));
  LVL_CHECK_LAUNCH("clip_loss_fwd");
  return LVL_OK;
}

extern "C" int lvl_clip_loss_bwd(const void* img_all, const void* txt_all, const float* lse_all, const float* scale,
                                 const float* upstream, float coef, int B, int G, int E, int row0, int rows_only,
                                 float* dimg, float* dtxt, int dtype, void* stream) {
  LVL_REQUIRE(img_all && txt_all && lse_all && scale && dimg && dtxt, "clip_loss_bwd: null pointer");
  LVL_REQUIRE(B >= 0 && G > 0 && E > 0 && E % 8 == 0 && row0 >= 0 && row0 + B <= G,
              "clip_loss_bwd: bad shape B=%d G=%d E=%d row0=%d", B, G, E, row0);
  LVL_REQUIRE((size_t)(E + G) * sizeof(float) <= 150 * 1024, "clip_loss_bwd: G=%d too large for the LDS-resident row", G);
  LVL_REQUIRE(lvl_aligned16(img_all) && lvl_aligned16(txt_all), "clip_loss_bwd: pointers must be 16-byte aligned");
  if (B == 0) return LVL_OK;
  const size_t shmem = (size_t)(E + G) * sizeof(float);
  LVL_DISPATCH_DTYPE(dtype, {
    if (shmem > 64 * 1024)
      if (int rc = lvl_allow_lds<clip_bwd_kernel<T>>()) return rc;
    hipLaunchKernelGGL((clip_bwd_kernel<T>), dim3(B, 2), dim3(256), shmem, (hipStream_t)stream, (const T*)img_all,
                       (const T*)txt_all, lse_all, scale, upstream, coef, B, G, E, row0, rows_only, dimg, dtxt);
  });
  LVL_CHECK_LAUNCH("clip_loss_bwd");
  return LVL_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// SSLCLIPLoss (loss.py:121-217): per-pair temperature. scale(i,j) = scales[ind[i] + ind[j]] with
// scales = {pseudo, sqrt(pseudo*real), real}; logits = scale(i,j) * (a_i . b_j). Same slab structure; the row
// statistics additionally keep the three bucket expectations sum_{j in bucket k} p_j z_j (z = unscaled dot) that
// give d(loss)/d(scales[k]) without a second pass.
// ---------------------------------------------------------------------------------------------------------------
namespace {

template <typename T>
__global__ __launch_bounds__(256) void ssl_fwd_kernel(const T* __restrict__ img_all, const T* __restrict__ txt_all,
                                                      const int32_t* __restrict__ ind,
                                                      const float* __restrict__ scales, int B, int G, int E, int row0,
                                                      float* __restrict__ stats, int32_t* __restrict__ argmax,
                                                      float* __restrict__ logits) {
  extern __shared__ __attribute__((aligned(16))) float smem[];   // a_s[E] then the 4 wave records
  using State = RowState<3, 2>;
  float* a_s = smem;
  float* red = smem + E;
  const int i = blockIdx.x, dir = blockIdx.y, gi = row0 + i;
  const T* A = dir == 0 ? img_all : txt_all;
  const T* Bm = dir == 0 ? txt_all : img_all;
  stage_row(a_s, A, gi, E, 1.f);
  const int ind_i = ind[gi] != 0;                                   // any non-zero indicator counts as 1
  const float sc0 = scales[ind_i], sc1 = scales[ind_i + 1];          // partner indicator 0 / 1

  // State::update spelled out on plain locals: through the struct or any call this loop allocates 3-4 fewer SGPRs
  float m = -INFINITY, l = 0.f, ex[3] = {0.f, 0.f, 0.f}, best = -INFINITY, diag_z = 0.f, diag_l = 0.f;
  int bi = 0x7fffffff;
  for (int j = threadIdx.x; j < G; j += blockDim.x) {
    const float zr = dot_row(Bm + (int64_t)j * E, a_s, E);
    const int ind_j = ind[j] != 0;
    const int bucket = ind_i + ind_j;
    const float z = zr * (ind_j ? sc1 : sc0);
    if (logits) logits[((int64_t)dir * B + i) * G + j] = z;
    if (j == gi) { diag_z = zr; diag_l = z; }
    if (z > best) { best = z; bi = j; }
    const float mn = fmaxf(m, z);
    const float al = __expf(m - mn), p = __expf(z - mn);
    l = l * al + p;
#pragma unroll
    for (int k = 0; k < 3; ++k) ex[k] = ex[k] * al + (bucket == k ? p * zr : 0.f);
    m = mn;
  }
  State s{m, l, {ex[0], ex[1], ex[2]}, best, {diag_z, diag_l}, bi};
  s.wave_reduce();
  if ((threadIdx.x & 63) == 0) s.store(red + (threadIdx.x >> 6) * State::REC);
  __syncthreads();
  // stats row: {log-sum-exp, diagonal (target) logit, the three bucket expectations of the unscaled dot, diagonal
  // unscaled dot, max logit, 0}
  if (threadIdx.x == 0)
    State::finish(red, State::REC, stats + ((int64_t)dir * B + i) * State::STATS, argmax + dir * B + i);
}

template <typename T>
__global__ __launch_bounds__(256) void ssl_bwd_kernel(const T* __restrict__ img_all, const T* __restrict__ txt_all,
                                                      const int32_t* __restrict__ ind,
                                                      const float* __restrict__ lse_all,
                                                      const float* __restrict__ scales,
                                                      const float* __restrict__ upstream_p, float coef, int B, int G,
                                                      int E, int row0, float* __restrict__ dimg,
                                                      float* __restrict__ dtxt) {
  extern __shared__ __attribute__((aligned(16))) float smem[];   // a_s[E], c[G]
  float* a_s = smem;
  float* c = smem + E;
  const int i = blockIdx.x, dir = blockIdx.y, gi = row0 + i;
  const T* A = dir == 0 ? img_all : txt_all;
  const T* Bm = dir == 0 ? txt_all : img_all;
  stage_row(a_s, A, gi, E, 1.f);
  const int ind_i = ind[gi] != 0;                                   // any non-zero indicator counts as 1
  const float sc0 = scales[ind_i], sc1 = scales[ind_i + 1];
  const float L_own = lse_all[(int64_t)dir * G + gi];
  const float* L_other = lse_all + (int64_t)(1 - dir) * G;
  for (int j = threadIdx.x; j < G; j += blockDim.x) {
    const float s = ind[j] != 0 ? sc1 : sc0;
    const float z = dot_row(Bm + (int64_t)j * E, a_s, E) * s;
    c[j] = s * (__expf(z - L_own) + __expf(z - L_other[j]) - (j == gi ? 2.f : 0.f));
  }
  __syncthreads();
  float* dst = (dir == 0 ? dimg : dtxt) + (int64_t)i * E;
  const float k = coef * (upstream_p ? *upstream_p : 1.0f);
  contract_rows(dst, c, Bm, G, E, k);
}

}  // namespace

extern "C" int lvl_ssl_clip_loss_fwd(const void* img_all, const void* txt_all, const int32_t* ind_all,
                                     const float* scales3, int B, int G, int E, int row0, float* stats,
                                     int32_t* argmax, float* logits, int dtype, void* stream) {
  LVL_REQUIRE(img_all && txt_all && ind_all && scales3 && stats && argmax, "ssl_clip_loss_fwd: null pointer");
  LVL_REQUIRE(B >= 0 && G > 0 && E > 0 && E % 8 == 0 && row0 >= 0 && row0 + B <= G,
              "ssl_clip_loss_fwd: bad shape B=%d G=%d E=%d row0=%d", B, G, E, row0);
  LVL_REQUIRE(lvl_aligned16(img_all) && lvl_aligned16(txt_all), "ssl_clip_loss_fwd: pointers must be 16-byte aligned");
  if (B == 0) return LVL_OK;
  const size_t shmem = (size_t)(E + 40) * sizeof(float);
  LVL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((ssl_fwd_kernel<T>), dim3(B, 2), dim3(256), shmem, (hipStream_t)stream,
                                               (const T*)img_all, (const T*)txt_all, ind_all, scales3, B, G, E, row0,
                                               stats, argmax, logits));
  LVL_CHECK_LAUNCH("ssl_clip_loss_fwd");
  return LVL_OK;
}

extern "C" int lvl_ssl_clip_loss_bwd(const void* img_all, const void* txt_all, const int32_t* ind_all,
                                     const float* lse_all, const float* scales3, const float* upstream, float coef,
                                     int B, int G, int E, int row0, float* dimg, float* dtxt, int dtype,
                                     void* stream) {
  LVL_REQUIRE(img_all && txt_all && ind_all && lse_all && scales3 && dimg && dtxt, "ssl_clip_loss_bwd: null pointer");
  LVL_REQUIRE(B >= 0 && G > 0 && E > 0 && E % 8 == 0 && row0 >= 0 && row0 + B <= G,
              "ssl_clip_loss_bwd: bad shape B=%d G=%d E=%d row0=%d", B, G, E, row0);
  LVL_REQUIRE((size_t)(E + G) * sizeof(float) <= 150 * 1024, "ssl_clip_loss_bwd: G=%d too large for the LDS-resident row", G);
  LVL_REQUIRE(lvl_aligned16(img_all) && lvl_aligned16(txt_all), "ssl_clip_loss_bwd: pointers must be 16-byte aligned");
  if (B == 0) return LVL_OK;
  const size_t shmem = (size_t)(E + G) * sizeof(float);
  LVL_DISPATCH_DTYPE(dtype, {
    if (shmem > 64 * 1024)
      if (int rc = lvl_allow_lds<ssl_bwd_kernel<T>>()) return rc;
    hipLaunchKernelGGL((ssl_bwd_kernel<T>), dim3(B, 2), dim3(256), shmem, (hipStream_t)stream, (const T*)img_all,
                       (const T*)txt_all, ind_all, lse_all, scales3, upstream, coef, B, G, E, row0, dimg, dtxt);
  });
  LVL_CHECK_LAUNCH("ssl_clip_loss_bwd");
  return LVL_OK;
}
