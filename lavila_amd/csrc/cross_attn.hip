// Multi-query cross-attention pooling, gfx950: the core of coca.py's CrossAttention (reference
// lavila/models/coca.py:93-123) as the narrator uses it on top of the video tower (narrator.py:44-49,88-90): NQ learned
// queries x H heads attend to the T tokens of a clip through ONE key/value head of 64 channels shared by all query heads
// (to_kv has 2 * dim_head outputs):
//     out[b, n, h, :] = softmax_j( 0.125 * q[b, n, h, :] . k[b, j, :] ) v[b, j, :]
// Work per clip is tiny next to the tower (0.6 GFLOP vs 185): a latency-tolerant f32 VALU kernel -- 8 lanes per
// (query, head) row with 8 channels each, keys and values staged 64 at a time through LDS, flash-style running
// (max, sum) over blocks of 8 keys, no score tensor.
#include "common.h"

namespace {

constexpr int KC = 64;        // keys per LDS chunk
constexpr int ROWS = 32;      // (query, head) rows per 256-thread workgroup

template <typename T>
__global__ __launch_bounds__(256) void mq_cross_attn_kernel(const T* __restrict__ q, int64_t q_bstride,
                                                            const T* __restrict__ kv, T* __restrict__ out, int NQ,
                                                            int H, int Tk) {
  __shared__ __attribute__((aligned(16))) float ks[KC][64], vs[KC][64];
  const int tid = threadIdx.x, sub = tid & 7, rloc = tid >> 3;
  const int b = blockIdx.y, nrows = NQ * H;
  const int row = blockIdx.x * ROWS + rloc;
  const int rr = row < nrows ? row : nrows - 1;
  float qv[8];
  Elem<T>::load8(q + (int64_t)b * q_bstride + (int64_t)rr * 64 + sub * 8, qv);
#pragma unroll
  for (int c = 0; c < 8; ++c) qv[c] *= 0.125f;
  float m = -INFINITY, l = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const T* kvb = kv + (int64_t)b * Tk * 128;
  for (int j0 = 0; j0 < Tk; j0 += KC) {
    __syncthreads();
    // stage 64 keys x (k | v): 1024 vectors of 8 elements, 4 per thread
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int vec = p * 256 + tid, key = vec >> 4, c8 = vec & 15;
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (j0 + key < Tk) Elem<T>::load8(kvb + (int64_t)(j0 + key) * 128 + c8 * 8, v);
      float* dst = c8 < 8 ? &ks[key][c8 * 8] : &vs[key][(c8 - 8) * 8];
      *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
      *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
    __syncthreads();
    const int nk = Tk - j0 < KC ? Tk - j0 : KC;
    for (int jb = 0; jb < nk; jb += 8) {
      float s[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float4 a = *reinterpret_cast<const float4*>(&ks[jb + i][sub * 8]);
        const float4 c = *reinterpret_cast<const float4*>(&ks[jb + i][sub * 8 + 4]);
        float d = qv[0] * a.x;
        d = fmaf(qv[1], a.y, d); d = fmaf(qv[2], a.z, d); d = fmaf(qv[3], a.w, d);
        d = fmaf(qv[4], c.x, d); d = fmaf(qv[5], c.y, d); d = fmaf(qv[6], c.z, d); d = fmaf(qv[7], c.w, d);
        d += dpp_move<0xB1>(d);       // lanes of a quad
        d += dpp_move<0x4E>(d);
        d += dpp_move<0x141>(d);      // the other quad of the 8-lane group (mirror within half rows)
        s[i] = jb + i < nk ? d : -INFINITY;
      }
      float mb = s[0];
#pragma unroll
      for (int i = 1; i < 8; ++i) mb = fmaxf(mb, s[i]);
      const float mn = fmaxf(m, mb);
      const float corr = __expf(m - mn);          // exp(-inf) = 0 on the first block
      l *= corr;
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[c] *= corr;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float p = __expf(s[i] - mn);        // masked keys: exp(-inf) = 0
        l += p;
        const float4 a = *reinterpret_cast<const float4*>(&vs[jb + i][sub * 8]);
        const float4 c = *reinterpret_cast<const float4*>(&vs[jb + i][sub * 8 + 4]);
        acc[0] = fmaf(p, a.x, acc[0]); acc[1] = fmaf(p, a.y, acc[1]); acc[2] = fmaf(p, a.z, acc[2]);
        acc[3] = fmaf(p, a.w, acc[3]); acc[4] = fmaf(p, c.x, acc[4]); acc[5] = fmaf(p, c.y, acc[5]);
        acc[6] = fmaf(p, c.z, acc[6]); acc[7] = fmaf(p, c.w, acc[7]);
      }
      m = mn;
    }
  }
  if (row < nrows) {
    const float inv = 1.f / l;
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] *= inv;
    Elem<T>::store8(out + ((int64_t)b * nrows + row) * 64 + sub * 8, acc);
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------
// Two kernels in the forward's VALU form and one small sum, no atomics:
//   mq_bwd_rows_kernel   the forward's mapping (8 lanes per (query, head) row, keys through LDS). Pass 1 repeats the forward
//                        (running max / sum / output) and leaves lse and delta = dO . O per row; pass 2 walks the keys again:
//                        p = exp(s - lse), ds = p (dO . v - delta), dq += ds k. The row's dq goes to `dq` (per-clip
//                        queries) or, f32, to a per-clip slab (shared queries).
//   mq_bwd_kv_kernel     8 lanes per KEY, 32 keys per workgroup, all NQ x H rows streamed through LDS 64 at a time in row
//                        order: dv += p dO, dk += ds q in f32 registers, one rounding at the end.
//   mq_bwd_dq_sum_kernel shared queries: the per-clip slabs added in clip order.
constexpr int RC = 64;        // (query, head) rows per LDS chunk of the key/value kernel

__device__ __forceinline__ float dot8_group(const float (&a)[8], const float4 x, const float4 y) {
  float d = a[0] * x.x;
  d = fmaf(a[1], x.y, d); d = fmaf(a[2], x.z, d); d = fmaf(a[3], x.w, d);
  d = fmaf(a[4], y.x, d); d = fmaf(a[5], y.y, d); d = fmaf(a[6], y.z, d); d = fmaf(a[7], y.w, d);
  d += dpp_move<0xB1>(d);       // lanes of a quad
  d += dpp_move<0x4E>(d);
  d += dpp_move<0x141>(d);      // the other quad of the 8-lane group
  return d;
}

template <typename T>
__device__ __forceinline__ void mq_stage_kv(float (*ks)[64], float (*vs)[64], const T* kvb, int j0, int Tk, int tid) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int vec = p * 256 + tid, key = vec >> 4, c8 = vec & 15;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (j0 + key < Tk) Elem<T>::load8(kvb + (int64_t)(j0 + key) * 128 + c8 * 8, v);
    float* dst = c8 < 8 ? &ks[key][c8 * 8] : &vs[key][(c8 - 8) * 8];
    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void mq_bwd_rows_kernel(const T* __restrict__ q, int64_t q_bstride,
                                                          const T* __restrict__ kv, const T* __restrict__ dout,
                                                          T* __restrict__ dq, float* __restrict__ dq_slab,
                                                          float* __restrict__ stats, int NQ, int H, int Tk) {
  __shared__ __attribute__((aligned(16))) float ks[KC][64], vs[KC][64];
  const int tid = threadIdx.x, sub = tid & 7, rloc = tid >> 3;
  const int b = blockIdx.y, nrows = NQ * H;
  const int row = blockIdx.x * ROWS + rloc;
  const int rr = row < nrows ? row : nrows - 1;
  float qv[8], dv[8];
  Elem<T>::load8(q + (int64_t)b * q_bstride + (int64_t)rr * 64 + sub * 8, qv);
  Elem<T>::load8(dout + ((int64_t)b * nrows + rr) * 64 + sub * 8, dv);
#pragma unroll
  for (int c = 0; c < 8; ++c) qv[c] *= 0.125f;
  const T* kvb = kv + (int64_t)b * Tk * 128;
  // pass 1: the forward
  float m = -INFINITY, l = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int j0 = 0; j0 < Tk; j0 += KC) {
    __syncthreads();
    mq_stage_kv<T>(ks, vs, kvb, j0, Tk, tid);
    __syncthreads();
    const int nk = Tk - j0 < KC ? Tk - j0 : KC;
    for (int j = 0; j < nk; ++j) {
      const float s = dot8_group(qv, *reinterpret_cast<const float4*>(&ks[j][sub * 8]),
                                 *reinterpret_cast<const float4*>(&ks[j][sub * 8 + 4]));
      const float mn = fmaxf(m, s);
      const float corr = __expf(m - mn);          // exp(-inf) = 0 on the first key
      const float p = __expf(s - mn);
      l = fmaf(l, corr, p);
      const float4 a = *reinterpret_cast<const float4*>(&vs[j][sub * 8]);
      const float4 c = *reinterpret_cast<const float4*>(&vs[j][sub * 8 + 4]);
      acc[0] = fmaf(p, a.x, acc[0] * corr); acc[1] = fmaf(p, a.y, acc[1] * corr);
      acc[2] = fmaf(p, a.z, acc[2] * corr); acc[3] = fmaf(p, a.w, acc[3] * corr);
      acc[4] = fmaf(p, c.x, acc[4] * corr); acc[5] = fmaf(p, c.y, acc[5] * corr);
      acc[6] = fmaf(p, c.z, acc[6] * corr); acc[7] = fmaf(p, c.w, acc[7] * corr);
      m = mn;
    }
  }
  float delta = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) delta = fmaf(dv[c], acc[c], delta);
  delta += dpp_move<0xB1>(delta);
  delta += dpp_move<0x4E>(delta);
  delta += dpp_move<0x141>(delta);
  delta /= l;
  const float lse = m + __logf(l);
  if (row < nrows && sub == 0) {
    stats[((int64_t)b * nrows + row) * 2] = lse;
    stats[((int64_t)b * nrows + row) * 2 + 1] = delta;
  }
  // pass 2: dq
  float dqa[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int j0 = 0; j0 < Tk; j0 += KC) {
    __syncthreads();
    mq_stage_kv<T>(ks, vs, kvb, j0, Tk, tid);
    __syncthreads();
    const int nk = Tk - j0 < KC ? Tk - j0 : KC;
    for (int j = 0; j < nk; ++j) {
      const float4 k0 = *reinterpret_cast<const float4*>(&ks[j][sub * 8]);
      const float4 k1 = *reinterpret_cast<const float4*>(&ks[j][sub * 8 + 4]);
      const float s = dot8_group(qv, k0, k1);
      const float dp = dot8_group(dv, *reinterpret_cast<const float4*>(&vs[j][sub * 8]),
                                  *reinterpret_cast<const float4*>(&vs[j][sub * 8 + 4]));
      const float ds = __expf(s - lse) * (dp - delta);
      dqa[0] = fmaf(ds, k0.x, dqa[0]); dqa[1] = fmaf(ds, k0.y, dqa[1]); dqa[2] = fmaf(ds, k0.z, dqa[2]);
      dqa[3] = fmaf(ds, k0.w, dqa[3]); dqa[4] = fmaf(ds, k1.x, dqa[4]); dqa[5] = fmaf(ds, k1.y, dqa[5]);
      dqa[6] = fmaf(ds, k1.z, dqa[6]); dqa[7] = fmaf(ds, k1.w, dqa[7]);
    }
  }
  if (row < nrows) {
#pragma unroll
    for (int c = 0; c < 8; ++c) dqa[c] *= 0.125f;
    const int64_t o = ((int64_t)b * nrows + row) * 64 + sub * 8;
    if (dq_slab != nullptr) Elem<float>::store8(dq_slab + o, dqa);
    else Elem<T>::store8(dq + o, dqa);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void mq_bwd_kv_kernel(const T* __restrict__ q, int64_t q_bstride,
                                                        const T* __restrict__ kv, const T* __restrict__ dout,
                                                        const float* __restrict__ stats, T* __restrict__ dkv, int NQ,
                                                        int H, int Tk) {
  __shared__ __attribute__((aligned(16))) float qs[RC][64], os[RC][64];
  __shared__ float st[RC][2];
  const int tid = threadIdx.x, sub = tid & 7;
  const int b = blockIdx.y, nrows = NQ * H;
  const int key = blockIdx.x * 32 + (tid >> 3);
  float kvv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, vv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (key < Tk) {
    Elem<T>::load8(kv + ((int64_t)b * Tk + key) * 128 + sub * 8, kvv);
    Elem<T>::load8(kv + ((int64_t)b * Tk + key) * 128 + 64 + sub * 8, vv);
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) kvv[c] *= 0.125f;
  float dk[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, dv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const T* qb = q + (int64_t)b * q_bstride;
  const T* ob = dout + (int64_t)b * nrows * 64;
  const float* sb = stats + (int64_t)b * nrows * 2;
  for (int r0 = 0; r0 < nrows; r0 += RC) {
    __syncthreads();
    // stage 64 rows of q and dO: 2 x 512 vectors of 8 elements
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int vec = p * 256 + tid, which = vec >> 9, r = (vec >> 3) & 63, c8 = vec & 7;
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (r0 + r < nrows) Elem<T>::load8((which ? ob : qb) + (int64_t)(r0 + r) * 64 + c8 * 8, v);
      float* dst = which ? &os[r][c8 * 8] : &qs[r][c8 * 8];
      *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
      *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
    if (tid < 2 * RC) st[tid >> 1][tid & 1] = r0 + (tid >> 1) < nrows ? sb[(int64_t)(r0 + (tid >> 1)) * 2 + (tid & 1)] : 0.f;
    __syncthreads();
    const int nr = nrows - r0 < RC ? nrows - r0 : RC;
    for (int r = 0; r < nr; ++r) {
      const float4 q0 = *reinterpret_cast<const float4*>(&qs[r][sub * 8]);
      const float4 q1 = *reinterpret_cast<const float4*>(&qs[r][sub * 8 + 4]);
      const float4 o0 = *reinterpret_cast<const float4*>(&os[r][sub * 8]);
      const float4 o1 = *reinterpret_cast<const float4*>(&os[r][sub * 8 + 4]);
      const float s = dot8_group(kvv, q0, q1);
      const float dp = dot8_group(vv, o0, o1);
      const float p = __expf(s - st[r][0]);
      const float ds = p * (dp - st[r][1]);
      dv[0] = fmaf(p, o0.x, dv[0]); dv[1] = fmaf(p, o0.y, dv[1]); dv[2] = fmaf(p, o0.z, dv[2]); dv[3] = fmaf(p, o0.w, dv[3]);
      dv[4] = fmaf(p, o1.x, dv[4]); dv[5] = fmaf(p, o1.y, dv[5]); dv[6] = fmaf(p, o1.z, dv[6]); dv[7] = fmaf(p, o1.w, dv[7]);
      dk[0] = fmaf(ds, q0.x, dk[0]); dk[1] = fmaf(ds, q0.y, dk[1]); dk[2] = fmaf(ds, q0.z, dk[2]); dk[3] = fmaf(ds, q0.w, dk[3]);
      dk[4] = fmaf(ds, q1.x, dk[4]); dk[5] = fmaf(ds, q1.y, dk[5]); dk[6] = fmaf(ds, q1.z, dk[6]); dk[7] = fmaf(ds, q1.w, dk[7]);
    }
  }
  if (key < Tk) {
#pragma unroll
    for (int c = 0; c < 8; ++c) dk[c] *= 0.125f;
    Elem<T>::store8(dkv + ((int64_t)b * Tk + key) * 128 + sub * 8, dk);
    Elem<T>::store8(dkv + ((int64_t)b * Tk + key) * 128 + 64 + sub * 8, dv);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void mq_bwd_dq_sum_kernel(const float* __restrict__ slab, T* __restrict__ dq, int B,
                                                            int64_t n8) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int b = 0; b < B; ++b) {
    float v[8];
    Elem<float>::load8(slab + ((int64_t)b * n8 + i) * 8, v);
#pragma unroll
    for (int c = 0; c < 8; ++c) a[c] += v[c];
  }
  Elem<T>::store8(dq + i * 8, a);
}

}  // namespace

extern "C" int lvl_mq_cross_attn_fwd(const void* q, int64_t q_batch_stride, const void* kv, void* out, int B, int NQ,
                                     int H, int Tk, int dtype, void* stream) {
  LVL_REQUIRE(B == 0 || (q && kv && out), "mq_cross_attn_fwd: null pointer");
  LVL_REQUIRE(B >= 0 && NQ > 0 && H > 0 && Tk > 0, "mq_cross_attn_fwd: bad shape B=%d NQ=%d H=%d T=%d", B, NQ, H, Tk);
  LVL_REQUIRE(lvl_aligned16(q) && lvl_aligned16(kv) && lvl_aligned16(out) && q_batch_stride % 8 == 0,
              "mq_cross_attn_fwd: pointers must be 16-byte aligned");
  if (B == 0) return LVL_OK;
  const dim3 grid((unsigned)((NQ * H + ROWS - 1) / ROWS), (unsigned)B);
  LVL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((mq_cross_attn_kernel<T>), grid, dim3(256), 0, (hipStream_t)stream,
                                               (const T*)q, q_batch_stride, (const T*)kv, (T*)out, NQ, H, Tk));
  LVL_CHECK_LAUNCH("mq_cross_attn_fwd");
  return LVL_OK;
}

extern "C" int64_t lvl_mq_cross_attn_bwd_ws(int B, int NQ, int H, int shared_q) {
  if (B <= 0 || NQ <= 0 || H <= 0) return -1;
  const int64_t rows = (int64_t)B * NQ * H;
  return rows * 2 + (shared_q ? rows * 64 : 0);       // (lse, delta) per row (+ the per-clip dq slabs)
}

extern "C" int lvl_mq_cross_attn_bwd(const void* q, int64_t q_batch_stride, const void* kv, const void* dout, void* dq,
                                     void* dkv, float* ws, int B, int NQ, int H, int Tk, int dtype, void* stream) {
  LVL_REQUIRE(B == 0 || (q && kv && dout && dq && dkv && ws), "mq_cross_attn_bwd: null pointer");
  LVL_REQUIRE(B >= 0 && NQ > 0 && H > 0 && Tk > 0, "mq_cross_attn_bwd: bad shape B=%d NQ=%d H=%d T=%d", B, NQ, H, Tk);
  LVL_REQUIRE(lvl_aligned16(q) && lvl_aligned16(kv) && lvl_aligned16(dout) && lvl_aligned16(dq) && lvl_aligned16(dkv) &&
                  lvl_aligned16(ws) && q_batch_stride % 8 == 0,
              "mq_cross_attn_bwd: pointers must be 16-byte aligned");
  LVL_REQUIRE(q_batch_stride == 0 || q_batch_stride == (int64_t)NQ * H * 64,
              "mq_cross_attn_bwd: the query batch stride is 0 (shared queries) or NQ*H*64");
  if (B == 0) return LVL_OK;
  hipStream_t st = (hipStream_t)stream;
  const int nrows = NQ * H;
  float* slab = q_batch_stride == 0 ? ws + (int64_t)B * nrows * 2 : nullptr;
  const dim3 rgrid((unsigned)((nrows + ROWS - 1) / ROWS), (unsigned)B), kgrid((unsigned)((Tk + 31) / 32), (unsigned)B);
  LVL_DISPATCH_DTYPE(dtype, {
    hipLaunchKernelGGL((mq_bwd_rows_kernel<T>), rgrid, dim3(256), 0, st, (const T*)q, q_batch_stride, (const T*)kv,
                       (const T*)dout, (T*)dq, slab, ws, NQ, H, Tk);
    hipLaunchKernelGGL((mq_bwd_kv_kernel<T>), kgrid, dim3(256), 0, st, (const T*)q, q_batch_stride, (const T*)kv,
                       (const T*)dout, (const float*)ws, (T*)dkv, NQ, H, Tk);
    if (slab != nullptr) {
      const int64_t n8 = (int64_t)nrows * 8;
      hipLaunchKernelGGL((mq_bwd_dq_sum_kernel<T>), dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, st,
                         (const float*)slab, (T*)dq, B, n8);
    }
  });
  LVL_CHECK_LAUNCH("mq_cross_attn_bwd");
  return LVL_OK;
}
