// Key-masked bidirectional attention (forward + backward): the entry points, and the shape-generic kernels (f32 arithmetic,
// any element type, any key count) that serve float32 and bf16 beyond 256 keys; bf16 with Tk <= 256 goes to the KEYMASK
// instantiations of the MFMA rows attention (cross_attn_mfma.hip, cross_attn_bwd_mfma.hip: one workgroup per (context,
// head), exact single-pass softmax) through the rows attention's own check and launchers (RowsAttn, internal.h): an entry
// here keeps its null-pointer, dtype and alignment lines and the launches of the generic kernels. The self-attention of a padded text batch (DistilBERT's MultiHeadSelfAttention under an attention_mask; transformers fills
// the scores of hidden keys with the most negative finite value before the softmax). Operands as lvl_attn_rows_drop_fwd:
// q rows q_stride apart, per-context keys / values kv_stride apart, contexts kv_ctx_stride apart; keymask [contexts, Tk]
// bytes, non-zero = visible, NULL = all visible.
//   P = softmax over the VISIBLE keys of the context (row maximum over visible keys only); a hidden key has P = 0 and
//   dS = 0 exactly: the generic kernels never read it, and its dk / dv rows are written as zeros.
//   A context with no visible key gets the uniform distribution over its Tk keys (what the finite fill gives): out =
//   mean(v), dv = mean-weighted dout, dq = dk = 0.
// The attn_generic.hip form: one 64-lane wave owns one (query row, head) in the forward and the dq pass, one (key, head)
// in the dk / dv pass; online softmax over 64-key chunks, p broadcast with v_readlane. The backward recomputes the row's
// (max, sum) and delta = dout . out and leaves (lse, delta) per (row, head) in the workspace for the key pass. No atomics, no
// cross-wave communication: bit-reproducible.
//
// DROP (lvl_keymask_attn_drop_fwd / _bwd, p > 0): dropout on the probabilities with the mask of dropout.h over
// e = ((((ctx * H + h) * idx_qrep + i) << s) | j, s = 8 up to 256 keys (the MFMA kernels' mapping), else the smallest s with
// 2^s >= Tk. The running (m, l), lse and delta = sum_j P dP are those of the UNDROPPED softmax; the output accumulates
// Pd = keep ? scale P : 0, the backward regenerates keep: dP = keep ? scale (dout . v) : 0, dS = P (dP - delta), dv = Pd^T dout.
// One Philox call gives the keep bits of four consecutive keys: in the row passes every lane draws one group, so one call
// per lane covers the 256 keys of four chunks and a lane fetches its bit with a shuffle; in the key pass a workgroup owns
// four consecutive keys (one per wave) and its waves share the groups of the query rows through LDS.
#include "internal.h"
#include "dropout.h"

namespace {

template <typename T>
__device__ __forceinline__ void km_load_row64(const T* p, float (&r)[64]) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float v[8];
    Elem<T>::load8(p + c * 8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) r[c * 8 + j] = v[j];
  }
}

template <typename T>
__device__ __forceinline__ float km_dot_row64(const T* p, const float (&r)[64]) {
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float v[8];
    Elem<T>::load8(p + c * 8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = fmaf(v[j], r[c * 8 + j], acc);
  }
  return acc;
}

// no visible key in the context (wave-uniform)
__device__ __forceinline__ bool km_context_empty(const uint8_t* mk, int Tk, int lane) {
  if (mk == nullptr) return false;
  for (int j0 = 0; j0 < Tk; j0 += 64) {
    const int j = j0 + lane;
    if (__builtin_amdgcn_ballot_w64(j < Tk && mk[j] != 0) != 0) return false;
  }
  return true;
}

constexpr int kMfmaMaxKeys = 256;       // bf16 up to here: the key-masked instantiations of the MFMA rows attention

struct KmOperands {
  int64_t q_stride, kv_stride, kv_ctx_stride, mask_ctx_stride;
  int Tk, H, qrep;
};

struct KmDrop {
  uint64_t seed;
  uint32_t site, thr;
  float scale;
  int idx_qrep;                // query rows per context in the element index (>= qrep: the full call's)
  int gshift;                  // s - 2: element group = (row id << gshift) | (key >> 2)
};

// element group 0 of query row `row` (of all contexts) under head h
__device__ __forceinline__ uint64_t km_row_group(const KmOperands& d, const KmDrop& dr, int64_t ctx, int64_t row, int h) {
  return ((uint64_t)(ctx * d.H + h) * (uint64_t)dr.idx_qrep + (uint64_t)(row - ctx * d.qrep)) << dr.gshift;
}

// a * b rounded to float32, never contracted into the add or subtract that uses it: dP = scale * (dout . v) has to be the
// same number in the pass that sums delta and in the passes that subtract it (one visible key: dP - delta == 0 exactly)
__device__ __forceinline__ float km_mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// keep bits of the 256 keys j0 .. j0 + 255 of a row (j0 % 256 == 0): this lane's nibble is keys j0 + 4 lane .. + 3
__device__ __forceinline__ uint32_t km_keep256(const KmDrop& dr, uint64_t rowgrp, int j0, int lane) {
  return lvl_drop::group_keep(dr.seed, dr.site, rowgrp + (uint64_t)((j0 >> 2) + lane), dr.thr);
}

// keep of key j0 + lane (j0 % 64 == 0) out of the nibbles of its 256-key block; every lane of the wave calls it
__device__ __forceinline__ bool km_keep_lane(uint32_t nib, int j0, int lane) {
  const uint32_t kb = (uint32_t)__shfl((int)nib, ((j0 & 255) >> 2) + (lane >> 2), 64);
  return ((kb >> (lane & 3)) & 1u) != 0;
}

// The forward of one (query row, head): running (m, l) and the unnormalised output channel `lane` in acc. qs is the
// query scaled by 1/8. Hidden keys are never loaded. DROP: acc sums the kept keys times scale, (m, l) all visible keys.
template <typename T, bool DROP>
__device__ __forceinline__ void km_row_forward(const float (&qs)[64], const T* kb, const T* vb, const uint8_t* mk,
                                               bool empty, const KmOperands& d, const KmDrop& dr, uint64_t rowgrp,
                                               int lane, float& m, float& l, float& acc) {
  m = -INFINITY; l = 0.f; acc = 0.f;
  uint32_t nib = 0;
  for (int j0 = 0; j0 < d.Tk; j0 += 64) {
    if constexpr (DROP)
      if ((j0 & 255) == 0) nib = km_keep256(dr, rowgrp, j0, lane);
    const int j = j0 + lane;
    const bool vis = j < d.Tk && (empty || mk == nullptr || mk[j] != 0);
    const uint64_t bits = __builtin_amdgcn_ballot_w64(vis);
    if (bits == 0) continue;                                  // a chunk of hidden keys: m may still be -inf
    float s = -INFINITY;
    if (vis) s = empty ? 0.f : km_dot_row64(kb + (int64_t)j * d.kv_stride, qs);
    const float m_new = fmaxf(m, wave_max(s));                // finite: the chunk has a visible key
    const float alpha = __expf(m - m_new);                    // exp(-inf) = 0 on the first visible chunk
    float p = vis ? __expf(s - m_new) : 0.f;
    l = l * alpha + wave_sum(p);
    acc *= alpha;
    uint64_t kept = bits;
    if constexpr (DROP) {
      const bool keep = km_keep_lane(nib, j0, lane);
      p = keep ? dr.scale * p : 0.f;
      kept = __builtin_amdgcn_ballot_w64(vis && keep);        // a dropped key's value row is not read either
    }
    const int cnt = (d.Tk - j0 < 64) ? (d.Tk - j0) : 64;
    for (int jj = 0; jj < cnt; ++jj) {
      if (!((kept >> jj) & 1)) continue;
      const float pj = read_lane(p, jj);
      acc = fmaf(pj, Elem<T>::load(vb + (int64_t)(j0 + jj) * d.kv_stride + lane), acc);
    }
    m = m_new;
  }
}

template <typename T, bool DROP>
__global__ __launch_bounds__(256) void keymask_fwd_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                          const T* __restrict__ v, const uint8_t* __restrict__ mask,
                                                          T* __restrict__ out, KmOperands d, KmDrop dr, int64_t total) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= total) return;
  const int h = (int)(wid % d.H);
  const int64_t row = wid / d.H, ctx = row / d.qrep;
  const uint8_t* mk = mask ? mask + ctx * d.mask_ctx_stride : nullptr;
  const bool empty = km_context_empty(mk, d.Tk, lane);
  float qs[64];
  km_load_row64(q + row * d.q_stride + h * 64, qs);
#pragma unroll
  for (int c = 0; c < 64; ++c) qs[c] *= 0.125f;
  float m, l, acc;
  km_row_forward<T, DROP>(qs, k + ctx * d.kv_ctx_stride + h * 64, v + ctx * d.kv_ctx_stride + h * 64, mk, empty, d, dr,
                          DROP ? km_row_group(d, dr, ctx, row, h) : 0, lane, m, l, acc);
  Elem<T>::store(out + row * ((int64_t)d.H * 64) + h * 64 + lane, acc / l);
}

// dq pass: wave per (query row, head). Leaves stats[(row * H + h) * 2] = (lse, delta = dout . out) for the key pass.
template <typename T, bool DROP>
__global__ __launch_bounds__(256) void keymask_bwd_dq_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                             const T* __restrict__ v, const uint8_t* __restrict__ mask,
                                                             const T* __restrict__ dout, T* __restrict__ dq,
                                                             float* __restrict__ stats, KmOperands d, KmDrop dr,
                                                             int64_t total) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= total) return;
  const int h = (int)(wid % d.H);
  const int64_t row = wid / d.H, ctx = row / d.qrep;
  const uint8_t* mk = mask ? mask + ctx * d.mask_ctx_stride : nullptr;
  const bool empty = km_context_empty(mk, d.Tk, lane);
  const T* kb = k + ctx * d.kv_ctx_stride + h * 64;
  const T* vb = v + ctx * d.kv_ctx_stride + h * 64;
  const T* gp = dout + row * ((int64_t)d.H * 64) + h * 64;
  float qs[64], go[64];
  km_load_row64(q + row * d.q_stride + h * 64, qs);
  km_load_row64(gp, go);
#pragma unroll
  for (int c = 0; c < 64; ++c) qs[c] *= 0.125f;
  // pass 1: the row's (max, sum) and delta = sum_j P_j (dout . v_j) -- dout . out regrouped over the keys, from the SAME
  // dot products as pass 2 and the key pass: with one visible key P = 1 and dS = dp - delta is exactly 0
  // DROP: dp is dP = keep ? scale (dout . v_j) : 0 in both passes; P, l and lse stay those of the undropped softmax
  const uint64_t rowgrp = DROP ? km_row_group(d, dr, ctx, row, h) : 0;
  uint32_t nib = 0;
  float m = -INFINITY, l = 0.f, dsum = 0.f;
  for (int j0 = 0; j0 < d.Tk; j0 += 64) {
    if constexpr (DROP)
      if ((j0 & 255) == 0) nib = km_keep256(dr, rowgrp, j0, lane);
    const int j = j0 + lane;
    const bool vis = j < d.Tk && (empty || mk == nullptr || mk[j] != 0);
    if (__builtin_amdgcn_ballot_w64(vis) == 0) continue;
    bool keep = true;
    if constexpr (DROP) keep = km_keep_lane(nib, j0, lane);
    float s = -INFINITY, dp = 0.f;
    if (vis) {
      s = empty ? 0.f : km_dot_row64(kb + (int64_t)j * d.kv_stride, qs);
      if (keep) dp = km_dot_row64(vb + (int64_t)j * d.kv_stride, go);
      if constexpr (DROP) dp = km_mul_rounded(dr.scale, dp);  // dP
    }
    const float m_new = fmaxf(m, wave_max(s));
    const float alpha = __expf(m - m_new);
    const float p = vis ? __expf(s - m_new) : 0.f;
    l = l * alpha + wave_sum(p);
    dsum = dsum * alpha + wave_sum(p * dp);
    m = m_new;
  }
  const float delta = dsum / l;
  const float lse = m + __logf(l);
  if (lane == 0) {
    stats[wid * 2] = lse;
    stats[wid * 2 + 1] = delta;
  }
  float acc = 0.f;
  if (!empty) {                                               // the uniform row does not depend on the scores: dS = 0
    for (int j0 = 0; j0 < d.Tk; j0 += 64) {
      if constexpr (DROP)
        if ((j0 & 255) == 0) nib = km_keep256(dr, rowgrp, j0, lane);
      const int j = j0 + lane;
      const bool vis = j < d.Tk && (mk == nullptr || mk[j] != 0);
      const uint64_t bits = __builtin_amdgcn_ballot_w64(vis);
      if (bits == 0) continue;
      bool keep = true;
      if constexpr (DROP) keep = km_keep_lane(nib, j0, lane);
      float ds = 0.f;
      if (vis) {
        const float s = km_dot_row64(kb + (int64_t)j * d.kv_stride, qs);
        float dp = keep ? km_dot_row64(vb + (int64_t)j * d.kv_stride, go) : 0.f;
        if constexpr (DROP) dp = km_mul_rounded(dr.scale, dp);
        ds = __expf(s - lse) * (dp - delta);
      }
      const int cnt = (d.Tk - j0 < 64) ? (d.Tk - j0) : 64;
      for (int jj = 0; jj < cnt; ++jj) {
        if (!((bits >> jj) & 1)) continue;
        acc = fmaf(read_lane(ds, jj), Elem<T>::load(kb + (int64_t)(j0 + jj) * d.kv_stride + lane), acc);
      }
    }
  }
  Elem<T>::store(dq + row * d.q_stride + h * 64 + lane, acc * 0.125f);
}

// dk / dv pass: wave per (context, key, head) over the qrep query rows of the context
template <typename T>
__global__ __launch_bounds__(256) void keymask_bwd_dkv_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                              const T* __restrict__ v, const uint8_t* __restrict__ mask,
                                                              const T* __restrict__ dout, const float* __restrict__ stats,
                                                              T* __restrict__ dk, T* __restrict__ dv, KmOperands d,
                                                              int64_t total) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= total) return;
  const int h = (int)(wid % d.H);
  const int j = (int)((wid / d.H) % d.Tk);
  const int64_t ctx = wid / ((int64_t)d.H * d.Tk);
  const uint8_t* mk = mask ? mask + ctx * d.mask_ctx_stride : nullptr;
  const bool empty = km_context_empty(mk, d.Tk, lane);
  const int64_t koff = ctx * d.kv_ctx_stride + (int64_t)j * d.kv_stride + h * 64;
  if (!empty && mk != nullptr && mk[j] == 0) {                // a hidden key: exact zeros, nothing read
    Elem<T>::store(dk + koff + lane, 0.f);
    Elem<T>::store(dv + koff + lane, 0.f);
    return;
  }
  float ks[64], vr[64];
  km_load_row64(k + koff, ks);
  km_load_row64(v + koff, vr);
#pragma unroll
  for (int c = 0; c < 64; ++c) ks[c] *= 0.125f;
  const int64_t D = (int64_t)d.H * 64, row0 = ctx * d.qrep;
  float dka = 0.f, dva = 0.f;
  for (int i0 = 0; i0 < d.qrep; i0 += 64) {
    const int i = i0 + lane;
    float p = 0.f, ds = 0.f;
    if (i < d.qrep) {
      const int64_t row = row0 + i;
      const float s = empty ? 0.f : km_dot_row64(q + row * d.q_stride + h * 64, ks);
      const float dp = km_dot_row64(dout + row * D + h * 64, vr);
      const float* st = stats + (row * d.H + h) * 2;
      p = __expf(s - st[0]);
      ds = empty ? 0.f : p * (dp - st[1]);
    }
    const int cnt = (d.qrep - i0 < 64) ? (d.qrep - i0) : 64;
    for (int ii = 0; ii < cnt; ++ii) {
      const int64_t row = row0 + i0 + ii;
      dva = fmaf(read_lane(p, ii), Elem<T>::load(dout + row * D + h * 64 + lane), dva);
      dka = fmaf(read_lane(ds, ii), Elem<T>::load(q + row * d.q_stride + h * 64 + lane), dka);
    }
  }
  Elem<T>::store(dk + koff + lane, dka * 0.125f);
  Elem<T>::store(dv + koff + lane, dva);
}

// The key pass under dropout: one workgroup per (context, 4 consecutive keys, head), wave w owns key 4 jg + w. The keep
// bits of (query row, the workgroup's four keys) are ONE element group: wave w draws the groups of rows i00 + 64 w + lane
// of a 256-row round into LDS, and every wave reads its own bit of them.
template <typename T>
__global__ __launch_bounds__(256) void keymask_bwd_dkv_drop_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                   const T* __restrict__ v,
                                                                   const uint8_t* __restrict__ mask,
                                                                   const T* __restrict__ dout,
                                                                   const float* __restrict__ stats, T* __restrict__ dk,
                                                                   T* __restrict__ dv, KmOperands d, KmDrop dr,
                                                                   int kgroups) {
  __shared__ uint32_t nibs[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = (int)(blockIdx.x % d.H);
  const int jg = (int)((blockIdx.x / d.H) % kgroups);
  const int64_t ctx = blockIdx.x / ((unsigned)d.H * (unsigned)kgroups);
  const int j = jg * 4 + wave;
  const uint8_t* mk = mask ? mask + ctx * d.mask_ctx_stride : nullptr;
  const bool empty = km_context_empty(mk, d.Tk, lane);
  const bool hidden = j < d.Tk && !empty && mk != nullptr && mk[j] == 0;
  const bool active = j < d.Tk && !hidden;                    // wave-uniform; inactive waves still draw and join barriers
  const int64_t koff = ctx * d.kv_ctx_stride + (int64_t)j * d.kv_stride + h * 64;
  if (hidden) {                                               // exact zeros, nothing read
    Elem<T>::store(dk + koff + lane, 0.f);
    Elem<T>::store(dv + koff + lane, 0.f);
  }
  float ks[64], vr[64];
#pragma unroll
  for (int c = 0; c < 64; ++c) ks[c] = vr[c] = 0.f;
  if (active) {
    km_load_row64(k + koff, ks);
    km_load_row64(v + koff, vr);
#pragma unroll
    for (int c = 0; c < 64; ++c) ks[c] *= 0.125f;
  }
  const int64_t D = (int64_t)d.H * 64, row0 = ctx * d.qrep;
  const uint64_t rid0 = (uint64_t)(ctx * d.H + h) * (uint64_t)dr.idx_qrep;
  float dka = 0.f, dva = 0.f;
  for (int i00 = 0; i00 < d.qrep; i00 += 256) {
    __syncthreads();                                          // the last round's bits have been read
    if (i00 + 64 * wave < d.qrep)
      nibs[wave][lane] = lvl_drop::group_keep(dr.seed, dr.site,
                                              ((rid0 + (uint64_t)(i00 + 64 * wave + lane)) << dr.gshift) + (uint64_t)jg, dr.thr);
    __syncthreads();
    if (!active) continue;
    for (int i0 = i00; i0 < d.qrep && i0 < i00 + 256; i0 += 64) {
      const int i = i0 + lane;
      const bool keep = ((nibs[(i0 - i00) >> 6][lane] >> wave) & 1u) != 0;
      float pd = 0.f, ds = 0.f;
      if (i < d.qrep) {
        const int64_t row = row0 + i;
        const float s = empty ? 0.f : km_dot_row64(q + row * d.q_stride + h * 64, ks);
        const float* st = stats + (row * d.H + h) * 2;
        const float p = __expf(s - st[0]);
        float dp = 0.f;
        if (keep) {
          dp = km_mul_rounded(dr.scale, km_dot_row64(dout + row * D + h * 64, vr));
          pd = dr.scale * p;
        }
        ds = empty ? 0.f : p * (dp - st[1]);
      }
      const int cnt = (d.qrep - i0 < 64) ? (d.qrep - i0) : 64;
      for (int ii = 0; ii < cnt; ++ii) {
        const int64_t row = row0 + i0 + ii;
        dva = fmaf(read_lane(pd, ii), Elem<T>::load(dout + row * D + h * 64 + lane), dva);
        dka = fmaf(read_lane(ds, ii), Elem<T>::load(q + row * d.q_stride + h * 64 + lane), dka);
      }
    }
  }
  if (active) {
    Elem<T>::store(dk + koff + lane, dka * 0.125f);
    Elem<T>::store(dv + koff + lane, dva);
  }
}

}  // namespace

extern "C" int lvl_keymask_attn_fwd(const void* q, const void* k, const void* v, const uint8_t* keymask, void* out,
                                    int contexts, int qrep, int Tk, int H, int64_t q_stride, int64_t kv_stride,
                                    int64_t kv_ctx_stride, int64_t mask_ctx_stride, int dtype, void* stream) {
  LVL_REQUIRE(contexts == 0 || (q && k && v && out), "keymask_attn_fwd: null pointer");
  const RowsAttn r{q, k, v, contexts, qrep, Tk, H, q_stride, kv_stride, kv_ctx_stride,
                   /*keymasked*/ true, keymask, mask_ctx_stride, /*causal*/ false, /*seed, site, p*/ 0, 0, 0.f,
                   /*idx_qrep*/ qrep};
  if (int rc = lvl_rows_attn_check("keymask_attn_fwd", r)) return rc;
  LVL_REQUIRE(dtype == LVL_F32 || dtype == LVL_BF16, "keymask_attn_fwd: unknown dtype %d", dtype);
  LVL_REQUIRE(lvl_aligned16(q) && lvl_aligned16(k) && lvl_aligned16(v) && lvl_aligned16(out),
              "keymask_attn_fwd: pointers must be 16-byte aligned");
  if (contexts == 0) return LVL_OK;
  if (dtype == LVL_BF16 && Tk <= kMfmaMaxKeys) return lvl_launch_rows_attn_mfma_fwd(r, out, (hipStream_t)stream);
  const KmOperands d{q_stride, kv_stride, kv_ctx_stride, mask_ctx_stride, Tk, H, qrep};
  const int64_t total = (int64_t)contexts * qrep * H;
  LVL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((keymask_fwd_kernel<T, false>), dim3((unsigned)((total + 3) / 4)), dim3(256),
                                               0, (hipStream_t)stream, (const T*)q, (const T*)k, (const T*)v, keymask,
                                               (T*)out, d, KmDrop{}, total));
  LVL_CHECK_LAUNCH("keymask_attn_fwd");
  return LVL_OK;
}

extern "C" int lvl_keymask_attn_bwd(const void* q, const void* k, const void* v, const uint8_t* keymask, const void* dout,
                                    void* dq, void* dk, void* dv, float* ws, int contexts, int qrep, int Tk, int H,
                                    int64_t q_stride, int64_t kv_stride, int64_t kv_ctx_stride, int64_t mask_ctx_stride,
                                    int dtype, void* stream) {
  LVL_REQUIRE(contexts == 0 || (q && k && v && dout && dq && dk && dv && ws), "keymask_attn_bwd: null pointer");
  const RowsAttn r{q, k, v, contexts, qrep, Tk, H, q_stride, kv_stride, kv_ctx_stride,
                   /*keymasked*/ true, keymask, mask_ctx_stride, /*causal*/ false, /*seed, site, p*/ 0, 0, 0.f,
                   /*idx_qrep*/ qrep};
  if (int rc = lvl_rows_attn_check("keymask_attn_bwd", r)) return rc;
  LVL_REQUIRE(dtype == LVL_F32 || dtype == LVL_BF16, "keymask_attn_bwd: unknown dtype %d", dtype);
  LVL_REQUIRE(lvl_aligned16(q) && lvl_aligned16(k) && lvl_aligned16(v) && lvl_aligned16(dout) && lvl_aligned16(dq) &&
                  lvl_aligned16(dk) && lvl_aligned16(dv) && lvl_aligned16(ws),
              "keymask_attn_bwd: pointers must be 16-byte aligned");
  if (contexts == 0) return LVL_OK;
  if (dtype == LVL_BF16 && Tk <= kMfmaMaxKeys)
    return lvl_launch_rows_attn_mfma_bwd(r, dout, dq, dk, dv, (hipStream_t)stream);
  const KmOperands d{q_stride, kv_stride, kv_ctx_stride, mask_ctx_stride, Tk, H, qrep};
  const int64_t total_q = (int64_t)contexts * qrep * H, total_k = (int64_t)contexts * Tk * H;
  LVL_DISPATCH_DTYPE(dtype, {
    hipLaunchKernelGGL((keymask_bwd_dq_kernel<T, false>), dim3((unsigned)((total_q + 3) / 4)), dim3(256), 0,
                       (hipStream_t)stream, (const T*)q, (const T*)k, (const T*)v, keymask, (const T*)dout, (T*)dq, ws, d,
                       KmDrop{}, total_q);
    hipLaunchKernelGGL((keymask_bwd_dkv_kernel<T>), dim3((unsigned)((total_k + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (const T*)q, (const T*)k, (const T*)v, keymask, (const T*)dout, (const float*)ws, (T*)dk, (T*)dv, d,
                       total_k);
  });
  LVL_CHECK_LAUNCH("keymask_attn_bwd");
  return LVL_OK;
}

// ---- dropout on the key-masked probabilities -------------------------------------------------------------------------
static KmDrop km_drop_args(int Tk, int idx_qrep, uint64_t seed, uint32_t site, float p) {
  int s = 8;
  while ((1ll << s) < Tk) ++s;
  return KmDrop{seed, site, lvl_drop::threshold(p), lvl_drop::scale_of(p), idx_qrep, s - 2};
}

extern "C" int lvl_keymask_attn_drop_fwd(const void* q, const void* k, const void* v, const uint8_t* keymask, void* out,
                                         int contexts, int qrep, int Tk, int H, int64_t q_stride, int64_t kv_stride,
                                         int64_t kv_ctx_stride, int64_t mask_ctx_stride, int idx_qrep, uint64_t seed,
                                         uint32_t site, float p, int dtype, void* stream) {
  LVL_REQUIRE(contexts == 0 || (q && k && v && out), "keymask_attn_drop_fwd: null pointer");
  const RowsAttn r{q, k, v, contexts, qrep, Tk, H, q_stride, kv_stride, kv_ctx_stride,
                   /*keymasked*/ true, keymask, mask_ctx_stride, /*causal*/ false, seed, site, p, idx_qrep};
  if (int rc = lvl_rows_attn_check("keymask_attn_drop_fwd", r)) return rc;
  LVL_REQUIRE(dtype == LVL_F32 || dtype == LVL_BF16, "keymask_attn_drop_fwd: unknown dtype %d", dtype);
  LVL_REQUIRE(lvl_aligned16(q) && lvl_aligned16(k) && lvl_aligned16(v) && lvl_aligned16(out),
              "keymask_attn_drop_fwd: pointers must be 16-byte aligned");
  if (contexts == 0) return LVL_OK;
  if (p == 0.f)                                               // today's kernels, today's bits
    return lvl_keymask_attn_fwd(q, k, v, keymask, out, contexts, qrep, Tk, H, q_stride, kv_stride, kv_ctx_stride,
                                mask_ctx_stride, dtype, stream);
  if (dtype == LVL_BF16 && Tk <= kMfmaMaxKeys) return lvl_launch_rows_attn_mfma_fwd(r, out, (hipStream_t)stream);
  const KmOperands d{q_stride, kv_stride, kv_ctx_stride, mask_ctx_stride, Tk, H, qrep};
  const KmDrop dr = km_drop_args(Tk, idx_qrep, seed, site, p);
  const int64_t total = (int64_t)contexts * qrep * H;
  LVL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((keymask_fwd_kernel<T, true>), dim3((unsigned)((total + 3) / 4)), dim3(256), 0,
                                               (hipStream_t)stream, (const T*)q, (const T*)k, (const T*)v, keymask,
                                               (T*)out, d, dr, total));
  LVL_CHECK_LAUNCH("keymask_attn_drop_fwd");
  return LVL_OK;
}

extern "C" int lvl_keymask_attn_drop_bwd(const void* q, const void* k, const void* v, const uint8_t* keymask,
                                         const void* dout, void* dq, void* dk, void* dv, float* ws, int contexts, int qrep,
                                         int Tk, int H, int64_t q_stride, int64_t kv_stride, int64_t kv_ctx_stride,
                                         int64_t mask_ctx_stride, int idx_qrep, uint64_t seed, uint32_t site, float p,
                                         int dtype, void* stream) {
  LVL_REQUIRE(contexts == 0 || (q && k && v && dout && dq && dk && dv && ws), "keymask_attn_drop_bwd: null pointer");
  const RowsAttn r{q, k, v, contexts, qrep, Tk, H, q_stride, kv_stride, kv_ctx_stride,
                   /*keymasked*/ true, keymask, mask_ctx_stride, /*causal*/ false, seed, site, p, idx_qrep};
  if (int rc = lvl_rows_attn_check("keymask_attn_drop_bwd", r)) return rc;
  LVL_REQUIRE(dtype == LVL_F32 || dtype == LVL_BF16, "keymask_attn_drop_bwd: unknown dtype %d", dtype);
  LVL_REQUIRE(lvl_aligned16(q) && lvl_aligned16(k) && lvl_aligned16(v) && lvl_aligned16(dout) && lvl_aligned16(dq) &&
                  lvl_aligned16(dk) && lvl_aligned16(dv) && lvl_aligned16(ws),
              "keymask_attn_drop_bwd: pointers must be 16-byte aligned");
  if (contexts == 0) return LVL_OK;
  if (p == 0.f)
    return lvl_keymask_attn_bwd(q, k, v, keymask, dout, dq, dk, dv, ws, contexts, qrep, Tk, H, q_stride, kv_stride,
                                kv_ctx_stride, mask_ctx_stride, dtype, stream);
  if (dtype == LVL_BF16 && Tk <= kMfmaMaxKeys)
    return lvl_launch_rows_attn_mfma_bwd(r, dout, dq, dk, dv, (hipStream_t)stream);
  const KmOperands d{q_stride, kv_stride, kv_ctx_stride, mask_ctx_stride, Tk, H, qrep};
  const KmDrop dr = km_drop_args(Tk, idx_qrep, seed, site, p);
  const int64_t total_q = (int64_t)contexts * qrep * H;
  const int kgroups = (Tk + 3) / 4;
  LVL_DISPATCH_DTYPE(dtype, {
    hipLaunchKernelGGL((keymask_bwd_dq_kernel<T, true>), dim3((unsigned)((total_q + 3) / 4)), dim3(256), 0,
                       (hipStream_t)stream, (const T*)q, (const T*)k, (const T*)v, keymask, (const T*)dout, (T*)dq, ws, d, dr,
                       total_q);
    hipLaunchKernelGGL((keymask_bwd_dkv_drop_kernel<T>), dim3((unsigned)((int64_t)contexts * kgroups * H)), dim3(256), 0,
                       (hipStream_t)stream, (const T*)q, (const T*)k, (const T*)v, keymask, (const T*)dout, (const float*)ws,
                       (T*)dk, (T*)dv, d, dr, kgroups);
  });
  LVL_CHECK_LAUNCH("keymask_attn_drop_bwd");
  return LVL_OK;
}
