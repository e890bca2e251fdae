// LayerNorm forward/backward, optionally fused with the residual(+bias) add that feeds it. gfx950.
//
// HBM-bound: one pass over [rows, cols]. One 64-lane wave owns one row at a time and keeps the
// whole row in registers, so every operand is read exactly once; statistics are the two-pass (mean, then
// centred variance) form in f32, matching F.layer_norm. Consecutive lanes take consecutive W-element vectors.
// Two vector widths: W = 4 when cols is a multiple of 256 (768 -> exactly 3 vectors per lane, no idle lanes,
// 25 % fewer registers than 2 x 8 -> one more wave per SIMD in the backward), W = 8 otherwise.
// Algorithmic bytes per row (E = element size): fwd cols*E*(n_in + n_out), bwd cols*E*(1 + n_in + 1).
#include <stdlib.h>

#include "internal.h"

// The general and the exact-width kernels must agree to the bit (activation checkpointing recomputes a forward that may take
// the other instantiation): no implicit contraction in this file, every fused multiply-add is written as one, and each
// expression of the row arithmetic is written once, in the ln_*_elem helpers that all four kernels call.
#pragma clang fp contract(off)

namespace {

constexpr int kRowsPerBlock = 4;          // 4 waves per 256-thread workgroup
constexpr int kLnBwdParts = 768;          // partial dgamma/dbeta/dxsum slabs (one per workgroup)

// The row arithmetic, per element (helpers over whole vectors cost the backward registers and a wave per SIMD). What differs
// between the kernels stays in them: column guards, operand flags, and with those the order x, += x2, += bias of the input sum.
// a row mean from the lanes' partial sums: mu, the variance, and the two means of the backward
__device__ __forceinline__ float ln_mean(float lane_sum, float inv_cols) { return wave_sum(lane_sum) * inv_cols; }
__device__ __forceinline__ void ln_sq_elem(float v, float mu, float& sq) { const float d = v - mu; sq = fmaf(d, d, sq); }
__device__ __forceinline__ float ln_rstd(float sq, float inv_cols, float eps) { return rsqrtf(ln_mean(sq, inv_cols) + eps); }
// the normalised element: the forward's, and what the backward rebuilds from its packed operands
__device__ __forceinline__ float ln_xhat_elem(float v, float mu, float rs) { return (v - mu) * rs; }
__device__ __forceinline__ float ln_norm_elem(float v, float mu, float rs, float g, float b) {
  return fmaf(ln_xhat_elem(v, mu, rs), g, b);
}
// s1 / s2: this lane's share of sum dy*g and sum dy*g*xhat; ag / ab: the dgamma / dbeta columns
__device__ __forceinline__ void ln_bwd_accum_elem(float dv, float xh, float g, float& s1, float& s2, float& ag, float& ab) {
  const float dgj = dv * g;
  s1 += dgj;
  s2 = fmaf(dgj, xh, s2);
  ag = fmaf(dv, xh, ag);
  ab += dv;
}
// dx = rstd * (dy*g - mean(dy*g) - xhat * mean(dy*g*xhat))
__device__ __forceinline__ float ln_bwd_dx_elem(float dv, float xh, float g, float rs, float c1, float c2) {
  return rs * fmaf(-xh, c2, dv * g - c1);
}
// the column sum of a stored gradient adds the value as stored (rounded to T)
template <typename T>
__device__ __forceinline__ void ln_bwd_colsum_elem(float o, float& ax) { ax += Elem<T>::round(o); }

// X2: the row is x + x2 (compile time: the plain LayerNorm then carries no registers for the second operand's two rows in
// flight -- 76 -> 64 VGPRs for 768 columns = 8 instead of 6 waves per SIMD, round 6)
// TB / TH (here and below): the element types of the branch x2 (and of its gradient) and of the normalised rows y (and of their
// gradient dy) where they differ from the stream's T -- the mixed family (lvl_layernorm_*_mixed: float32 stream, bf16 branch,
// bf16 normalised rows). Every operand is read and written in the type it has; the row arithmetic is the same f32 code.
template <typename T, int VPL, int W, bool X2, typename TB = T>
struct LnFwdRow {
  RawVec<T, W> x[VPL];
  RawVec<TB, W> x2[X2 ? VPL : 1];
  __device__ __forceinline__ void load(const T* __restrict__ px, const TB* __restrict__ px2, int64_t row, int cols,
                                       int lane, int nvec) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + i * 64;
      if (c < nvec) {
        x[i].load(px + row * cols + c * W);
        if constexpr (X2) x2[i].load(px2 + row * cols + c * W);
      }
    }
  }
};

// software-pipelined like the backward: the next row's packed operands are requested before this row is reduced
template <typename T, int VPL, int W, bool X2, typename TB = T, typename TH = T>
__global__ __launch_bounds__(256) void ln_fwd_kernel(
    const T* __restrict__ x, const TB* __restrict__ x2, const float* __restrict__ bias,
    const float* __restrict__ gamma, const float* __restrict__ beta, T* __restrict__ s_out,
    TH* __restrict__ out, float* __restrict__ mean, float* __restrict__ rstd, int64_t rows, int cols,
    float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nvec = cols / W;
  const float inv_cols = 1.0f / (float)cols;
  const int64_t stride = (int64_t)gridDim.x * kRowsPerBlock;
  int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + wave;
  LnFwdRow<T, VPL, W, X2, TB> cur, nxt;
  if (row < rows) cur.load(x, x2, row, cols, lane, nvec);
  for (; row < rows; row += stride) {
    if (row + stride < rows) nxt.load(x, x2, row + stride, cols, lane, nvec);
    float v[VPL][W];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + i * 64;
      if (c < nvec) {
        cur.x[i].unpack(v[i]);
        if constexpr (X2) {
          float w[W];
          cur.x2[i].unpack(w);
#pragma unroll
          for (int j = 0; j < W; ++j) v[i][j] += w[j];
        }
        if (bias != nullptr) {
          float bb[W];
          VecIO<float, W>::load(bias + c * W, bb);
#pragma unroll
          for (int j = 0; j < W; ++j) v[i][j] += bb[j];
        }
        if (s_out != nullptr) {
          // the sum is what downstream residuals read: round it once, then normalise the rounded value
          VecIO<T, W>::store(s_out + row * cols + c * W, v[i]);
#pragma unroll
          for (int j = 0; j < W; ++j) v[i][j] = Elem<T>::round(v[i][j]);
        }
#pragma unroll
        for (int j = 0; j < W; ++j) sum += v[i][j];
      }
    }
    const float mu = ln_mean(sum, inv_cols);
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      if (lane + i * 64 < nvec) {
#pragma unroll
        for (int j = 0; j < W; ++j) ln_sq_elem(v[i][j], mu, sq);
      }
    }
    const float rs = ln_rstd(sq, inv_cols, eps);
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + i * 64;
      if (c < nvec) {
        float g[W], b[W], o[W];
        VecIO<float, W>::load(gamma + c * W, g);
        VecIO<float, W>::load(beta + c * W, b);
#pragma unroll
        for (int j = 0; j < W; ++j) o[j] = ln_norm_elem(v[i][j], mu, rs, g[j], b[j]);
        VecIO<TH, W>::store(out + row * cols + c * W, o);
      }
    }
    if (lane == 0) {
      if (mean) mean[row] = mu;
      if (rstd) rstd[row] = rs;
    }
    cur = nxt;
  }
}

// EXACT-WIDTH forward (cols == VPL * 64 * W; s_out with SOUT only; round 6): ln_fwd_kernel with NO conditional vector-memory
// instruction in the row loop. Why it exists: the compiler's s_waitcnt insertion merges its counters conservatively over branches, and
// ln_fwd_kernel's per-chunk `c < nvec` / `row + stride < rows` / nullable-pointer branches
// left the row loop with `s_waitcnt vmcnt(0)` in front of the reductions (the prefetched NEXT row was waited for too) and
// behind each per-row reload of gamma / beta (three dependent L2 round trips per row). Here gamma, beta (and the optional
// bias) live in registers, the prefetch is unconditional (the last rows re-read row `rows - 1`), mean / rstd are stored by every
// lane (one address), and every wait the compiler places is a counted one: the next row's loads and this row's stores stay in
// flight across the reductions.
// The mixed forms are held to the waves per SIMD of the float32 instantiation they replace (the compiler's report, DESIGN.md
// section 4: the float32 exact forward without s_out, ln_fwd_kernel<float> with it); left alone the branch's unpacking costs
// the forms with a branch and no bias a wave or two. 1 = no demand, as for every same-type instantiation.
template <typename T, typename TB, int VPL, int W, bool X2, bool BIAS, bool SOUT>
constexpr int ln_fwd_exact_waves() {
  if (sizeof(T) == sizeof(TB) || W != 4 || !X2 || SOUT) return 1;
  return BIAS ? 1 : VPL == 4 ? 6 : 8;
}

template <typename T, int VPL, int W, bool X2, bool BIAS, typename TB = T, typename TH = T, bool SOUT = false>
__global__ __launch_bounds__(256, (ln_fwd_exact_waves<T, TB, VPL, W, X2, BIAS, SOUT>())) void ln_fwd_exact_kernel(
    const T* __restrict__ x, const TB* __restrict__ x2, const float* __restrict__ bias,
    const float* __restrict__ gamma, const float* __restrict__ beta, TH* __restrict__ out, float* __restrict__ mean,
    float* __restrict__ rstd, int64_t rows, float eps, T* __restrict__ s_out) {
  constexpr int cols = VPL * 64 * W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float inv_cols = 1.0f / (float)cols;
  const int64_t stride = (int64_t)gridDim.x * kRowsPerBlock;
  int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + wave;
  if (row >= rows) return;
  float g[VPL][W], b[VPL][W], bb[BIAS ? VPL : 1][W];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    VecIO<float, W>::load(gamma + (lane + i * 64) * W, g[i]);
    VecIO<float, W>::load(beta + (lane + i * 64) * W, b[i]);
    if constexpr (BIAS) VecIO<float, W>::load(bias + (lane + i * 64) * W, bb[i]);
  }
  RawVec<T, W> cur[VPL], nxt[VPL];
  RawVec<TB, W> cur2[X2 ? VPL : 1], nxt2[X2 ? VPL : 1];
  auto load_row = [&](int64_t r, RawVec<T, W> (&a)[VPL], RawVec<TB, W> (&a2)[X2 ? VPL : 1]) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      a[i].load(x + r * cols + (lane + i * 64) * W);
      if constexpr (X2) a2[i].load(x2 + r * cols + (lane + i * 64) * W);
    }
  };
  load_row(row, cur, cur2);
  // everything requested so far has landed before the loop is entered: the loop header then merges "nothing pending" with
  // the back edge's counted state instead of a conservative vmcnt(0) on every iteration
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    cur[i].pin();
    if constexpr (X2) cur2[i].pin();
#pragma unroll
    for (int j = 0; j < W; ++j) {
      asm volatile("" : "+v"(g[i][j]), "+v"(b[i][j]));
      if constexpr (BIAS) asm volatile("" : "+v"(bb[i][j]));
    }
  }
  for (; row < rows; row += stride) {
    load_row(row + stride < rows ? row + stride : rows - 1, nxt, nxt2);      // unconditional prefetch
    float v[VPL][W];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      cur[i].unpack(v[i]);
      if constexpr (X2) {
        float w[W];
        cur2[i].unpack(w);
#pragma unroll
        for (int j = 0; j < W; ++j) v[i][j] += w[j];
      }
      if constexpr (BIAS) {
#pragma unroll
        for (int j = 0; j < W; ++j) v[i][j] += bb[i][j];
      }
      if constexpr (SOUT) {          // as ln_fwd_kernel: the sum is stored, and normalised as stored
        VecIO<T, W>::store(s_out + row * cols + (lane + i * 64) * W, v[i]);
#pragma unroll
        for (int j = 0; j < W; ++j) v[i][j] = Elem<T>::round(v[i][j]);
      }
#pragma unroll
      for (int j = 0; j < W; ++j) sum += v[i][j];
    }
    const float mu = ln_mean(sum, inv_cols);
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i)
#pragma unroll
      for (int j = 0; j < W; ++j) ln_sq_elem(v[i][j], mu, sq);
    const float rs = ln_rstd(sq, inv_cols, eps);
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      float o[W];
#pragma unroll
      for (int j = 0; j < W; ++j) o[j] = ln_norm_elem(v[i][j], mu, rs, g[i][j], b[i][j]);
      VecIO<TH, W>::store(out + row * cols + (lane + i * 64) * W, o);
    }
    mean[row] = mu;          // every lane, one address: no exec-masked (conditional) store in the loop; both non-null here
    rstd[row] = rs;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      cur[i] = nxt[i];
      if constexpr (X2) cur2[i] = nxt2[i];
    }
  }
}

// APPLY: y = ln_norm_elem(x (+ x2) (+ bias), mean[row], rstd[row], gamma, beta) -- the forward's output rebuilt from the
// forward's operands and the statistics it stored (selective activation recompute: the normalised rows are not kept, the
// weight-gradient GEMM that reads them gets them back from here). No reductions; the input sum is formed in the forward's
// order and the element goes through the same ln_norm_elem, so the rows equal the forward's to the bit, whichever of
// the two forward kernels produced them and whichever of the two kernels below rebuilds them.
template <typename T, int VPL, int W, bool X2>
__global__ __launch_bounds__(256) void ln_apply_kernel(
    const T* __restrict__ x, const T* __restrict__ x2, const float* __restrict__ bias,
    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mean,
    const float* __restrict__ rstd, T* __restrict__ out, int64_t rows, int cols) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nvec = cols / W;
  const int64_t stride = (int64_t)gridDim.x * kRowsPerBlock;
  int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + wave;
  LnFwdRow<T, VPL, W, X2> cur, nxt;
  float mu = 0.f, rs = 0.f, mu_n = 0.f, rs_n = 0.f;
  if (row < rows) {
    cur.load(x, x2, row, cols, lane, nvec);
    mu = mean[row];
    rs = rstd[row];
  }
  for (; row < rows; row += stride) {
    if (row + stride < rows) {
      nxt.load(x, x2, row + stride, cols, lane, nvec);
      mu_n = mean[row + stride];
      rs_n = rstd[row + stride];
    }
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + i * 64;
      if (c < nvec) {
        float v[W], g[W], b[W], o[W];
        cur.x[i].unpack(v);
        if constexpr (X2) {
          float w[W];
          cur.x2[i].unpack(w);
#pragma unroll
          for (int j = 0; j < W; ++j) v[j] += w[j];
        }
        if (bias != nullptr) {
          float bb[W];
          VecIO<float, W>::load(bias + c * W, bb);
#pragma unroll
          for (int j = 0; j < W; ++j) v[j] += bb[j];
        }
        VecIO<float, W>::load(gamma + c * W, g);
        VecIO<float, W>::load(beta + c * W, b);
#pragma unroll
        for (int j = 0; j < W; ++j) o[j] = ln_norm_elem(v[j], mu, rs, g[j], b[j]);
        VecIO<T, W>::store(out + row * cols + c * W, o);
      }
    }
    cur = nxt;
    mu = mu_n;
    rs = rs_n;
  }
}

// EXACT-WIDTH apply (cols == VPL * 64 * W): as ln_fwd_exact_kernel, no conditional vector-memory instruction in the row loop --
// gamma, beta (and the optional bias) in registers, the next row and its mean / rstd prefetched unconditionally (the last
// rows re-read row `rows - 1`), so that the wait in front of a row's arithmetic is a counted one and the next row's loads
// and this row's stores stay in flight.
template <typename T, int VPL, int W, bool X2, bool BIAS>
__global__ __launch_bounds__(256) void ln_apply_exact_kernel(
    const T* __restrict__ x, const T* __restrict__ x2, const float* __restrict__ bias,
    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mean,
    const float* __restrict__ rstd, T* __restrict__ out, int64_t rows) {
  constexpr int cols = VPL * 64 * W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t stride = (int64_t)gridDim.x * kRowsPerBlock;
  int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + wave;
  if (row >= rows) return;
  float g[VPL][W], b[VPL][W], bb[BIAS ? VPL : 1][W];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    VecIO<float, W>::load(gamma + (lane + i * 64) * W, g[i]);
    VecIO<float, W>::load(beta + (lane + i * 64) * W, b[i]);
    if constexpr (BIAS) VecIO<float, W>::load(bias + (lane + i * 64) * W, bb[i]);
  }
  struct Row {
    RawVec<T, W> x[VPL], x2[X2 ? VPL : 1];
    float mu, rs;
  } cur, nxt;
  auto load_row = [&](int64_t r, Row& q) {
    q.mu = mean[r];
    q.rs = rstd[r];
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      q.x[i].load(x + r * cols + (lane + i * 64) * W);
      if constexpr (X2) q.x2[i].load(x2 + r * cols + (lane + i * 64) * W);
    }
  };
  load_row(row, cur);
  // everything requested so far has landed before the loop is entered (see ln_fwd_exact_kernel)
  asm volatile("" : "+v"(cur.mu), "+v"(cur.rs));
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    cur.x[i].pin();
    if constexpr (X2) cur.x2[i].pin();
#pragma unroll
    for (int j = 0; j < W; ++j) {
      asm volatile("" : "+v"(g[i][j]), "+v"(b[i][j]));
      if constexpr (BIAS) asm volatile("" : "+v"(bb[i][j]));
    }
  }
  for (; row < rows; row += stride) {
    load_row(row + stride < rows ? row + stride : rows - 1, nxt);      // unconditional prefetch
    const float mu = cur.mu, rs = cur.rs;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      float v[W], o[W];
      cur.x[i].unpack(v);
      if constexpr (X2) {
        float w[W];
        cur.x2[i].unpack(w);
#pragma unroll
        for (int j = 0; j < W; ++j) v[j] += w[j];
      }
      if constexpr (BIAS) {
#pragma unroll
        for (int j = 0; j < W; ++j) v[j] += bb[i][j];
      }
#pragma unroll
      for (int j = 0; j < W; ++j) o[j] = ln_norm_elem(v[j], mu, rs, g[i][j], b[i][j]);
      VecIO<T, W>::store(out + row * cols + (lane + i * 64) * W, o);
    }
    cur = nxt;
  }
}

// Backward: dx (+ dadd) and per-workgroup partial slabs [3][cols] = {sum dy*shat, sum dy, sum dx}.
// The row loop is software-pipelined: the packed operands of the NEXT row (and its mean/rstd) are requested before
// the current row is reduced, so each wave keeps two rows of loads in flight (4 waves/SIMD would otherwise leave
// HBM idle during the two cross-lane reductions).
template <typename T, int VPL, int W, typename TB = T, typename TH = T>
struct LnBwdRow {
  RawVec<TH, W> dy[VPL];
  RawVec<T, W> x[VPL];
  RawVec<TB, W> x2[VPL];
  RawVec<T, W> dadd[VPL];
  float mu, rs;
  __device__ __forceinline__ void load(const TH* __restrict__ pdy, const T* __restrict__ px,
                                       const TB* __restrict__ px2, const T* __restrict__ pdadd,
                                       const float* __restrict__ mean, const float* __restrict__ rstd, int64_t row,
                                       int cols, int lane, int nvec) {
    mu = mean[row];
    rs = rstd[row];
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + i * 64;
      if (c < nvec) {
        const int64_t off = row * cols + c * W;
        dy[i].load(pdy + off);
        x[i].load(px + off);
        if (px2 != nullptr) x2[i].load(px2 + off);
        if (pdadd != nullptr) dadd[i].load(pdadd + off);
      }
    }
  }
};

// the tail of both backward kernels: combine the 4 waves of a workgroup through LDS, then one partial slab per workgroup
template <int VPL, int W>
__device__ __forceinline__ void ln_bwd_combine(float* smem, float* __restrict__ part, float (&ag)[VPL][W], float (&ab)[VPL][W],
                                               float (&ax)[VPL][W], int cols, int nvec, int lane, int wave) {
  if (wave > 0) {
    float* dst = smem + (size_t)(wave - 1) * 3 * cols;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + i * 64;
      if (c < nvec) {
#pragma unroll
        for (int j = 0; j < W; ++j) {
          dst[c * W + j] = ag[i][j];
          dst[cols + c * W + j] = ab[i][j];
          dst[2 * cols + c * W + j] = ax[i][j];
        }
      }
    }
  }
  __syncthreads();
  if (wave == 0) {
    float* pg = part + (size_t)blockIdx.x * 3 * cols;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + i * 64;
      if (c < nvec) {
#pragma unroll
        for (int j = 0; j < W; ++j) {
          float a = ag[i][j], b = ab[i][j], e = ax[i][j];
          for (int w = 0; w < 3; ++w) {
            a += smem[(size_t)w * 3 * cols + c * W + j];
            b += smem[(size_t)w * 3 * cols + cols + c * W + j];
            e += smem[(size_t)w * 3 * cols + 2 * cols + c * W + j];
          }
          pg[c * W + j] = a;
          pg[cols + c * W + j] = b;
          pg[2 * cols + c * W + j] = e;
        }
      }
    }
  }
}

// Stochastic depth (lvl_droppath_add_layernorm_*): the sample of a row. The entries take rows < 2^32, so that this is one
// 32-bit division: straight-line code (a 64-bit division, or a choice between the two, would put a branch into the row loops)
__device__ __forceinline__ uint32_t dp_sample(int64_t row, int64_t rps) { return (uint32_t)row / (uint32_t)rps; }

// EXACT-WIDTH backward (cols == VPL * 64 * W; round 6): ln_bwd_kernel with no conditional vector-memory instruction in the
// row loop (see ln_fwd_exact_kernel: the general kernel's loop waits vmcnt(0) -- for the prefetched next row as well -- in
// front of every reduction). X2: the normalised row is x + x2 (+ bias, zeros when there is none); DADD: dx = dx_ln + dadd;
// PLAIN: dx_ln is stored to dx_plain as well. mean / rstd of the next row are prefetched with it.
// DY (stochastic depth, with neither X2 nor PLAIN): dy = scale[sample of the row] * dx is stored beside dx -- formed from
// dx AS STORED (rounded to T) and rounded once more, which is what the composed form (dp_dy_kernel on the stored dx) gives
// to the bit -- and the column sums are those of dy as stored instead of dx's. The row's scale is prefetched with the row.
// DUP (the mixed family, not with PLAIN): dx is stored to dx_plain as well, rounded once to the branch's type -- the branch
// gradient where the stream's gradient is dx itself.
template <typename T, int VPL, int W, bool X2, bool DADD, bool PLAIN, bool DY = false, typename TB = T, typename TH = T,
          bool DUP = false>
__global__ __launch_bounds__(256, (VPL * W <= 12 ? (sizeof(T) == 2 ? 3 : 2) : 1)) void ln_bwd_exact_kernel(
    const TH* __restrict__ dy, const T* __restrict__ x, const TB* __restrict__ x2,
    const float* __restrict__ bias, const float* __restrict__ gamma, const float* __restrict__ mean,
    const float* __restrict__ rstd, const T* __restrict__ dadd, T* __restrict__ dx, TB* __restrict__ dx_plain,
    float* __restrict__ part, int64_t rows, const float* __restrict__ scale, T* __restrict__ dy_out, int64_t rps) {
  static_assert(!DY || (!X2 && !PLAIN), "the dy output belongs to the kept-sum forms");
  static_assert(!DUP || (!PLAIN && !DY), "dx_plain holds one gradient");
  extern __shared__ __attribute__((aligned(16))) float smem[];   // [3 waves][3][cols]
  constexpr int cols = VPL * 64 * W, nvec = VPL * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float inv_cols = 1.0f / (float)cols;
  float g[VPL][W], ag[VPL][W], ab[VPL][W], ax[VPL][W], bb[X2 ? VPL : 1][W];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
#pragma unroll
    for (int j = 0; j < W; ++j) { ag[i][j] = 0.f; ab[i][j] = 0.f; ax[i][j] = 0.f; }
    VecIO<float, W>::load(gamma + (lane + i * 64) * W, g[i]);
    if constexpr (X2) {
#pragma unroll
      for (int j = 0; j < W; ++j) bb[i][j] = 0.f;
    }
  }
  if constexpr (X2) {
    if (bias != nullptr) {            // before the loop: a branch here costs nothing
#pragma unroll
      for (int i = 0; i < VPL; ++i) VecIO<float, W>::load(bias + (lane + i * 64) * W, bb[i]);
    }
  }
  const int64_t stride = (int64_t)gridDim.x * kRowsPerBlock;
  int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + wave;
  struct Row {
    RawVec<TH, W> dy[VPL];
    RawVec<T, W> x[VPL];
    RawVec<TB, W> x2[X2 ? VPL : 1];
    RawVec<T, W> dadd[DADD ? VPL : 1];
    float mu, rs, c;
  } cur, nxt;
  auto load_row = [&](int64_t r, Row& q) {
    q.mu = mean[r];
    q.rs = rstd[r];
    if constexpr (DY) q.c = scale[dp_sample(r, rps)];
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int64_t off = r * cols + (lane + i * 64) * W;
      q.dy[i].load(dy + off);
      q.x[i].load(x + off);
      if constexpr (X2) q.x2[i].load(x2 + off);
      if constexpr (DADD) q.dadd[i].load(dadd + off);
    }
  };
  if (row < rows) {
    load_row(row, cur);
    // everything requested so far has landed before the loop is entered (see ln_fwd_exact_kernel)
    asm volatile("" : "+v"(cur.mu), "+v"(cur.rs));
    if constexpr (DY) asm volatile("" : "+v"(cur.c));
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      cur.dy[i].pin();
      cur.x[i].pin();
      if constexpr (X2) cur.x2[i].pin();
      if constexpr (DADD) cur.dadd[i].pin();
#pragma unroll
      for (int j = 0; j < W; ++j) {
        asm volatile("" : "+v"(g[i][j]));
        if constexpr (X2) asm volatile("" : "+v"(bb[i][j]));
      }
    }
  }
  for (; row < rows; row += stride) {
    load_row(row + stride < rows ? row + stride : rows - 1, nxt);      // unconditional prefetch
    const float mu = cur.mu, rs = cur.rs;
    auto xhat = [&](int i, float (&xh)[W]) {
      cur.x[i].unpack(xh);
      if constexpr (X2) {
        float w[W];
        cur.x2[i].unpack(w);
#pragma unroll
        for (int j = 0; j < W; ++j) xh[j] = (xh[j] + w[j]) + bb[i][j];      // x, += x2, += bias as in every kernel
      }
#pragma unroll
      for (int j = 0; j < W; ++j) xh[j] = ln_xhat_elem(xh[j], mu, rs);
    };
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      float xh[W], dv[W];
      xhat(i, xh);
      cur.dy[i].unpack(dv);
#pragma unroll
      for (int j = 0; j < W; ++j) ln_bwd_accum_elem(dv[j], xh[j], g[i][j], s1, s2, ag[i][j], ab[i][j]);
    }
    const float c1 = ln_mean(s1, inv_cols), c2 = ln_mean(s2, inv_cols);
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      float xh[W], dv[W], o[W];
      xhat(i, xh);
      cur.dy[i].unpack(dv);
#pragma unroll
      for (int j = 0; j < W; ++j) o[j] = ln_bwd_dx_elem(dv[j], xh[j], g[i][j], rs, c1, c2);
      const int64_t off = row * cols + (lane + i * 64) * W;
      if constexpr (PLAIN) {           // the normalisation's own input gradient leaves separately, and is what is summed
#pragma unroll
        for (int j = 0; j < W; ++j) ln_bwd_colsum_elem<T>(o[j], ax[i][j]);
        VecIO<TB, W>::store(dx_plain + off, o);
      }
      if constexpr (DADD) {
        float e[W];
        cur.dadd[i].unpack(e);
#pragma unroll
        for (int j = 0; j < W; ++j) o[j] += e[j];
      }
      if constexpr (!PLAIN && !DY) {
#pragma unroll
        for (int j = 0; j < W; ++j) ln_bwd_colsum_elem<T>(o[j], ax[i][j]);
      }
      VecIO<T, W>::store(dx + off, o);
      if constexpr (DUP) VecIO<TB, W>::store(dx_plain + off, o);
      if constexpr (DY) {
        float d[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
          d[j] = cur.c * Elem<T>::round(o[j]);
          ln_bwd_colsum_elem<T>(d[j], ax[i][j]);
        }
        VecIO<T, W>::store(dy_out + off, d);
      }
    }
    cur = nxt;
  }
  ln_bwd_combine<VPL, W>(smem, part, ag, ab, ax, cols, nvec, lane, wave);
}

// DUP (the mixed family): dx_plain receives dx itself, rounded once to the branch's type, instead of the gradient without dadd
template <typename T, int VPL, int W, typename TB = T, typename TH = T, bool DUP = false>
__global__ __launch_bounds__(256, (VPL * W <= 12 ? (sizeof(T) == 2 ? 3 : 2) : 1)) void ln_bwd_kernel(
    const TH* __restrict__ dy, const T* __restrict__ x, const TB* __restrict__ x2,
    const float* __restrict__ bias, const float* __restrict__ gamma, const float* __restrict__ mean,
    const float* __restrict__ rstd, const T* __restrict__ dadd, T* __restrict__ dx, TB* __restrict__ dx_plain,
    float* __restrict__ part, int64_t rows, int cols) {
  extern __shared__ __attribute__((aligned(16))) float smem[];   // [3 waves][3][cols]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nvec = cols / W;
  const float inv_cols = 1.0f / (float)cols;
  float g[VPL][W], ag[VPL][W], ab[VPL][W], ax[VPL][W];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = lane + i * 64;
#pragma unroll
    for (int j = 0; j < W; ++j) { ag[i][j] = 0.f; ab[i][j] = 0.f; ax[i][j] = 0.f; g[i][j] = 0.f; }
    if (c < nvec) VecIO<float, W>::load(gamma + c * W, g[i]);
  }
  float bb[VPL][W];     // residual-branch bias (recompute variant only)
  if (bias != nullptr) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + i * 64;
#pragma unroll
      for (int j = 0; j < W; ++j) bb[i][j] = 0.f;
      if (c < nvec) VecIO<float, W>::load(bias + c * W, bb[i]);
    }
  }
  const int64_t stride = (int64_t)gridDim.x * kRowsPerBlock;
  int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + wave;
  LnBwdRow<T, VPL, W, TB, TH> cur, nxt;
  if (row < rows) cur.load(dy, x, x2, dadd, mean, rstd, row, cols, lane, nvec);
  for (; row < rows; row += stride) {
    if (row + stride < rows) nxt.load(dy, x, x2, dadd, mean, rstd, row + stride, cols, lane, nvec);
    const float mu = cur.mu, rs = cur.rs;
    // normalised input of vector i, rebuilt from the packed operands (cheaper than holding it across the reduction)
    auto xhat = [&](int i, float (&xh)[W]) {
      cur.x[i].unpack(xh);
      if (x2 != nullptr) {
        float w[W];
        cur.x2[i].unpack(w);
#pragma unroll
        for (int j = 0; j < W; ++j) xh[j] += w[j];
      }
      if (bias != nullptr) {
#pragma unroll
        for (int j = 0; j < W; ++j) xh[j] += bb[i][j];
      }
#pragma unroll
      for (int j = 0; j < W; ++j) xh[j] = ln_xhat_elem(xh[j], mu, rs);
    };
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      if (lane + i * 64 < nvec) {
        float xh[W], dv[W];
        xhat(i, xh);
        cur.dy[i].unpack(dv);
#pragma unroll
        for (int j = 0; j < W; ++j) ln_bwd_accum_elem(dv[j], xh[j], g[i][j], s1, s2, ag[i][j], ab[i][j]);
      }
    }
    const float c1 = ln_mean(s1, inv_cols), c2 = ln_mean(s2, inv_cols);
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + i * 64;
      if (c < nvec) {
        float xh[W], dv[W], o[W];
        xhat(i, xh);
        cur.dy[i].unpack(dv);
#pragma unroll
        for (int j = 0; j < W; ++j) o[j] = ln_bwd_dx_elem(dv[j], xh[j], g[i][j], rs, c1, c2);
        if (!DUP && dx_plain != nullptr) {
#pragma unroll
          for (int j = 0; j < W; ++j) ln_bwd_colsum_elem<T>(o[j], ax[i][j]);
          VecIO<TB, W>::store(dx_plain + row * cols + c * W, o);
        }
        if (dadd != nullptr) {
          float e[W];
          cur.dadd[i].unpack(e);
#pragma unroll
          for (int j = 0; j < W; ++j) o[j] += e[j];
        }
        if (DUP || dx_plain == nullptr) {
#pragma unroll
          for (int j = 0; j < W; ++j) ln_bwd_colsum_elem<T>(o[j], ax[i][j]);
        }
        VecIO<T, W>::store(dx + row * cols + c * W, o);
        if constexpr (DUP) VecIO<TB, W>::store(dx_plain + row * cols + c * W, o);
      }
    }
    cur = nxt;
  }
  ln_bwd_combine<VPL, W>(smem, part, ag, ab, ax, cols, nvec, lane, wave);
}

// STOCHASTIC DEPTH (lvl_droppath_add_layernorm_*): the row is s = res + c * (y + bias) with one c = scale[sample] per row.
constexpr int kDpDyParts = 768;           // partial column-sum slabs of the dy pass (one per workgroup)

// Forward: ln_fwd_kernel's two-operand form with the scaled sum, always keeping s. Per element v = fma(c, y, res), then
// v = fma(c, bias, v): with c = 1 both are the correctly rounded sums ln_fwd_kernel forms (x, += x2, += bias), with c = 0 both
// return res. s is rounded once when stored and the statistics are those of the rounded value, through the ln_*_elem helpers.
// EXACT (cols == VPL * 64 * W): no conditional vector-memory instruction in the row loop, as ln_fwd_exact_kernel -- gamma,
// beta and the bias in registers, everything requested before the loop pinned there. Both forms prefetch the next row (and its
// sample's scale) unconditionally (the last rows re-read row `rows - 1`) and store mean / rstd from every lane.
template <typename T, int VPL, int W, bool EXACT, bool BIAS>
__global__ __launch_bounds__(256) void dp_ln_fwd_kernel(
    const T* __restrict__ res, const T* __restrict__ y, const float* __restrict__ bias, const float* __restrict__ scale,
    const float* __restrict__ gamma, const float* __restrict__ beta, T* __restrict__ s_out, T* __restrict__ out,
    float* __restrict__ mean, float* __restrict__ rstd, int64_t rows, int64_t rps, int cols_rt, float eps) {
  const int cols = EXACT ? VPL * 64 * W : cols_rt;
  const int nvec = cols / W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float inv_cols = 1.0f / (float)cols;
  const int64_t stride = (int64_t)gridDim.x * kRowsPerBlock;
  int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + wave;
  if (row >= rows) return;
  auto on = [&](int i) { return EXACT || lane + i * 64 < nvec; };
  float g[EXACT ? VPL : 1][W], b[EXACT ? VPL : 1][W], bb[EXACT && BIAS ? VPL : 1][W];
  if constexpr (EXACT) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      VecIO<float, W>::load(gamma + (lane + i * 64) * W, g[i]);
      VecIO<float, W>::load(beta + (lane + i * 64) * W, b[i]);
      if constexpr (BIAS) VecIO<float, W>::load(bias + (lane + i * 64) * W, bb[i]);
    }
  }
  struct Row {
    RawVec<T, W> x[VPL], y[VPL];
    float c;
  } cur, nxt;
  auto load_row = [&](int64_t r, Row& q) {
    q.c = scale[dp_sample(r, rps)];
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      if (on(i)) {
        const int64_t off = r * cols + (lane + i * 64) * W;
        q.x[i].load(res + off);
        q.y[i].load(y + off);
      }
    }
  };
  load_row(row, cur);
  if constexpr (EXACT) {
    // everything requested so far has landed before the loop is entered (see ln_fwd_exact_kernel)
    asm volatile("" : "+v"(cur.c));
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      cur.x[i].pin();
      cur.y[i].pin();
#pragma unroll
      for (int j = 0; j < W; ++j) {
        asm volatile("" : "+v"(g[i][j]), "+v"(b[i][j]));
        if constexpr (BIAS) asm volatile("" : "+v"(bb[i][j]));
      }
    }
  }
  for (; row < rows; row += stride) {
    load_row(row + stride < rows ? row + stride : rows - 1, nxt);      // unconditional prefetch
    const float c = cur.c;
    float v[VPL][W];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      if (on(i)) {
        float w[W];
        cur.x[i].unpack(v[i]);
        cur.y[i].unpack(w);
#pragma unroll
        for (int j = 0; j < W; ++j) v[i][j] = fmaf(c, w[j], v[i][j]);
        if constexpr (BIAS) {
          if constexpr (EXACT) {
#pragma unroll
            for (int j = 0; j < W; ++j) v[i][j] = fmaf(c, bb[i][j], v[i][j]);
          } else {
            float bv[W];
            VecIO<float, W>::load(bias + (lane + i * 64) * W, bv);
#pragma unroll
            for (int j = 0; j < W; ++j) v[i][j] = fmaf(c, bv[j], v[i][j]);
          }
        }
        // the sum is what downstream residuals read: round it once, then normalise the rounded value
        VecIO<T, W>::store(s_out + row * cols + (lane + i * 64) * W, v[i]);
#pragma unroll
        for (int j = 0; j < W; ++j) v[i][j] = Elem<T>::round(v[i][j]);
#pragma unroll
        for (int j = 0; j < W; ++j) sum += v[i][j];
      }
    }
    const float mu = ln_mean(sum, inv_cols);
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      if (on(i)) {
#pragma unroll
        for (int j = 0; j < W; ++j) ln_sq_elem(v[i][j], mu, sq);
      }
    }
    const float rs = ln_rstd(sq, inv_cols, eps);
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      if (on(i)) {
        float o[W];
        if constexpr (EXACT) {
#pragma unroll
          for (int j = 0; j < W; ++j) o[j] = ln_norm_elem(v[i][j], mu, rs, g[i][j], b[i][j]);
        } else {
          float gv[W], bv[W];
          VecIO<float, W>::load(gamma + (lane + i * 64) * W, gv);
          VecIO<float, W>::load(beta + (lane + i * 64) * W, bv);
#pragma unroll
          for (int j = 0; j < W; ++j) o[j] = ln_norm_elem(v[i][j], mu, rs, gv[j], bv[j]);
        }
        VecIO<T, W>::store(out + row * cols + (lane + i * 64) * W, o);
      }
    }
    mean[row] = mu;          // every lane, one address
    rstd[row] = rs;
    cur = nxt;
  }
}

// Backward, composed form (float32, widths without an exact kernel), second pass (the first is lvl_layernorm_bwd on the kept
// sum): dy = c * ds from the stored ds, and one partial slab [cols] per workgroup of the column sums of dy as stored. One
// wave per row as above, so a row's c is one value per wave.
template <typename T, int VPL, int W, bool EXACT>
__global__ __launch_bounds__(256) void dp_dy_kernel(const T* __restrict__ ds, const float* __restrict__ scale,
                                                    T* __restrict__ dy, float* __restrict__ part, int64_t rows,
                                                    int64_t rps, int cols_rt) {
  extern __shared__ __attribute__((aligned(16))) float smem[];   // [3 waves][cols]
  const int cols = EXACT ? VPL * 64 * W : cols_rt;
  const int nvec = cols / W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  auto on = [&](int i) { return EXACT || lane + i * 64 < nvec; };
  float ax[VPL][W];
#pragma unroll
  for (int i = 0; i < VPL; ++i)
#pragma unroll
    for (int j = 0; j < W; ++j) ax[i][j] = 0.f;
  const int64_t stride = (int64_t)gridDim.x * kRowsPerBlock;
  int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + wave;
  struct Row {
    RawVec<T, W> d[VPL];
    float c;
  } cur, nxt;
  auto load_row = [&](int64_t r, Row& q) {
    q.c = scale[dp_sample(r, rps)];
#pragma unroll
    for (int i = 0; i < VPL; ++i)
      if (on(i)) q.d[i].load(ds + r * cols + (lane + i * 64) * W);
  };
  if (row < rows) load_row(row, cur);
  for (; row < rows; row += stride) {
    load_row(row + stride < rows ? row + stride : rows - 1, nxt);      // unconditional prefetch
    const float c = cur.c;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      if (on(i)) {
        float v[W], o[W];
        cur.d[i].unpack(v);
#pragma unroll
        for (int j = 0; j < W; ++j) {
          o[j] = c * v[j];
          ln_bwd_colsum_elem<T>(o[j], ax[i][j]);
        }
        VecIO<T, W>::store(dy + row * cols + (lane + i * 64) * W, o);
      }
    }
    cur = nxt;
  }
  if (wave > 0) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      if (on(i)) {
#pragma unroll
        for (int j = 0; j < W; ++j) smem[(size_t)(wave - 1) * cols + (lane + i * 64) * W + j] = ax[i][j];
      }
    }
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      if (on(i)) {
#pragma unroll
        for (int j = 0; j < W; ++j) {
          const int k = (lane + i * 64) * W + j;
          float a = ax[i][j];
          for (int w = 0; w < 3; ++w) a += smem[(size_t)w * cols + k];
          part[(size_t)blockIdx.x * cols + k] = a;
        }
      }
    }
  }
}

// Column sums of a partial slab part[nparts][width] (f32), deterministic, in two coalesced stages:
//   stage 1: grid (width/256, kColsumMid): a workgroup owns 256 columns (one 16-byte vector per lane = 1 KiB per row
//            per wave) and one of kColsumMid row chunks; its 4 waves take the chunk's rows round-robin with every load
//            issued before the first add, merge through LDS and write one row of mid[kColsumMid][width];
//   stage 2: 64 columns x 16 row groups per workgroup sum the kColsumMid rows of mid and scatter the result into up to
//            three `seg`-wide outputs.
// The whole slab (7-19 MB) is in flight at once in stage 1: two short launches (~4 + 3 us) instead of one
// latency chain of 8 dependent round trips per thread behind 144 workgroups (50 us, 99 calls per step in round 2).
constexpr int kColsumMid = 64;

__global__ __launch_bounds__(256) void colsum_stage1_kernel(const float* __restrict__ part, int nparts, int width,
                                                            float* __restrict__ mid) {
  __shared__ float4 red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 256 + lane * 4;
  const int rpc = (nparts + kColsumMid - 1) / kColsumMid;
  const int r0 = blockIdx.y * rpc, r1 = min(r0 + rpc, nparts);
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < width) {
    int p = r0 + wave;
    for (; p + 12 < r1; p += 16) {          // 4 rows in flight per wave
      const float4 v0 = *reinterpret_cast<const float4*>(part + (size_t)p * width + c);
      const float4 v1 = *reinterpret_cast<const float4*>(part + (size_t)(p + 4) * width + c);
      const float4 v2 = *reinterpret_cast<const float4*>(part + (size_t)(p + 8) * width + c);
      const float4 v3 = *reinterpret_cast<const float4*>(part + (size_t)(p + 12) * width + c);
      a.x += (v0.x + v1.x) + (v2.x + v3.x);
      a.y += (v0.y + v1.y) + (v2.y + v3.y);
      a.z += (v0.z + v1.z) + (v2.z + v3.z);
      a.w += (v0.w + v1.w) + (v2.w + v3.w);
    }
    for (; p < r1; p += 4) {
      const float4 v = *reinterpret_cast<const float4*>(part + (size_t)p * width + c);
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
  }
  red[wave][lane] = a;
  __syncthreads();
  if (wave == 0 && c < width) {
    const float4 b = red[1][lane], d = red[2][lane], e = red[3][lane];
    float4 o;
    o.x = (a.x + b.x) + (d.x + e.x);
    o.y = (a.y + b.y) + (d.y + e.y);
    o.z = (a.z + b.z) + (d.z + e.z);
    o.w = (a.w + b.w) + (d.w + e.w);
    *reinterpret_cast<float4*>(mid + (size_t)blockIdx.y * width + c) = o;
  }
}

// Tail (optional): zero_dst[0, tail_n) = 0 and copy_dst[0, tail_n) = copy_src[...] ride along (the k third of a qkv bias
// gradient is exactly 0 and its v third may arrive ready-made: no memset / copy launches beside the reduction).
__global__ __launch_bounds__(256) void colsum_stage2_kernel(const float* __restrict__ mid, int width, int seg,
                                                            float* __restrict__ out0, float* __restrict__ out1,
                                                            float* __restrict__ out2, float* __restrict__ zero_dst,
                                                            const float* __restrict__ copy_src,
                                                            float* __restrict__ copy_dst, int tail_n) {
  __shared__ float4 red[16][16];
  const int cg = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const int c = blockIdx.x * 64 + cg * 4;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < tail_n; i += gridDim.x * 256) {
    if (zero_dst) zero_dst[i] = 0.f;
    if (copy_dst) copy_dst[i] = copy_src[i];
  }
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < width) {
    float4 v[kColsumMid / 16];
#pragma unroll
    for (int i = 0; i < kColsumMid / 16; ++i) v[i] = *reinterpret_cast<const float4*>(mid + (size_t)(rg + 16 * i) * width + c);
#pragma unroll
    for (int i = 0; i < kColsumMid / 16; ++i) { a.x += v[i].x; a.y += v[i].y; a.z += v[i].z; a.w += v[i].w; }
  }
  red[rg][cg] = a;
  __syncthreads();
  if (rg == 0 && c < width) {
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float4 b = red[i][cg];
      o[0] += b.x; o[1] += b.y; o[2] += b.z; o[3] += b.w;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = c + e;
      const int sg = k / seg;
      float* dst = sg == 0 ? out0 : (sg == 1 ? out1 : out2);
      if (dst && k < width) dst[k - sg * seg] = o[e];
    }
  }
}

// (VPL, W) for a row length: W = 4 with exactly cols/256 vectors per lane when possible
constexpr int ln_w(int cols) { return cols % 256 == 0 && cols <= 1024 ? 4 : 8; }
constexpr int ln_vpl(int cols) { return ln_w(cols) == 4 ? cols / 256 : (cols / 8 <= 128 ? 2 : (cols / 8 <= 256 ? 4 : 8)); }
#define LN_CASE(CALL, VPL, W) case (W) * 16 + (VPL): CALL(VPL, W); break
#define LN_DISPATCH(cols, CALL)                                                           \
  switch (ln_w(cols) * 16 + ln_vpl(cols)) {                                               \
    LN_CASE(CALL, 1, 4); LN_CASE(CALL, 2, 4); LN_CASE(CALL, 3, 4); LN_CASE(CALL, 4, 4);   \
    LN_CASE(CALL, 2, 8); LN_CASE(CALL, 4, 8); LN_CASE(CALL, 8, 8);                        \
    default: return lvl_fail(LVL_EINVAL, "layernorm: no kernel for cols=%d", (int)(cols));  \
  }

// Is there an exact-width kernel for (T, VPL, W)? Where LN_DISPATCH picks (VPL, W) for the width VPL * 64 * W itself (1024
// columns go to (4, 4), never to (2, 8)); in the backward for the 2-byte type of the training step only. The launch code asks
// this with `if constexpr`: what is compiled is what can be chosen.
template <typename T, int VPL, int W>
constexpr bool ln_has_exact(bool backward) {
  return ln_vpl(VPL * 64 * W) == VPL && ln_w(VPL * 64 * W) == W && (!backward || sizeof(T) == 2);
}

// LAVILA_LN_EXACT=0 sends every call to the general kernels (the bit-for-bit test compares the two families through it)
bool ln_exact_enabled() {
  static const bool on = !(getenv("LAVILA_LN_EXACT") && atoi(getenv("LAVILA_LN_EXACT")) == 0);
  return on;
}

// one workgroup of 256 threads per kRowsPerBlock rows; more than 64 KiB of dynamic LDS needs the limit raised first
template <auto Kernel, typename... Args>
int ln_launch(int64_t blocks, size_t shmem, hipStream_t st, Args... args) {
  if (shmem > 64 * 1024)
    if (int rc = lvl_allow_lds<Kernel>()) return rc;
  hipLaunchKernelGGL(Kernel, dim3((unsigned)blocks), dim3(256), shmem, st, args...);
  return LVL_OK;
}

// The exact-width kernel where there is one for the operands of this call (in the backward: the operand combinations of the
// training step), the general kernel otherwise.
template <typename T, int VPL, int W>
int ln_fwd_launch(const T* x, const T* x2, const float* bias, const float* gamma, const float* beta, T* s_out, T* y,
                  float* mean, float* rstd, int64_t rows, int cols, float eps, int64_t blocks, hipStream_t st) {
#define LN_E(X2, BIAS) \
  ln_launch<ln_fwd_exact_kernel<T, VPL, W, X2, BIAS>>(blocks, 0, st, x, x2, bias, gamma, beta, y, mean, rstd, rows, eps, \
                                                      (T*)nullptr)
#define LN_G(X2) \
  ln_launch<ln_fwd_kernel<T, VPL, W, X2>>(blocks, 0, st, x, x2, bias, gamma, beta, s_out, y, mean, rstd, rows, cols, eps)
  if constexpr (ln_has_exact<T, VPL, W>(false)) {
    if (ln_exact_enabled() && cols == VPL * 64 * W && !s_out && mean && rstd && (x2 || !bias))
      return !x2 ? LN_E(false, false) : (bias ? LN_E(true, true) : LN_E(true, false));
  }
  return x2 ? LN_G(true) : LN_G(false);
#undef LN_G
#undef LN_E
}

template <typename T, int VPL, int W>
int ln_apply_launch(const T* x, const T* x2, const float* bias, const float* gamma, const float* beta, const float* mean,
                    const float* rstd, T* y, int64_t rows, int cols, int64_t blocks, hipStream_t st) {
#define LN_E(X2, BIAS) \
  ln_launch<ln_apply_exact_kernel<T, VPL, W, X2, BIAS>>(blocks, 0, st, x, x2, bias, gamma, beta, mean, rstd, y, rows)
#define LN_G(X2) ln_launch<ln_apply_kernel<T, VPL, W, X2>>(blocks, 0, st, x, x2, bias, gamma, beta, mean, rstd, y, rows, cols)
  if constexpr (ln_has_exact<T, VPL, W>(false)) {
    if (ln_exact_enabled() && cols == VPL * 64 * W && (x2 || !bias))
      return !x2 ? LN_E(false, false) : (bias ? LN_E(true, true) : LN_E(true, false));
  }
  return x2 ? LN_G(true) : LN_G(false);
#undef LN_G
#undef LN_E
}

template <typename T, int VPL, int W>
int ln_bwd_launch(const T* dy, const T* x, const T* x2, const float* bias, const float* gamma, const float* mean,
                  const float* rstd, const T* dadd, T* dx, T* dx_plain, float* ws, int64_t rows, int cols, int64_t blocks,
                  hipStream_t st) {
  const size_t shmem = (size_t)3 * 3 * cols * sizeof(float);
#define LN_ARGS blocks, shmem, st, dy, x, x2, bias, gamma, mean, rstd, dadd, dx, dx_plain, ws, rows
#define LN_E(X2, DADD, PLAIN) \
  ln_launch<ln_bwd_exact_kernel<T, VPL, W, X2, DADD, PLAIN>>(LN_ARGS, (const float*)nullptr, (T*)nullptr, (int64_t)1)
  if constexpr (ln_has_exact<T, VPL, W>(true)) {
    if (ln_exact_enabled() && cols == VPL * 64 * W && rows > 0) {
      if (!x2 && !bias && !dx_plain) return dadd ? LN_E(false, true, false) : LN_E(false, false, false);
      if (x2 && !dadd && !dx_plain) return LN_E(true, false, false);
      if (x2 && dadd && dx_plain) return LN_E(true, true, true);
    }
  }
  return ln_launch<ln_bwd_kernel<T, VPL, W>>(LN_ARGS, cols);
#undef LN_E
#undef LN_ARGS
}

// THE MIXED FAMILY (lvl_layernorm_*_mixed): the float32 residual stream under autocast. T = float for x, s_out, dadd and dx;
// bf16 for the branch x2 and its gradient dx2, for the normalised rows y and for their gradient dy. The kernels are the ones
// above with TB = TH = bf16_t: the lane layout (VPL, W) is the float32 instantiation's, so every sum is formed in its order.
// An exact-width form is built for 256-1024 columns (W = 4) where the compiler's resource report gives it, without scratch, the
// waves per SIMD of the float32 instantiation it replaces (profiles/ln_mixed_resource_usage_after.txt): the
// float32 exact forward of the same operands, ln_fwd_kernel<float> where the sum is kept, and in the backward -- float32 has no
// exact backward -- ln_bwd_kernel<float>. One form misses that: 768 columns with branch and bias and no kept sum (7 waves only
// with scratch); it takes the general kernel.
template <int VPL, int W>
constexpr bool ln_mixed_exact() { return W == 4 && ln_has_exact<float, VPL, W>(false); }
template <int VPL, int W, bool X2, bool BIAS, bool SOUT>
constexpr bool ln_mixed_fwd_exact() { return ln_mixed_exact<VPL, W>() && !(VPL == 3 && X2 && BIAS && !SOUT); }

template <int VPL, int W, bool X2, bool BIAS, bool SOUT>
int ln_fwd_mixed_form(const float* x, const bf16_t* x2, const float* bias, const float* gamma, const float* beta,
                      float* s_out, bf16_t* y, float* mean, float* rstd, int64_t rows, int cols, float eps, int64_t blocks,
                      bool general, hipStream_t st) {
  if constexpr (ln_mixed_fwd_exact<VPL, W, X2, BIAS, SOUT>()) {
    if (!general && ln_exact_enabled() && cols == VPL * 64 * W && mean && rstd)
      return ln_launch<ln_fwd_exact_kernel<float, VPL, W, X2, BIAS, bf16_t, bf16_t, SOUT>>(
          blocks, 0, st, x, x2, bias, gamma, beta, y, mean, rstd, rows, eps, s_out);
  }
  return ln_launch<ln_fwd_kernel<float, VPL, W, X2, bf16_t, bf16_t>>(blocks, 0, st, x, x2, bias, gamma, beta, s_out, y, mean,
                                                                     rstd, rows, cols, eps);
}

template <int VPL, int W>
int ln_fwd_mixed_launch(const float* x, const bf16_t* x2, const float* bias, const float* gamma, const float* beta,
                        float* s_out, bf16_t* y, float* mean, float* rstd, int64_t rows, int cols, float eps,
                        int64_t blocks, bool general, hipStream_t st) {
#define LN_F(X2, BIAS, SOUT, GENERAL)                                                                                 \
  ln_fwd_mixed_form<VPL, W, X2, BIAS, SOUT>(x, x2, bias, gamma, beta, s_out, y, mean, rstd, rows, cols, eps, blocks, GENERAL, st)
  if (!x2) return LN_F(false, false, false, general || bias || s_out);      // the exact plain form has neither
  if (s_out) return bias ? LN_F(true, true, true, general) : LN_F(true, false, true, general);
  return bias ? LN_F(true, true, false, general) : LN_F(true, false, false, general);
#undef LN_F
}

// dx2 with `plain`: the gradient without dadd (ln_bwd_kernel's dx_plain); without: dx itself (DUP). The exact-width kernel for
// the operand combinations of the training step, the general kernel otherwise.
template <int VPL, int W>
int ln_bwd_mixed_launch(const bf16_t* dy, const float* x, const bf16_t* x2, const float* bias, const float* gamma,
                        const float* mean, const float* rstd, const float* dadd, float* dx, bf16_t* dx2, float* ws,
                        int64_t rows, int cols, int64_t blocks, bool plain, bool general, hipStream_t st) {
  const size_t shmem = (size_t)3 * 3 * cols * sizeof(float);
#define LN_ARGS blocks, shmem, st, dy, x, x2, bias, gamma, mean, rstd, dadd, dx, dx2, ws, rows
#define LN_E(X2, DADD, PLAIN, DUP)                                                                  \
  ln_launch<ln_bwd_exact_kernel<float, VPL, W, X2, DADD, PLAIN, false, bf16_t, bf16_t, DUP>>(       \
      LN_ARGS, (const float*)nullptr, (float*)nullptr, (int64_t)1)
  if constexpr (ln_mixed_exact<VPL, W>()) {
    if (!general && ln_exact_enabled() && cols == VPL * 64 * W && rows > 0) {
      if (!x2 && !bias && !dadd && !dx2) return LN_E(false, false, false, false);
      if (!x2 && !bias && dx2 && !plain) return dadd ? LN_E(false, true, false, true) : LN_E(false, false, false, true);
      if (x2 && !dadd && dx2 && !plain) return LN_E(true, false, false, true);
      if (x2 && dadd && dx2 && plain) return LN_E(true, true, true, false);
    }
  }
  if (dx2 && !plain) return ln_launch<ln_bwd_kernel<float, VPL, W, bf16_t, bf16_t, true>>(LN_ARGS, cols);
  return ln_launch<ln_bwd_kernel<float, VPL, W, bf16_t, bf16_t>>(LN_ARGS, cols);
#undef LN_E
#undef LN_ARGS
}

}  // namespace

int lvl_ln_bwd_parts() { return kLnBwdParts; }

int lvl_colsum_mid_rows() { return kColsumMid; }

// out0/out1/out2 receive consecutive `seg`-wide segments of the column sums of part[nparts][width] (width % 4 == 0);
// mid: kColsumMid * width floats of scratch (the callers place it behind their partial slab)
int lvl_launch_column_reduce_tail(const float* part, int nparts, int width, int seg, float* mid, float* out0, float* out1,
                                  float* out2, float* zero_dst, const float* copy_src, float* copy_dst, int tail_n,
                                  hipStream_t st) {
  hipLaunchKernelGGL(colsum_stage1_kernel, dim3((width + 255) / 256, kColsumMid), dim3(256), 0, st, part, nparts, width,
                     mid);
  hipLaunchKernelGGL(colsum_stage2_kernel, dim3((width + 63) / 64), dim3(256), 0, st, mid, width, seg, out0, out1, out2,
                     zero_dst, copy_src, copy_dst, (zero_dst || copy_dst) ? tail_n : 0);
  LVL_CHECK_LAUNCH("column_reduce");
  return LVL_OK;
}

int lvl_launch_column_reduce(const float* part, int nparts, int width, int seg, float* mid, float* out0, float* out1,
                             float* out2, hipStream_t st) {
  return lvl_launch_column_reduce_tail(part, nparts, width, seg, mid, out0, out1, out2, nullptr, nullptr, nullptr, 0, st);
}

// workgroups of a forward launch (lvl_layernorm_fwd and lvl_layernorm_fwd_mixed, whose forms take the registers of their
// float32 instantiation or fewer)
static int64_t ln_fwd_blocks(int64_t rows, const void* x2) {
  const int64_t blocks = (rows + kRowsPerBlock - 1) / kRowsPerBlock;
  // long per-wave row chains: 2 x the resident workgroups at 6 waves/SIMD for the two-operand form (76 VGPRs); the plain form
  // (56 VGPRs, 8 waves/SIMD) measured best with 4 x its resident workgroups (0.136 ms at 8192 against 0.142 at 3072 and 0.176
  // at 2048 for 200 960 rows of 768: profiles/r06_rowops_ln_fwd.txt)
  const int64_t cap = x2 == nullptr ? 8192 : 3072;
  return blocks > cap ? cap : blocks;
}

extern "C" int lvl_layernorm_fwd(const void* x, const void* x2, const float* xbias, const float* gamma,
                                 const float* beta, void* s_out, void* y, float* mean, float* rstd, int64_t rows,
                                 int cols, float eps, int dtype, void* stream) {
  LVL_REQUIRE(rows == 0 || (x && gamma && beta && y), "layernorm_fwd: null pointer");
  LVL_REQUIRE(rows >= 0 && cols > 0 && cols % 8 == 0 && cols <= 4096,
              "layernorm_fwd: cols=%d must be a multiple of 8, <= 4096", cols);
  LVL_REQUIRE(lvl_aligned16(x) && lvl_aligned16(x2) && lvl_aligned16(xbias) && lvl_aligned16(y) &&
                  lvl_aligned16(s_out) && lvl_aligned16(gamma) && lvl_aligned16(beta),
              "layernorm_fwd: pointers must be 16-byte aligned");
  if (rows == 0) return LVL_OK;
  const int64_t blocks = ln_fwd_blocks(rows, x2);
#define LN_FWD(VPL, W)                                                                                               \
  if (int rc = ln_fwd_launch<T, VPL, W>((const T*)x, (const T*)x2, xbias, gamma, beta, (T*)s_out, (T*)y, mean, rstd, rows, \
                                        cols, eps, blocks, (hipStream_t)stream))                                       \
  return rc
  LVL_DISPATCH_DTYPE(dtype, LN_DISPATCH(cols, LN_FWD));
#undef LN_FWD
  LVL_CHECK_LAUNCH("layernorm_fwd");
  return LVL_OK;
}

extern "C" int lvl_layernorm_apply(const void* x, const void* x2, const float* xbias, const float* gamma,
                                   const float* beta, const float* mean, const float* rstd, void* y, int64_t rows,
                                   int cols, int dtype, void* stream) {
  LVL_REQUIRE(rows == 0 || (x && gamma && beta && mean && rstd && y), "layernorm_apply: null pointer");
  LVL_REQUIRE(rows >= 0 && cols > 0 && cols % 8 == 0 && cols <= 4096,
              "layernorm_apply: cols=%d must be a multiple of 8, <= 4096", cols);
  LVL_REQUIRE(lvl_aligned16(x) && lvl_aligned16(x2) && lvl_aligned16(xbias) && lvl_aligned16(y) &&
                  lvl_aligned16(gamma) && lvl_aligned16(beta),
              "layernorm_apply: pointers must be 16-byte aligned");
  if (rows == 0) return LVL_OK;
  int64_t blocks = (rows + kRowsPerBlock - 1) / kRowsPerBlock;
  // the forward's grids (same rows in flight per wave, fewer registers than the forward in either form)
  const int64_t apply_cap = x2 != nullptr ? 3072 : 8192;
  if (blocks > apply_cap) blocks = apply_cap;
#define LN_APPLY(VPL, W)                                                                                              \
  if (int rc = ln_apply_launch<T, VPL, W>((const T*)x, (const T*)x2, xbias, gamma, beta, mean, rstd, (T*)y, rows, cols, \
                                          blocks, (hipStream_t)stream))                                                \
  return rc
  LVL_DISPATCH_DTYPE(dtype, LN_DISPATCH(cols, LN_APPLY));
#undef LN_APPLY
  LVL_CHECK_LAUNCH("layernorm_apply");
  return LVL_OK;
}

extern "C" int lvl_layernorm_bwd(const void* dy, const void* x, const void* x2, const float* xbias,
                                 const float* gamma, const float* mean, const float* rstd, const void* dadd,
                                 void* dx, void* dx_plain, float* dgamma, float* dbeta, float* dxsum, float* ws,
                                 int64_t rows, int cols, int dtype, void* stream) {
  LVL_REQUIRE((rows == 0 || (dy && x && mean && rstd && dx)) && gamma && ws, "layernorm_bwd: null pointer");
  LVL_REQUIRE(rows >= 0 && cols > 0 && cols % 8 == 0 && cols <= 4096,
              "layernorm_bwd: cols=%d must be a multiple of 8, <= 4096", cols);
  LVL_REQUIRE(lvl_aligned16(dy) && lvl_aligned16(x) && lvl_aligned16(x2) && lvl_aligned16(xbias) &&
                  lvl_aligned16(dadd) && lvl_aligned16(dx) && lvl_aligned16(dx_plain) && lvl_aligned16(gamma),
              "layernorm_bwd: pointers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int64_t blocks = (rows + kRowsPerBlock - 1) / kRowsPerBlock;
  if (blocks > kLnBwdParts) blocks = kLnBwdParts;
  if (blocks < 1) blocks = 1;
#define LN_BWD(VPL, W)                                                                                               \
  if (int rc = ln_bwd_launch<T, VPL, W>((const T*)dy, (const T*)x, (const T*)x2, xbias, gamma, mean, rstd, (const T*)dadd, \
                                        (T*)dx, (T*)dx_plain, ws, rows, cols, blocks, st))                             \
  return rc
  LVL_DISPATCH_DTYPE(dtype, LN_DISPATCH(cols, LN_BWD));
#undef LN_BWD
  LVL_CHECK_LAUNCH("layernorm_bwd");
  return lvl_launch_column_reduce(ws, (int)blocks, 3 * cols, cols, ws + (size_t)kLnBwdParts * 3 * cols, dgamma, dbeta,
                                  dxsum, st);
}

extern "C" int lvl_layernorm_fwd_mixed(const float* x, const void* x2, const float* xbias, const float* gamma,
                                       const float* beta, float* s_out, void* y, float* mean, float* rstd, int64_t rows,
                                       int cols, float eps, int flags, void* stream) {
  LVL_REQUIRE(rows == 0 || (x && gamma && beta && y), "layernorm_fwd_mixed: null pointer");
  LVL_REQUIRE(rows >= 0 && cols > 0 && cols % 8 == 0 && cols <= 4096,
              "layernorm_fwd_mixed: cols=%d must be a multiple of 8, <= 4096", cols);
  LVL_REQUIRE((flags & ~LVL_LN_GENERAL) == 0, "layernorm_fwd_mixed: unknown flags %d", flags);
  LVL_REQUIRE(lvl_aligned16(x) && lvl_aligned16(x2) && lvl_aligned16(xbias) && lvl_aligned16(y) &&
                  lvl_aligned16(s_out) && lvl_aligned16(gamma) && lvl_aligned16(beta),
              "layernorm_fwd_mixed: pointers must be 16-byte aligned");
  if (rows == 0) return LVL_OK;
  const int64_t blocks = ln_fwd_blocks(rows, x2);
#define LN_FWD(VPL, W)                                                                                                  \
  if (int rc = ln_fwd_mixed_launch<VPL, W>(x, (const bf16_t*)x2, xbias, gamma, beta, s_out, (bf16_t*)y, mean, rstd, rows, \
                                           cols, eps, blocks, (flags & LVL_LN_GENERAL) != 0, (hipStream_t)stream))        \
  return rc
  LN_DISPATCH(cols, LN_FWD);
#undef LN_FWD
  LVL_CHECK_LAUNCH("layernorm_fwd_mixed");
  return LVL_OK;
}

extern "C" int lvl_layernorm_bwd_mixed(const void* dy, const float* x, const void* x2, const float* xbias,
                                       const float* gamma, const float* mean, const float* rstd, const float* dadd,
                                       float* dx, void* dx2, float* dgamma, float* dbeta, float* dxsum, float* ws,
                                       int64_t rows, int cols, int flags, void* stream) {
  LVL_REQUIRE((rows == 0 || (dy && x && mean && rstd && dx)) && gamma && ws, "layernorm_bwd_mixed: null pointer");
  LVL_REQUIRE(rows >= 0 && cols > 0 && cols % 8 == 0 && cols <= 4096,
              "layernorm_bwd_mixed: cols=%d must be a multiple of 8, <= 4096", cols);
  LVL_REQUIRE((flags & ~(LVL_LN_GENERAL | LVL_LN_PLAIN)) == 0, "layernorm_bwd_mixed: unknown flags %d", flags);
  LVL_REQUIRE(!(flags & LVL_LN_PLAIN) || rows == 0 || dx2, "layernorm_bwd_mixed: LVL_LN_PLAIN needs dx2");
  LVL_REQUIRE(lvl_aligned16(dy) && lvl_aligned16(x) && lvl_aligned16(x2) && lvl_aligned16(xbias) &&
                  lvl_aligned16(dadd) && lvl_aligned16(dx) && lvl_aligned16(dx2) && lvl_aligned16(gamma),
              "layernorm_bwd_mixed: pointers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int64_t blocks = (rows + kRowsPerBlock - 1) / kRowsPerBlock;
  if (blocks > kLnBwdParts) blocks = kLnBwdParts;
  if (blocks < 1) blocks = 1;
#define LN_BWD(VPL, W)                                                                                                  \
  if (int rc = ln_bwd_mixed_launch<VPL, W>((const bf16_t*)dy, x, (const bf16_t*)x2, xbias, gamma, mean, rstd, dadd, dx,   \
                                           (bf16_t*)dx2, ws, rows, cols, blocks, (flags & LVL_LN_PLAIN) != 0,             \
                                           (flags & LVL_LN_GENERAL) != 0, st))                                            \
  return rc
  LN_DISPATCH(cols, LN_BWD);
#undef LN_BWD
  LVL_CHECK_LAUNCH("layernorm_bwd_mixed");
  return lvl_launch_column_reduce(ws, (int)blocks, 3 * cols, cols, ws + (size_t)kLnBwdParts * 3 * cols, dgamma, dbeta,
                                  dxsum, st);
}

namespace {

template <typename T, int VPL, int W>
int dp_ln_fwd_launch(const T* res, const T* y, const float* bias, const float* scale, const float* gamma, const float* beta,
                     T* s_out, T* out, float* mean, float* rstd, int64_t rows, int64_t rps, int cols, float eps,
                     int64_t blocks, hipStream_t st) {
#define DP_F(EXACT, BIAS)                                                                                               \
  ln_launch<dp_ln_fwd_kernel<T, VPL, W, EXACT, BIAS>>(blocks, 0, st, res, y, bias, scale, gamma, beta, s_out, out, mean, \
                                                      rstd, rows, rps, cols, eps)
  if constexpr (ln_has_exact<T, VPL, W>(false)) {
    if (ln_exact_enabled() && cols == VPL * 64 * W) return bias ? DP_F(true, true) : DP_F(true, false);
  }
  return bias ? DP_F(false, true) : DP_F(false, false);
#undef DP_F
}

// Where the DY instantiation keeps the waves per SIMD of the instantiation it extends and does not spill (compiler report,
// DESIGN.md section 4): 768 and 2048 columns, and 1024 columns with dadd. 256 columns with dadd and 512 columns lose a wave,
// 1024 columns without dadd drop from 4 to 3, 4096 columns spill: those take the composed form.
template <int VPL, int W, bool DADD>
constexpr bool dp_fused_ok() { return (VPL == 3 && W == 4) || (VPL == 4 && W == 8) || (VPL == 4 && W == 4 && DADD); }

// The fused backward where there is an exact-width kernel (bf16): ln_bwd_exact_kernel<..., DY = true>; *fused tells.
template <typename T, int VPL, int W, bool DADD>
int dp_bwd_fused_launch(const T* dh, const T* s, const float* gamma, const float* mean, const float* rstd, const float* scale,
                        const T* dadd, T* ds, T* dy, float* ws, int64_t rows, int64_t rps, int cols, int64_t blocks,
                        hipStream_t st, bool* fused) {
  *fused = false;
  if constexpr (ln_has_exact<T, VPL, W>(true) && dp_fused_ok<VPL, W, DADD>()) {
    if (ln_exact_enabled() && cols == VPL * 64 * W && rows > 0) {
      *fused = true;
      const size_t shmem = (size_t)3 * 3 * cols * sizeof(float);
      return ln_launch<ln_bwd_exact_kernel<T, VPL, W, false, DADD, false, true>>(
          blocks, shmem, st, dh, s, (const T*)nullptr, (const float*)nullptr, gamma, mean, rstd, dadd, ds, (T*)nullptr, ws,
          rows, scale, dy, rps);
    }
  }
  return LVL_OK;
}

template <typename T, int VPL, int W>
int dp_dy_launch(const T* ds, const float* scale, T* dy, float* part, int64_t rows, int64_t rps, int cols, int64_t blocks,
                 hipStream_t st) {
  const size_t shmem = (size_t)3 * cols * sizeof(float);
  if constexpr (ln_has_exact<T, VPL, W>(false)) {
    if (ln_exact_enabled() && cols == VPL * 64 * W)
      return ln_launch<dp_dy_kernel<T, VPL, W, true>>(blocks, shmem, st, ds, scale, dy, part, rows, rps, cols);
  }
  return ln_launch<dp_dy_kernel<T, VPL, W, false>>(blocks, shmem, st, ds, scale, dy, part, rows, rps, cols);
}

}  // namespace

int lvl_dp_dy_parts() { return kDpDyParts; }

extern "C" int lvl_droppath_add_layernorm_fwd(const void* res, const void* y, const float* ybias, const float* scale,
                                              const float* gamma, const float* beta, void* s_out, void* h_out,
                                              float* mean, float* rstd, int64_t rows, int64_t rows_per_sample, int cols,
                                              float eps, int dtype, void* stream) {
  LVL_REQUIRE(rows == 0 || (res && y && scale && gamma && beta && s_out && h_out && mean && rstd),
              "droppath_add_layernorm_fwd: null pointer");
  LVL_REQUIRE(rows >= 0 && cols > 0 && cols % 8 == 0 && cols <= 4096,
              "droppath_add_layernorm_fwd: cols=%d must be a multiple of 8, <= 4096", cols);
  LVL_REQUIRE(rows_per_sample > 0 && rows % rows_per_sample == 0,
              "droppath_add_layernorm_fwd: rows=%lld must be a multiple of rows_per_sample=%lld", (long long)rows,
              (long long)rows_per_sample);
  LVL_REQUIRE(rows < ((int64_t)1 << 32), "droppath_add_layernorm_fwd: rows=%lld must be below 2^32", (long long)rows);
  LVL_REQUIRE(lvl_aligned16(res) && lvl_aligned16(y) && lvl_aligned16(ybias) && lvl_aligned16(s_out) &&
                  lvl_aligned16(h_out) && lvl_aligned16(gamma) && lvl_aligned16(beta),
              "droppath_add_layernorm_fwd: pointers must be 16-byte aligned");
  if (rows == 0) return LVL_OK;
  int64_t blocks = (rows + kRowsPerBlock - 1) / kRowsPerBlock;
  if (blocks > 3072) blocks = 3072;       // the grid of lvl_layernorm_fwd's two-operand form
#define DP_FWD(VPL, W)                                                                                                  \
  if (int rc = dp_ln_fwd_launch<T, VPL, W>((const T*)res, (const T*)y, ybias, scale, gamma, beta, (T*)s_out, (T*)h_out,   \
                                           mean, rstd, rows, rows_per_sample, cols, eps, blocks, (hipStream_t)stream))    \
  return rc
  LVL_DISPATCH_DTYPE(dtype, LN_DISPATCH(cols, DP_FWD));
#undef DP_FWD
  LVL_CHECK_LAUNCH("droppath_add_layernorm_fwd");
  return LVL_OK;
}

extern "C" int lvl_droppath_add_layernorm_bwd(const void* dh, const void* s, const float* gamma, const float* mean,
                                              const float* rstd, const float* scale, const void* dadd, void* ds,
                                              void* dy, float* dgamma, float* dbeta, float* dysum, float* ws,
                                              int64_t rows, int64_t rows_per_sample, int cols, int dtype, void* stream) {
  LVL_REQUIRE((rows == 0 || (scale && dy)) && dgamma && dbeta && ws, "droppath_add_layernorm_bwd: null pointer");
  LVL_REQUIRE(rows >= 0 && rows_per_sample > 0 && rows % rows_per_sample == 0,
              "droppath_add_layernorm_bwd: rows=%lld must be a multiple of rows_per_sample=%lld", (long long)rows,
              (long long)rows_per_sample);
  LVL_REQUIRE(rows < ((int64_t)1 << 32), "droppath_add_layernorm_bwd: rows=%lld must be below 2^32", (long long)rows);
  LVL_REQUIRE((rows == 0 || (dh && s && mean && rstd && ds)) && gamma, "droppath_add_layernorm_bwd: null pointer");
  LVL_REQUIRE(cols > 0 && cols % 8 == 0 && cols <= 4096,
              "droppath_add_layernorm_bwd: cols=%d must be a multiple of 8, <= 4096", cols);
  LVL_REQUIRE(lvl_aligned16(dh) && lvl_aligned16(s) && lvl_aligned16(dadd) && lvl_aligned16(ds) && lvl_aligned16(dy) &&
                  lvl_aligned16(gamma),
              "droppath_add_layernorm_bwd: pointers must be 16-byte aligned");
  {
    // the fused form: lvl_layernorm_bwd's exact-width kernel on its grid, storing dy beside ds
    int64_t nb = (rows + kRowsPerBlock - 1) / kRowsPerBlock;
    if (nb > kLnBwdParts) nb = kLnBwdParts;
    bool fused = false;
#define DP_BWD(VPL, W)                                                                                                    \
  if (int rc = dadd ? dp_bwd_fused_launch<T, VPL, W, true>((const T*)dh, (const T*)s, gamma, mean, rstd, scale,            \
                                                           (const T*)dadd, (T*)ds, (T*)dy, ws, rows, rows_per_sample,     \
                                                           cols, nb, (hipStream_t)stream, &fused)                         \
                    : dp_bwd_fused_launch<T, VPL, W, false>((const T*)dh, (const T*)s, gamma, mean, rstd, scale,           \
                                                            (const T*)nullptr, (T*)ds, (T*)dy, ws, rows, rows_per_sample, \
                                                            cols, nb, (hipStream_t)stream, &fused))                        \
  return rc
    LVL_DISPATCH_DTYPE(dtype, LN_DISPATCH(cols, DP_BWD));
#undef DP_BWD
    if (fused) {
      LVL_CHECK_LAUNCH("droppath_add_layernorm_bwd");
      return lvl_launch_column_reduce(ws, (int)nb, 3 * cols, cols, ws + (size_t)kLnBwdParts * 3 * cols, dgamma, dbeta, dysum,
                                      (hipStream_t)stream);
    }
  }
  // the composed form: the one LayerNorm backward on the kept sum, then dy and its column sums
  if (int rc = lvl_layernorm_bwd(dh, s, nullptr, nullptr, gamma, mean, rstd, dadd, ds, nullptr, dgamma, dbeta, nullptr, ws,
                                 rows, cols, dtype, stream))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  float* part = ws + lvl_workspace_floats("layernorm_bwd", rows, cols);
  int64_t blocks = (rows + kRowsPerBlock - 1) / kRowsPerBlock;
  if (blocks > kDpDyParts) blocks = kDpDyParts;
  if (blocks < 1) blocks = 1;
#define DP_DY(VPL, W)                                                                                                  \
  if (int rc = dp_dy_launch<T, VPL, W>((const T*)ds, scale, (T*)dy, part, rows, rows_per_sample, cols, blocks, st)) \
  return rc
  LVL_DISPATCH_DTYPE(dtype, LN_DISPATCH(cols, DP_DY));
#undef DP_DY
  LVL_CHECK_LAUNCH("droppath_add_layernorm_bwd");
  if (dysum == nullptr) return LVL_OK;
  return lvl_launch_column_reduce(part, (int)blocks, cols, cols, part + (size_t)kDpDyParts * cols, dysum, nullptr, nullptr,
                                  st);
}
