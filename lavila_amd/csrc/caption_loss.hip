// Vocabulary cross-entropy of the narrator's criterion (CaptionLoss, loss.py:220-253) in row form, gfx950.
//
// The logits are rows = B*T rows of `vocab` elements, row r at x + r*row_stride (elements), class stride 1. Three kernels:
//   forward   one pass over each row: log-sum-exp, first argmax, the label's logit -> lse, nll, pred, correct, counted;
//   reduce    one workgroup, fixed summation order: loss, caption_acc, ppl;
//   backward  one pass: coef * upstream * (exp(x - lse) - [j == label]) in the logits' dtype into [rows, Vp] rows,
//             Vp = vocab rounded up to 8, the columns [vocab, Vp) written as zeros.
// A workgroup owns whole rows (the grid is capped and loops). No atomics; every sum is merged in a fixed order.
//
// Running sum. Everything is carried in base 2: a term is 2^(x log2(e) - M) with M an INTEGER >= the largest exponent
// seen, so raising M rescales the sum by an exact power of two. The only roundings are those of the terms and of the
// additions, however often the maximum moves (an e^(m_old - m_new) rescale would add one rounding of an exponential per
// move, 49 of them on a float32 lane at vocab 50257). M = -inf (nothing finite seen yet) is replaced by 0 wherever it
// is subtracted: -inf entries give 2^-inf = 0 and no inf - inf is formed.
//
// Addresses. Nothing is assumed about a row's alignment beyond the element size (row_stride = 50257 puts bf16 rows on
// 2-byte boundaries). The forward processes a scalar head up to the row's first 16-byte boundary, whole workgroup sweeps
// of 16-byte vectors with no predicate on any memory instruction, one partial sweep, a scalar tail. The backward's
// OUTPUT rows are 16-byte aligned by construction; its sweeps are laid on them, and the logits of an output vector are
// read with one 16-byte load that is declared element-aligned (the hardware splits a load that straddles). Columns at
// or past `vocab` are never read.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxGrid = 2048;                        // 8 workgroups per CU; beyond that a workgroup loops over rows
constexpr float kLog2e = 1.44269504088896341f;
constexpr float kLn2 = 0.69314718055994531f;

template <typename T> struct Vec16;                   // one 16-byte vector of T
template <> struct Vec16<float> { static constexpr int W = 4; };
template <> struct Vec16<bf16_t> { static constexpr int W = 8; };

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));   // 16 bytes on a 4- / 2-byte boundary
typedef uint32_t u32x4_a2 __attribute__((ext_vector_type(4), aligned(2)));

__device__ __forceinline__ void unpack16(const uint4& r, float (&v)[4]) {
  v[0] = __uint_as_float(r.x); v[1] = __uint_as_float(r.y); v[2] = __uint_as_float(r.z); v[3] = __uint_as_float(r.w);
}
__device__ __forceinline__ void unpack16(const uint4& r, float (&v)[8]) {
  v[0] = bf16_lo(r.x); v[1] = bf16_hi(r.x); v[2] = bf16_lo(r.y); v[3] = bf16_hi(r.y);
  v[4] = bf16_lo(r.z); v[5] = bf16_hi(r.z); v[6] = bf16_lo(r.w); v[7] = bf16_hi(r.w);
}
__device__ __forceinline__ uint4 load16_aligned(const float* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ uint4 load16_aligned(const bf16_t* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ uint4 load16_any(const float* p) {
  const u32x4_a4 r = *reinterpret_cast<const u32x4_a4*>(p);
  return make_uint4(r.x, r.y, r.z, r.w);
}
__device__ __forceinline__ uint4 load16_any(const bf16_t* p) {
  const u32x4_a2 r = *reinterpret_cast<const u32x4_a2*>(p);
  return make_uint4(r.x, r.y, r.z, r.w);
}
__device__ __forceinline__ uint4 pack16(const float (&v)[4]) {
  return make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
}
__device__ __forceinline__ uint4 pack16(const float (&v)[8]) {
  return make_uint4(f32x2_to_bf16x2(v[0], v[1]), f32x2_to_bf16x2(v[2], v[3]), f32x2_to_bf16x2(v[4], v[5]),
                    f32x2_to_bf16x2(v[6], v[7]));
}

__device__ __forceinline__ float finite_or_zero(float M) { return M == -INFINITY ? 0.f : M; }

// one lane's running state of a row: sum = sum_j 2^(x_j log2e - M), the largest x seen and its FIRST index
struct Run {
  float M, sum, best;
  int idx;
  __device__ __forceinline__ void init() { M = -INFINITY; sum = 0.f; best = -INFINITY; idx = 0x7fffffff; }
  // raise M to cover a largest new element vmax; exact (a power of two), also from and to -inf
  __device__ __forceinline__ float raise(float vmax) {
    const float Mn = fmaxf(M, ceilf(vmax * kLog2e)), Mu = finite_or_zero(Mn);
    sum *= __builtin_amdgcn_exp2f(M - Mu);              // M = -inf: sum is 0 and stays 0
    M = Mn;
    return Mu;
  }
  __device__ __forceinline__ void one(float x, int j) {
    const float Mu = raise(x);
    sum += __builtin_amdgcn_exp2f(fmaf(x, kLog2e, -Mu));
    if (x > best) { best = x; idx = j; }                // indices ascend within a lane: strict > keeps the first
  }
  template <int W>
  __device__ __forceinline__ void vec(const float (&v)[W], int j0) {
    float vmax = v[0];
#pragma unroll
    for (int k = 1; k < W; ++k) vmax = fmaxf(vmax, v[k]);
    const float Mu = raise(vmax);
    float part = 0.f;
#pragma unroll
    for (int k = 0; k < W; ++k) part += __builtin_amdgcn_exp2f(fmaf(v[k], kLog2e, -Mu));
    sum += part;
    if (vmax > best) {                                  // rare after a lane's first vectors
      best = vmax;
#pragma unroll
      for (int k = W - 1; k >= 0; --k)
        if (v[k] == vmax) idx = j0 + k;
    }
  }
};

__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- forward ----------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void token_xent_fwd_kernel(const T* __restrict__ x, int64_t row_stride,
                                                                  const int64_t* __restrict__ labels,
                                                                  int64_t label_stride, int64_t rows, int vocab,
                                                                  int64_t pad_id, float* __restrict__ lse_out,
                                                                  float* __restrict__ nll_out, int32_t* __restrict__ pred_out,
                                                                  int32_t* __restrict__ correct_out,
                                                                  int32_t* __restrict__ counted_out) {
  constexpr int W = Vec16<T>::W;
  __shared__ float red_M[4], red_sum[4], red_best[4];
  __shared__ int red_idx[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    const T* row = x + r * row_stride;
    const int head = min(vocab, (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) / sizeof(T)));
    const int nvec = (vocab - head) / W, tail0 = head + nvec * W;
    const T* body = row + head;                         // 16-byte aligned (or nvec == 0)
    Run s;
    s.init();
    if (tid < head) s.one(Elem<T>::load(row + tid), tid);
    // whole sweeps: every lane loads, nothing is predicated; four sweeps in flight, then single ones
    int v0 = 0;
    for (; v0 + 4 * kThreads <= nvec; v0 += 4 * kThreads) {
      uint4 raw[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) raw[u] = load16_aligned(body + (size_t)(v0 + u * kThreads + tid) * W);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float v[W];
        unpack16(raw[u], v);
        s.vec<W>(v, head + (v0 + u * kThreads + tid) * W);
      }
    }
    for (; v0 + kThreads <= nvec; v0 += kThreads) {
      float v[W];
      unpack16(load16_aligned(body + (size_t)(v0 + tid) * W), v);
      s.vec<W>(v, head + (v0 + tid) * W);
    }
    if (v0 + tid < nvec) {                              // the one partial sweep
      float v[W];
      unpack16(load16_aligned(body + (size_t)(v0 + tid) * W), v);
      s.vec<W>(v, head + (v0 + tid) * W);
    }
    if (tail0 + tid < vocab) s.one(Elem<T>::load(row + tail0 + tid), tail0 + tid);

    // merge the lanes of a wave, then the four waves in wave order
    const float Mw = wave_max(s.M), Mwu = finite_or_zero(Mw);
    const float sw = wave_sum(s.sum * __builtin_amdgcn_exp2f(s.M - Mwu));
    const float bw = wave_max(s.best);
    const int iw = wave_min_int(s.best == bw ? s.idx : 0x7fffffff);
    if (lane == 0) { red_M[wave] = Mw; red_sum[wave] = sw; red_best[wave] = bw; red_idx[wave] = iw; }
    __syncthreads();
    if (tid == 0) {
      float Mr = red_M[0], best = red_best[0];
      for (int w = 1; w < 4; ++w) { Mr = fmaxf(Mr, red_M[w]); best = fmaxf(best, red_best[w]); }
      const float Mu = finite_or_zero(Mr);
      float sum = 0.f;
      int idx = 0x7fffffff;
      for (int w = 0; w < 4; ++w) {
        sum += red_sum[w] * __builtin_amdgcn_exp2f(red_M[w] - Mu);
        if (red_best[w] == best) idx = min(idx, red_idx[w]);
      }
      if (idx == 0x7fffffff) idx = 0;                   // a row without any value > -inf: torch.argmax gives 0
      const float lse = (Mu + __builtin_amdgcn_logf(sum)) * kLn2;
      const int64_t label = labels[r * label_stride];
      const bool counted = label != pad_id;             // the pad id is compared first and may lie outside [0, vocab)
      float nll = 0.f;
      if (counted) nll = (label >= 0 && label < vocab) ? lse - Elem<T>::load(row + label) : __builtin_nanf("");
      lse_out[r] = lse;
      nll_out[r] = nll;
      pred_out[r] = idx;
      correct_out[r] = counted && label == idx;
      counted_out[r] = counted;
    }
    __syncthreads();                                    // red_* are rewritten by the next row
  }
}

// ---- reduce -----------------------------------------------------------------------------------------------------
// out[3] = {loss, caption_acc, ppl}. Lane c takes the captions c, c + 256, ... and sums each over t in order; the
// lanes are merged by wave_sum and the waves in wave order.
__global__ __launch_bounds__(kThreads) void token_xent_reduce_kernel(const float* __restrict__ nll,
                                                                     const int32_t* __restrict__ correct,
                                                                     const int32_t* __restrict__ counted, int B, int T,
                                                                     float* __restrict__ out) {
  __shared__ float red[4][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float sum_nll = 0.f, sum_ppl = 0.f, n_ok = 0.f, n_counted = 0.f;
  for (int b = tid; b < B; b += kThreads) {
    float s = 0.f;
    int ok = 0, n = 0;
    for (int t = 0; t < T; ++t) {
      const size_t r = (size_t)b * T + t;
      s += nll[r];
      ok += correct[r];
      n += counted[r];
    }
    sum_nll += s;
    sum_ppl += expf(s / (float)n);                      // no counted label: 0 / 0 = NaN, as in the reference
    n_ok += (float)ok;                                  // counts stay exact in float32 below 2^24 label positions
    n_counted += (float)n;
  }
  sum_nll = wave_sum(sum_nll); sum_ppl = wave_sum(sum_ppl); n_ok = wave_sum(n_ok); n_counted = wave_sum(n_counted);
  if (lane == 0) { red[wave][0] = sum_nll; red[wave][1] = sum_ppl; red[wave][2] = n_ok; red[wave][3] = n_counted; }
  __syncthreads();
  if (tid == 0) {
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int w = 0; w < 4; ++w)
      for (int k = 0; k < 4; ++k) a[k] += red[w][k];
    out[0] = a[0] / ((float)B * (float)T);
    out[1] = 100.f * a[2] / (a[3] + 1e-8f);
    out[2] = a[1] / (float)B;
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void token_xent_bwd_kernel(const T* __restrict__ x, int64_t row_stride,
                                                                  const int64_t* __restrict__ labels,
                                                                  int64_t label_stride, const float* __restrict__ lse,
                                                                  const float* __restrict__ upstream_p, float coef,
                                                                  int64_t rows, int vocab, int64_t pad_id,
                                                                  T* __restrict__ dlogits) {
  constexpr int W = Vec16<T>::W;
  const int tid = threadIdx.x;
  const int Vp = (vocab + 7) & ~7, nfull = vocab / W, nout = Vp / W;       // vectors of logits / of the output row
  const float k = coef * (upstream_p ? *upstream_p : 1.0f);
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    const T* row = x + r * row_stride;
    uint4* out = reinterpret_cast<uint4*>(dlogits + r * (int64_t)Vp);
    const int64_t label = labels[r * label_stride];
    if (label == pad_id || label < 0 || label >= vocab) {                  // row-uniform: nothing of the row is read
      const float f = label == pad_id ? 0.f : __builtin_nanf("");
      float v[W], z[W];
#pragma unroll
      for (int e = 0; e < W; ++e) { v[e] = f; z[e] = 0.f; }
      const uint4 fill = pack16(v);
      for (int i = tid; i < nfull; i += kThreads) out[i] = fill;
      if (tid == 0 && nfull < nout) {
#pragma unroll
        for (int e = 0; e < W; ++e) z[e] = nfull * W + e < vocab ? f : 0.f;
        out[nfull] = pack16(z);
      }
      if (tid == 1 && nfull + 1 < nout) {                                  // float32: Vp - vocab can pass one vector
#pragma unroll
        for (int e = 0; e < W; ++e) z[e] = 0.f;
        out[nfull + 1] = pack16(z);
      }
      continue;
    }
    const float c = -lse[r] * kLog2e;
    const int lab = (int)label;
    // whole sweeps of whole vectors: no predicate on a load or a store
    int v0 = 0;
    for (; v0 + kThreads <= nfull; v0 += kThreads) {
      const int i = v0 + tid;
      float v[W];
      unpack16(load16_any(row + (size_t)i * W), v);
#pragma unroll
      for (int e = 0; e < W; ++e) v[e] = __builtin_amdgcn_exp2f(fmaf(v[e], kLog2e, c));
      if ((unsigned)(lab - i * W) < (unsigned)W) {
#pragma unroll
        for (int e = 0; e < W; ++e)
          if (i * W + e == lab) v[e] -= 1.f;
      }
#pragma unroll
      for (int e = 0; e < W; ++e) v[e] *= k;
      out[i] = pack16(v);
    }
    // the partial sweep, the vector that straddles `vocab` (read element by element) and the all-pad vector
    for (int i = v0 + tid; i < nout; i += kThreads) {      // float32: up to two vectors past the last whole one
      float v[W];
      if (i < nfull) {
        unpack16(load16_any(row + (size_t)i * W), v);
      } else {
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] = i * W + e < vocab ? Elem<T>::load(row + i * W + e) : 0.f;
      }
#pragma unroll
      for (int e = 0; e < W; ++e) {
        const float p = __builtin_amdgcn_exp2f(fmaf(v[e], kLog2e, c)) - (i * W + e == lab ? 1.f : 0.f);
        v[e] = i * W + e < vocab ? p * k : 0.f;
      }
      out[i] = pack16(v);
    }
  }
}

#define TOKEN_XENT_REQUIRE(name)                                                                                      \
  LVL_REQUIRE(rows >= 0 && vocab > 0 && row_stride >= vocab, name ": bad shape rows=%lld vocab=%d row_stride=%lld",   \
              (long long)rows, vocab, (long long)row_stride);                                                         \
  LVL_REQUIRE(dtype == LVL_F32 || dtype == LVL_BF16, name ": unknown dtype %d", dtype);                             \
  if (rows == 0) return LVL_OK;                                                                                       \
  LVL_REQUIRE(logits && labels, name ": null pointer");                                                               \
  LVL_REQUIRE((reinterpret_cast<uintptr_t>(logits) & (dtype == LVL_F32 ? 3 : 1)) == 0,                                \
              name ": logits must be aligned to their element size")

}  // namespace

extern "C" int lvl_token_xent_fwd(const void* logits, int64_t row_stride, const int64_t* labels, int64_t label_stride,
                                  int64_t rows, int vocab, int64_t pad_id, float* lse, float* nll, int32_t* pred,
                                  int32_t* correct, int32_t* counted, int dtype, void* stream) {
  TOKEN_XENT_REQUIRE("token_xent_fwd");
  LVL_REQUIRE(lse && nll && pred && correct && counted, "token_xent_fwd: null output pointer");
  const dim3 grid((unsigned)(rows < kMaxGrid ? rows : kMaxGrid));
  LVL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((token_xent_fwd_kernel<T>), grid, dim3(kThreads), 0, (hipStream_t)stream,
                                               (const T*)logits, row_stride, labels, label_stride, rows, vocab, pad_id,
                                               lse, nll, pred, correct, counted));
  LVL_CHECK_LAUNCH("token_xent_fwd");
  return LVL_OK;
}

extern "C" int lvl_token_xent_reduce(const float* nll, const int32_t* correct, const int32_t* counted, int B, int T,
                                     float* out3, void* stream) {
  LVL_REQUIRE(B > 0 && T > 0, "token_xent_reduce: bad shape B=%d T=%d", B, T);
  LVL_REQUIRE(nll && correct && counted && out3, "token_xent_reduce: null pointer");
  hipLaunchKernelGGL(token_xent_reduce_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, nll, correct, counted, B,
                     T, out3);
  LVL_CHECK_LAUNCH("token_xent_reduce");
  return LVL_OK;
}

extern "C" int lvl_token_xent_bwd(const void* logits, int64_t row_stride, const int64_t* labels, int64_t label_stride,
                                  const float* lse, const float* upstream, float coef, int64_t rows, int vocab,
                                  int64_t pad_id, void* dlogits, int dtype, void* stream) {
  TOKEN_XENT_REQUIRE("token_xent_bwd");
  LVL_REQUIRE(lse && dlogits && lvl_aligned16(dlogits), "token_xent_bwd: lse and a 16-byte aligned gradient are required");
  const dim3 grid((unsigned)(rows < kMaxGrid ? rows : kMaxGrid));
  LVL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((token_xent_bwd_kernel<T>), grid, dim3(kThreads), 0, (hipStream_t)stream,
                                               (const T*)logits, row_stride, labels, label_stride, lse, upstream, coef,
                                               rows, vocab, pad_id, (T*)dlogits));
  LVL_CHECK_LAUNCH("token_xent_bwd");
  return LVL_OK;
}
