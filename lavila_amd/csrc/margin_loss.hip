// Max-margin ranking losses of the retrieval fine-tune (MaxMarginRankingLoss / AdaptiveMaxMarginRankingLoss,
// loss.py:256-367) in slab form, gfx950.
//
// With x[i,j] = cos(txt_i, img_j), d_i = x[i,i], m_i = margin * w_i and c_i = m_i - d_i the reference's loss is
//     (1/N) sum_i sum_j relu(c_i + x[i,j]) + relu(c_i + x[j,i])
// Three kernels, no [B,G] tensor in HBM, no atomics, every sum merged in a fixed order:
//   prepare  all G gathered rows: both inverse norms (clamped at 1e-8, loss.py:260-262), d_j, c_j, m_j;
//   forward  one workgroup per (16 local rows, direction) in the shape of clip_fwd_mfma_kernel: the raw rows go
//            through v_mfma_f32_16x16x32_bf16 (float32 rows as bf16 hi + lo, three MFMAs; bf16 rows as they are),
//            a cosine is the f32 accumulator times the two f32 inverse norms, the epilogue is the hinge:
//            per (direction, row) the hinge sum and the number of active terms;
//   backward one workgroup per (16 local rows, 64 gradient columns), BOTH directions: it recomputes the scores with
//            the forward's device functions, so it holds cnt_i (active terms of row i in both directions) itself,
//            and applies the normalisation backward with g.u^ taken from the scores (g.u^ = sum_j s_ij x_ij - cnt_i d_i),
//            which is what lets the gradient columns be split over workgroups without a reduction between them.
// The diagonal is analytic: skipped (fix_norm) or relu(m_i) without a gradient; c_i + x[i,i] is never evaluated.
#include "attn_mfma_common.h"

namespace {

using namespace attn_mfma;

constexpr float kEps = 1e-8f;       // sim_matrix's clamp on the row norms

// ---- one definition of a score, shared by forward and backward (their active sets must agree) ------------------
template <typename T> struct Frag;                               // 8 contraction elements of one row, as MFMA operand
template <> struct Frag<float> { uint4 hi, lo; };
template <> struct Frag<bf16_t> { uint4 v; };

__device__ __forceinline__ Frag<float> load_frag(const float* p) {
  float v[8];
  Elem<float>::load8(p, v);
  Frag<float> f;
  split8(v, f.hi, f.lo);
  return f;
}
__device__ __forceinline__ Frag<bf16_t> load_frag(const bf16_t* p) {
  return Frag<bf16_t>{*reinterpret_cast<const uint4*>(p)};
}

// acc += own rows . other rows over 32 channels. DIR 0: the own (A) rows are text rows, DIR 1: image rows. The three
// partial products are ordered by (text, image), not by (A, B): txt.lo*img.hi, txt.hi*img.lo, txt.hi*img.hi, so that
// the pair (txt_i, img_j) gets the same bits in either direction (a product commutes; the k order is the same).
template <int DIR>
__device__ __forceinline__ f32x4 dot_step(const Frag<float>& a, const Frag<float>& b, f32x4 acc) {
  if (DIR == 0) {
    acc = mfma(a.lo, b.hi, acc);
    acc = mfma(a.hi, b.lo, acc);
  } else {
    acc = mfma(a.hi, b.lo, acc);
    acc = mfma(a.lo, b.hi, acc);
  }
  return mfma(a.hi, b.hi, acc);
}
template <int DIR>
__device__ __forceinline__ f32x4 dot_step(const Frag<bf16_t>& a, const Frag<bf16_t>& b, f32x4 acc) {
  return mfma(a.v, b.v, acc);
}

// cosine of a (text, image) pair from the dot product of the RAW rows: normalised rows are never rounded to bf16
// (contraction off: forward and backward must round a score and a hinge argument alike, wherever they are inlined)
__device__ __forceinline__ float cosine(float dot, float inv_txt, float inv_img) {
#pragma clang fp contract(off)
  return (dot * inv_txt) * inv_img;
}
// argument of a hinge term: relu(c + x), active when > 0
__device__ __forceinline__ float hinge_arg(float c, float x) {
#pragma clang fp contract(off)
  return c + x;
}

// prep: [7][G] f32 = {inverse image norm, inverse text norm, d, c, m, clamped image norm, clamped text norm}
struct Prep {
  const float *inv_img, *inv_txt, *d, *c, *m, *den_img, *den_txt;
  __device__ __forceinline__ Prep(const float* p, int G) : inv_img(p), inv_txt(p + G), d(p + 2 * (size_t)G),
                                                            c(p + 3 * (size_t)G), m(p + 4 * (size_t)G),
                                                            den_img(p + 5 * (size_t)G), den_txt(p + 6 * (size_t)G) {}
};

// the 16 own rows of a workgroup as A fragments (lane: row i0 + (lane & 15), channels ks*32 + (lane >> 4)*8 .. +7)
template <typename T, int EK>
__device__ __forceinline__ void load_own(const T* rows, int row0, int i0, int B, int lane, Frag<T> (&a)[EK]) {
  const int ia = min(i0 + (lane & 15), B - 1);
  const T* ap = rows + (size_t)(row0 + ia) * (EK * 32) + (lane >> 4) * 8;
#pragma unroll
  for (int ks = 0; ks < EK; ++ks) a[ks] = load_frag(ap + ks * 32);
}

// cosines of the 16 own rows against gathered rows jt*16 .. +15: x[r] = cos(own row (lane>>4)*4 + r, column j)
template <int DIR, typename T, int EK>
__device__ __forceinline__ void tile_cosines(const Frag<T> (&a)[EK], const T* other, int j, int lane,
                                             const float (&inv_own)[4], float inv_other, float (&x)[4]) {
  const T* bp = other + (size_t)j * (EK * 32) + (lane >> 4) * 8;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < EK; ++ks) acc = dot_step<DIR>(a[ks], load_frag(bp + ks * 32), acc);
#pragma unroll
  for (int r = 0; r < 4; ++r) x[r] = DIR == 0 ? cosine(acc[r], inv_own[r], inv_other) : cosine(acc[r], inv_other, inv_own[r]);
}

// sum over the 16 column lanes of a row group, the same order in every lane
__device__ __forceinline__ float cols16_sum(float v) {
#pragma unroll
  for (int o = 1; o <= 8; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int cols16_sum(int v) {
#pragma unroll
  for (int o = 1; o <= 8; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- prepare --------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void margin_prepare_kernel(const T* __restrict__ img_all, const T* __restrict__ txt_all,
                                                             const float* __restrict__ weight, float margin, int G,
                                                             int E, float* __restrict__ prep) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= G) return;                                  // whole waves leave; no barrier follows
  float sv = 0.f, st = 0.f, tv = 0.f;
  for (int e = lane * 8; e < E; e += 64 * 8) {
    float v[8], t[8];
    Elem<T>::load8(img_all + (size_t)j * E + e, v);
    Elem<T>::load8(txt_all + (size_t)j * E + e, t);
#pragma unroll
    for (int k = 0; k < 8; ++k) { sv = fmaf(v[k], v[k], sv); st = fmaf(t[k], t[k], st); tv = fmaf(t[k], v[k], tv); }
  }
  sv = wave_sum(sv); st = wave_sum(st); tv = wave_sum(tv);
  if (lane == 0) {
    const float den_img = fmaxf(sqrtf(sv), kEps), den_txt = fmaxf(sqrtf(st), kEps);       // == kEps under the clamp
    const float inv_img = 1.f / den_img, inv_txt = 1.f / den_txt;
    const float d = cosine(tv, inv_txt, inv_img), m = weight ? margin * weight[j] : margin;
    prep[j] = inv_img;
    prep[(size_t)G + j] = inv_txt;
    prep[2 * (size_t)G + j] = d;
    prep[3 * (size_t)G + j] = m - d;
    prep[4 * (size_t)G + j] = m;
    prep[5 * (size_t)G + j] = den_img;
    prep[6 * (size_t)G + j] = den_txt;
  }
}

// ---- forward --------------------------------------------------------------------------------------------------
template <int DIR, typename T, int EK>
__device__ __forceinline__ void margin_fwd_sweep(const T* __restrict__ own, const T* __restrict__ other, const Prep& P,
                                                 int B, int G, int row0, int with_diag, float* __restrict__ hinge,
                                                 int32_t* __restrict__ count, float (&red)[4][16][2]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4, i0 = blockIdx.x * 16;
  const float* inv_o = DIR == 0 ? P.inv_txt : P.inv_img;      // norms of the own rows / of the swept rows
  const float* inv_s = DIR == 0 ? P.inv_img : P.inv_txt;
  Frag<T> a[EK];
  load_own<T, EK>(own, row0, i0, B, lane, a);
  float inv_own[4], c_own[4], sum[4];
  int cnt[4], gi[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    gi[r] = row0 + min(i0 + g * 4 + r, B - 1);
    inv_own[r] = inv_o[gi[r]];
    c_own[r] = P.c[gi[r]];
    sum[r] = 0.f;
    cnt[r] = 0;
  }
  const int ntiles = (G + 15) / 16;
#pragma unroll 1
  for (int jt = wave; jt < ntiles; jt += 4) {
    const int j = jt * 16 + c, jc = min(j, G - 1);
    float x[4];
    tile_cosines<DIR, T, EK>(a, other, jc, lane, inv_own, inv_s[jc], x);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float z = hinge_arg(c_own[r], x[r]);
      if (j < G && j != gi[r] && z > 0.f) { sum[r] += z; cnt[r] += 1; }      // columns ascend per lane
    }
  }
  // merge the 16 column lanes of each row, then the 4 waves in wave order
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float s = cols16_sum(sum[r]);
    const int n = cols16_sum(cnt[r]);
    if (c == 0) { red[wave][g * 4 + r][0] = s; red[wave][g * 4 + r][1] = __int_as_float(n); }
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    const int row = threadIdx.x, i = i0 + row;
    if (i < B) {
      float s = 0.f;
      int n = 0;
      for (int w = 0; w < 4; ++w) { s += red[w][row][0]; n += __float_as_int(red[w][row][1]); }
      if (with_diag) s += fmaxf(P.m[row0 + i], 0.f);       // fix_norm=False: the diagonal term is relu(m_i) exactly
      hinge[DIR * B + i] = s;
      count[DIR * B + i] = n;
    }
  }
}

template <typename T, int EK>
__global__ __launch_bounds__(256) void margin_fwd_kernel(const T* __restrict__ img_all, const T* __restrict__ txt_all,
                                                         const float* __restrict__ prep, int B, int G, int row0,
                                                         int with_diag, float* __restrict__ hinge,
                                                         int32_t* __restrict__ count) {
  __shared__ float red[4][16][2];
  const Prep P(prep, G);
  if (blockIdx.y == 0) margin_fwd_sweep<0, T, EK>(txt_all, img_all, P, B, G, row0, with_diag, hinge, count, red);
  else margin_fwd_sweep<1, T, EK>(img_all, txt_all, P, B, G, row0, with_diag, hinge, count, red);
}

// ---- backward -------------------------------------------------------------------------------------------------
constexpr int CH = 256;      // columns per LDS chunk of coefficients: 4 tiles per wave
constexpr int SW = 64;       // gradient columns per workgroup

// One direction of 16 own rows: acc[r][e] = sum_{j != i} s_ij * inv_j * other[j][e0 + m*4 + e] for the rows wave*4 + r
// (partial over the columns j = q mod 4 of lane group q; the caller merges the groups), and per row of the score
// layout the own-threshold count and sum_j s_ij x_ij, with s_ij = [c_i + x > 0] + [c_j + x > 0].
template <int DIR, typename T, int EK>
__device__ __forceinline__ void margin_bwd_sweep(const T* __restrict__ own, const T* __restrict__ other, const Prep& P,
                                                 int B, int G, int row0, int e0, float (*coef)[16],
                                                 float (&acc)[4][4], int (&cnt)[4], float (&sx)[4]) {
  constexpr int E = EK * 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4, i0 = blockIdx.x * 16;
  const float* inv_o = DIR == 0 ? P.inv_txt : P.inv_img;
  const float* inv_s = DIR == 0 ? P.inv_img : P.inv_txt;
  Frag<T> a[EK];
  load_own<T, EK>(own, row0, i0, B, lane, a);
  float inv_own[4], c_own[4];
  int gi[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    gi[r] = row0 + min(i0 + g * 4 + r, B - 1);
    inv_own[r] = inv_o[gi[r]];
    c_own[r] = P.c[gi[r]];
    cnt[r] = 0;
    sx[r] = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[r][e] = 0.f;
  }
#pragma unroll 1
  for (int j0 = 0; j0 < G; j0 += CH) {
    // scores of this chunk -> coefficients in LDS, coef[column][own row]
#pragma unroll 1
    for (int t = 0; t < CH / 64; ++t) {
      const int jl = (t * 4 + wave) * 16 + c, j = j0 + jl, jc = min(j, G - 1);
      float x[4], k[4];
      const float inv_j = inv_s[jc], c_j = P.c[jc];
      if (j0 + (t * 4 + wave) * 16 < G) tile_cosines<DIR, T, EK>(a, other, jc, lane, inv_own, inv_j, x);
      else x[0] = x[1] = x[2] = x[3] = 0.f;                                  // wave-uniform: a tile past the end
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool live = j < G && j != gi[r];
        const int o = live && hinge_arg(c_own[r], x[r]) > 0.f, p = live && hinge_arg(c_j, x[r]) > 0.f;
        const float s = (float)(o + p);
        cnt[r] += o;
        sx[r] += s * x[r];
        k[r] = s * inv_j;
      }
      *reinterpret_cast<float4*>(&coef[jl][g * 4]) = make_float4(k[0], k[1], k[2], k[3]);
    }
    __syncthreads();
    // rows wave*4 .. +3, lane group q takes the columns q, q + 4, ...: 4 channels of a swept row per lane
    const int q = g, m = c;
    const int jn = min(CH, G - j0);
    const T* bp = other + (size_t)j0 * E + e0 + m * 4;
#pragma unroll 4
    for (int jj = q; jj < jn; jj += 4) {
      float v[4];
      Elem<T>::load4(bp + (size_t)jj * E, v);
      const float4 k = *reinterpret_cast<const float4*>(&coef[jj][wave * 4]);
      const float kk[4] = {k.x, k.y, k.z, k.w};
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[r][e] = fmaf(kk[r], v[e], acc[r][e]);
    }
    __syncthreads();
  }
  // merge the four lane groups (every lane receives the sum; a + b commutes, so the four groups hold the same bits)
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[r][e] += __shfl_xor(acc[r][e], 16, 64);
      acc[r][e] += __shfl_xor(acc[r][e], 32, 64);
    }
}

template <typename T, int EK>
__global__ __launch_bounds__(256) void margin_bwd_kernel(const T* __restrict__ img_all, const T* __restrict__ txt_all,
                                                         const float* __restrict__ prep,
                                                         const float* __restrict__ upstream_p, float coef_host, int B,
                                                         int G, int row0, float* __restrict__ dimg,
                                                         float* __restrict__ dtxt) {
  constexpr int E = EK * 32;
  __shared__ __attribute__((aligned(16))) float coef[CH][16];
  __shared__ float red[4][16][3];
  __shared__ float rowstat[16][3];                       // cnt_i, sum s x of direction 0, of direction 1
  const Prep P(prep, G);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4, i0 = blockIdx.x * 16, e0 = blockIdx.y * SW;

  float acc_t[4][4], acc_v[4][4], sx_t[4], sx_v[4];
  int cnt_t[4], cnt_v[4];
  margin_bwd_sweep<0, T, EK>(txt_all, img_all, P, B, G, row0, e0, coef, acc_t, cnt_t, sx_t);
  margin_bwd_sweep<1, T, EK>(img_all, txt_all, P, B, G, row0, e0, coef, acc_v, cnt_v, sx_v);

  // per-row statistics: the 16 column lanes, then the 4 waves in wave order
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = cols16_sum(cnt_t[r] + cnt_v[r]);
    const float st = cols16_sum(sx_t[r]), sv = cols16_sum(sx_v[r]);
    if (c == 0) { red[wave][g * 4 + r][0] = __int_as_float(n); red[wave][g * 4 + r][1] = st; red[wave][g * 4 + r][2] = sv; }
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    int n = 0;
    float st = 0.f, sv = 0.f;
    for (int w = 0; w < 4; ++w) { n += __float_as_int(red[w][threadIdx.x][0]); st += red[w][threadIdx.x][1]; sv += red[w][threadIdx.x][2]; }
    rowstat[threadIdx.x][0] = (float)n;                  // exact: n <= 2G < 2^24
    rowstat[threadIdx.x][1] = st;
    rowstat[threadIdx.x][2] = sv;
  }
  __syncthreads();

  // epilogue: lane group q of wave w writes row w*4 + q, channels e0 + m*4 .. +3 of both gradients
  const int row = wave * 4 + g, i = i0 + row;
  if (i >= B) return;
  const int gi = row0 + i, ec = e0 + c * 4;
  float gt[4], gv[4], t[4], v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    gt[e] = g == 0 ? acc_t[0][e] : g == 1 ? acc_t[1][e] : g == 2 ? acc_t[2][e] : acc_t[3][e];
    gv[e] = g == 0 ? acc_v[0][e] : g == 1 ? acc_v[1][e] : g == 2 ? acc_v[2][e] : acc_v[3][e];
  }
  Elem<T>::load4(txt_all + (size_t)gi * E + ec, t);
  Elem<T>::load4(img_all + (size_t)gi * E + ec, v);
  const float inv_t = P.inv_txt[gi], inv_v = P.inv_img[gi], d = P.d[gi];
  const float n = rowstat[row][0];
  // g.u^ of the gradient w.r.t. the unit row: sum_j s_ij x_ij - cnt_i d_i (the same for both directions' unit rows)
  const float dot_t = rowstat[row][1] - n * d, dot_v = rowstat[row][2] - n * d;
  // norm at or below the clamp: u^ = u / 1e-8, no projection. Read off the clamped norm itself (fmaxf returned kEps),
  // not off the rounding of a division.
  const bool clamp_t = P.den_txt[gi] <= kEps, clamp_v = P.den_img[gi] <= kEps;
  const float k = coef_host * (upstream_p ? *upstream_p : 1.0f);
  float ot[4], ov[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float th = t[e] * inv_t, vh = v[e] * inv_v;
    const float a = gt[e] - n * vh, b = gv[e] - n * th;          // d(sum)/d(t^_i), d(sum)/d(v^_i)
    ot[e] = k * ((clamp_t ? a : a - dot_t * th) * inv_t);
    ov[e] = k * ((clamp_v ? b : b - dot_v * vh) * inv_v);
  }
  *reinterpret_cast<float4*>(dtxt + (size_t)i * E + ec) = make_float4(ot[0], ot[1], ot[2], ot[3]);
  *reinterpret_cast<float4*>(dimg + (size_t)i * E + ec) = make_float4(ov[0], ov[1], ov[2], ov[3]);
}

bool margin_width_ok(int E) { return E == 64 || E == 128 || E == 256 || E == 512; }

#define MARGIN_REQUIRE_COMMON(name, B, G, E, row0)                                                                    \
  LVL_REQUIRE(margin_width_ok(E), name ": E=%d is not supported; the supported widths are 64, 128, 256 and 512", E); \
  LVL_REQUIRE(B >= 0 && G > 0 && row0 >= 0 && row0 + B <= G, name ": bad shape B=%d G=%d E=%d row0=%d", B, G, E, row0); \
  LVL_REQUIRE(dtype == LVL_F32 || dtype == LVL_BF16, name ": unknown dtype %d", dtype);                             \
  LVL_REQUIRE(lvl_aligned16(img_all) && lvl_aligned16(txt_all), name ": pointers must be 16-byte aligned")

#define MARGIN_DISPATCH(KERNEL, grid, ...)                                                                  \
  LVL_DISPATCH_DTYPE(dtype, {                                                                               \
    switch (E) {                                                                                            \
      case 64: hipLaunchKernelGGL((KERNEL<T, 2>), grid, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); break;   \
      case 128: hipLaunchKernelGGL((KERNEL<T, 4>), grid, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); break;  \
      case 256: hipLaunchKernelGGL((KERNEL<T, 8>), grid, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); break;  \
      default: hipLaunchKernelGGL((KERNEL<T, 16>), grid, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); break;  \
    }                                                                                                       \
  })

}  // namespace

extern "C" int lvl_margin_loss_prepare(const void* img_all, const void* txt_all, const float* weight, float margin, int G,
                                       int E, float* prep, int dtype, void* stream) {
  LVL_REQUIRE(img_all && txt_all && prep, "margin_loss_prepare: null pointer");
  MARGIN_REQUIRE_COMMON("margin_loss_prepare", 0, G, E, 0);
  LVL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((margin_prepare_kernel<T>), dim3((unsigned)((G + 3) / 4)), dim3(256), 0,
                                               (hipStream_t)stream, (const T*)img_all, (const T*)txt_all, weight,
                                               margin, G, E, prep));
  LVL_CHECK_LAUNCH("margin_loss_prepare");
  return LVL_OK;
}

extern "C" int lvl_margin_loss_fwd(const void* img_all, const void* txt_all, const float* prep, int B, int G, int E,
                                   int row0, int with_diag, float* hinge, int32_t* count, int dtype, void* stream) {
  LVL_REQUIRE(img_all && txt_all && prep, "margin_loss_fwd: null pointer");
  MARGIN_REQUIRE_COMMON("margin_loss_fwd", B, G, E, row0);
  if (B == 0) return LVL_OK;                           // an empty slab has no outputs to point at
  LVL_REQUIRE(hinge && count, "margin_loss_fwd: null output pointer");
  const dim3 grid((unsigned)((B + 15) / 16), 2);
  MARGIN_DISPATCH(margin_fwd_kernel, grid, (const T*)img_all, (const T*)txt_all, prep, B, G, row0, with_diag, hinge, count);
  LVL_CHECK_LAUNCH("margin_loss_fwd");
  return LVL_OK;
}

extern "C" int lvl_margin_loss_bwd(const void* img_all, const void* txt_all, const float* prep, const float* upstream,
                                   float coef, int B, int G, int E, int row0, float* dimg, float* dtxt, int dtype,
                                   void* stream) {
  LVL_REQUIRE(img_all && txt_all && prep, "margin_loss_bwd: null pointer");
  MARGIN_REQUIRE_COMMON("margin_loss_bwd", B, G, E, row0);
  if (B == 0) return LVL_OK;
  LVL_REQUIRE(dimg && dtxt && lvl_aligned16(dimg) && lvl_aligned16(dtxt),
              "margin_loss_bwd: gradients must be non-null and 16-byte aligned");
  const dim3 grid((unsigned)((B + 15) / 16), (unsigned)(E / SW));
  MARGIN_DISPATCH(margin_bwd_kernel, grid, (const T*)img_all, (const T*)txt_all, prep, upstream, coef, B, G, row0, dimg, dtxt);
  LVL_CHECK_LAUNCH("margin_loss_bwd");
  return LVL_OK;
}
