// Clip ingest: decoded uint8 frames [B,F,H,W,3] -> the normalised clip [B,3,F,S,S] (lvl_clip_ingest) or straight to the
// patch matrix [B*F*N, ld] that lvl_patchify would gather from that clip (lvl_clip_ingest_patches), gfx950.
// Per sample one block {top, left, h, w, Ry, Rx, sy, sx}: the region is resized bilinearly (half-pixel centres, no
// antialiasing) to Ry x Rx, the S x S window at (sy, sx) of that is taken, mirrored along x if flip[b].
// This file is compiled with -ffp-contract=off (build.py, EXTRA_FLAGS): every product, sum and difference below is
// rounded on its own, which is what the host restatement (lavila_amd/ingest.py) and torch's eager float32 ops do.
// Thread = PX consecutive output pixels of one row, all three channels (the source is channel-interleaved, so the twelve
// bytes around a pixel are read together, as two 8-byte loads); source reuse is left to L1 / L2.
#include "internal.h"

namespace {

constexpr int kIngestBlock = 256;
constexpr int kIngestMaxBlocks = 8192;      // grid cap; the kernels walk further items with a grid stride

struct IngestArgs {
  const uint8_t* frames;
  const int32_t* params;      // [B, 8]
  const int32_t* flip;        // [B] or NULL
  int B, F, H, W, S;
  int64_t clip_stride, frame_stride, row_stride;      // bytes
  float mean[3], stdv[3];
};

struct IngestBlock { int top, left, h, w, Ry, Rx, sy, sx; };
struct IngestAxis { int i0, i1; float lam; };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The block of sample b, forced into the frame: a malformed block (refused by the host layer) must not become a read
// outside the source. A valid block passes unchanged.
__device__ __forceinline__ IngestBlock ingest_block(const IngestArgs& a, int b) {
  const int4 lo = *reinterpret_cast<const int4*>(a.params + (int64_t)b * 8);
  const int4 hi = *reinterpret_cast<const int4*>(a.params + (int64_t)b * 8 + 4);
  IngestBlock k;
  k.h = clampi(lo.z, 1, a.H);
  k.w = clampi(lo.w, 1, a.W);
  k.top = clampi(lo.x, 0, a.H - k.h);
  k.left = clampi(lo.y, 0, a.W - k.w);
  k.Ry = max(hi.x, 1);
  k.Rx = max(hi.y, 1);
  k.sy = clampi(hi.z, 0, max(k.Ry - a.S, 0));
  k.sx = clampi(hi.w, 0, max(k.Rx - a.S, 0));
  return k;
}

// source coordinate of index o of an axis resized from n to R (torch's area_pixel_compute_source_index, align_corners=False)
__device__ __forceinline__ IngestAxis ingest_axis(int n, int R, int o) {
  const float scale = (float)n / (float)R;
  float s = scale * ((float)o + 0.5f) - 0.5f;
  s = fmaxf(s, 0.f);
  IngestAxis x;
  x.i0 = min((int)s, n - 1);
  x.i1 = min(x.i0 + 1, n - 1);
  x.lam = s - (float)x.i0;
  return x;
}

// THE definition of one output value: both kernels call it, so they agree to the bit.
__device__ __forceinline__ float ingest_value(float p00, float p01, float p10, float p11, float lx, float ly, float mean,
                                              float stdv) {
  const float wx = 1.f - lx, wy = 1.f - ly;
  const float top = wx * p00 + lx * p01;
  const float bot = wx * p10 + lx * p11;
  const float v = wy * top + ly * bot;
  return (v - mean) / stdv;        // IEEE subtraction and correctly rounded division
}

// PX consecutive pixels x0 .. x0+PX-1 of window row y of frame (b, f), three channels.
// WIDE (frames at least 3 pixels wide): the two source pixels of a row, 6 bytes RGBRGB, come in ONE unaligned 8-byte load
// instead of six byte loads -- the window [start, start + 8) is slid back from the pixel's address where it would leave
// the frame row, so it always lies inside [0, 3 W) of that row: nothing outside the frame is touched, and the bytes of it
// that no pixel of the region owns are shifted out.
__device__ __forceinline__ uint64_t ingest_load8(const uint8_t* p) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}

template <int PX, bool WIDE>
__device__ __forceinline__ void ingest_pixels(const IngestArgs& a, int b, int f, int y, int x0, float (&v)[3][PX]) {
  const IngestBlock k = ingest_block(a, b);
  const bool flip = a.flip != nullptr && a.flip[b] != 0;
  const uint8_t* frame = a.frames + (int64_t)b * a.clip_stride + (int64_t)f * a.frame_stride;
  const IngestAxis ay = ingest_axis(k.h, k.Ry, y + k.sy);
  const uint8_t* r0 = frame + (int64_t)(k.top + ay.i0) * a.row_stride;
  const uint8_t* r1 = frame + (int64_t)(k.top + ay.i1) * a.row_stride;
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    const int x = flip ? a.S - 1 - (x0 + j) : x0 + j;      // the WINDOW is mirrored: flip after the crop
    const IngestAxis ax = ingest_axis(k.w, k.Rx, x + k.sx);
    const int o0 = (k.left + ax.i0) * 3;
    if constexpr (WIDE) {
      const int start = min(o0, a.W * 3 - 8);
      const int sh = (o0 - start) * 8;                     // <= 16 with a right neighbour, <= 40 without
      const uint64_t u0 = ingest_load8(r0 + start) >> sh, u1 = ingest_load8(r1 + start) >> sh;
      const int next = ax.i1 != ax.i0 ? 24 : 0;
      const uint64_t n0 = u0 >> next, n1 = u1 >> next;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        v[c][j] = ingest_value((float)((u0 >> (8 * c)) & 0xff), (float)((n0 >> (8 * c)) & 0xff),
                               (float)((u1 >> (8 * c)) & 0xff), (float)((n1 >> (8 * c)) & 0xff), ax.lam, ay.lam,
                               a.mean[c], a.stdv[c]);
    } else {
      const int o1 = (k.left + ax.i1) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        v[c][j] = ingest_value((float)r0[o0 + c], (float)r0[o1 + c], (float)r1[o0 + c], (float)r1[o1 + c], ax.lam, ay.lam,
                               a.mean[c], a.stdv[c]);
    }
  }
}

// ---- stores: PX consecutive elements, dst aligned to min(16, PX * sizeof(T)) bytes ----------------------------------
struct f16_t { uint16_t bits; };

template <typename T> struct IngestPack;
template <> struct IngestPack<float> {
  static constexpr int kPerWord = 1;
  static __device__ __forceinline__ uint32_t word(const float* v) { return __float_as_uint(v[0]); }
};
template <> struct IngestPack<bf16_t> {
  static constexpr int kPerWord = 2;
  static __device__ __forceinline__ uint32_t word(const float* v) { return f32x2_to_bf16x2(v[0], v[1]); }
};
template <> struct IngestPack<f16_t> {
  static constexpr int kPerWord = 2;
  static __device__ __forceinline__ uint32_t word(const float* v) {      // round-to-nearest-even: v_cvt_f16_f32
    const uint32_t lo = __builtin_bit_cast(uint16_t, (_Float16)v[0]), hi = __builtin_bit_cast(uint16_t, (_Float16)v[1]);
    return lo | (hi << 16);
  }
};

template <typename T, int PX>
__device__ __forceinline__ void ingest_store(T* dst, const float (&v)[PX]) {
  constexpr int kWords = PX / IngestPack<T>::kPerWord;
  static_assert(PX % 2 == 0 && kWords >= 1, "PX is even");
  uint32_t w[kWords];
#pragma unroll
  for (int i = 0; i < kWords; ++i) w[i] = IngestPack<T>::word(v + i * IngestPack<T>::kPerWord);
  uint32_t* d = reinterpret_cast<uint32_t*>(dst);
  if constexpr (kWords % 4 == 0) {
#pragma unroll
    for (int i = 0; i < kWords; i += 4) *reinterpret_cast<uint4*>(d + i) = make_uint4(w[i], w[i + 1], w[i + 2], w[i + 3]);
  } else if constexpr (kWords % 2 == 0) {
#pragma unroll
    for (int i = 0; i < kWords; i += 2) *reinterpret_cast<uint2*>(d + i) = make_uint2(w[i], w[i + 1]);
  } else {
#pragma unroll
    for (int i = 0; i < kWords; ++i) d[i] = w[i];
  }
}

// ---- u8 frames -> clip [B,3,F,S,S]; thread order follows the output rows ---------------------------------------------
template <typename T, int PX, bool WIDE>
__global__ __launch_bounds__(kIngestBlock) void clip_ingest_kernel(IngestArgs a, T* __restrict__ out) {
  const int gx = a.S / PX;
  const int64_t total = (int64_t)a.B * a.F * a.S * gx;
  for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total;
       id += (int64_t)gridDim.x * blockDim.x) {
    int64_t t = id;
    const int xg = (int)(t % gx); t /= gx;
    const int y = (int)(t % a.S); t /= a.S;
    const int f = (int)(t % a.F); t /= a.F;
    const int b = (int)t;
    float v[3][PX];
    ingest_pixels<PX, WIDE>(a, b, f, y, xg * PX, v);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      ingest_store<T, PX>(out + ((((int64_t)b * 3 + c) * a.F + f) * a.S + y) * a.S + (int64_t)xg * PX, v[c]);
  }
}

// ---- u8 frames -> patch matrix [B*F*gh*gw, ld], rows (b, f, py, px), columns (c, i, j), columns 3*P*P .. ld zero ----
// Thread order follows the OUTPUT: (j group, i) of one patch are neighbours, so a patch's P*P elements of one channel
// leave the wave as one contiguous run. The thread that owns a patch's first pixels also writes the row's pad columns.
template <typename T, int PX, bool WIDE>
__global__ __launch_bounds__(kIngestBlock) void clip_ingest_patches_kernel(IngestArgs a, T* __restrict__ out, int P,
                                                                           int64_t ld) {
  const int gj = P / PX, gw = a.S / P;
  const int64_t total = (int64_t)a.B * a.F * gw * gw * P * gj;
  const int kcols = 3 * P * P;
  for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total;
       id += (int64_t)gridDim.x * blockDim.x) {
    int64_t t = id;
    const int jg = (int)(t % gj); t /= gj;
    const int i = (int)(t % P); t /= P;
    const int px = (int)(t % gw); t /= gw;
    const int py = (int)(t % gw); t /= gw;
    const int f = (int)(t % a.F); t /= a.F;
    const int b = (int)t;
    float v[3][PX];
    ingest_pixels<PX, WIDE>(a, b, f, py * P + i, px * P + jg * PX, v);
    T* row = out + ((((int64_t)b * a.F + f) * gw + py) * gw + px) * ld;
#pragma unroll
    for (int c = 0; c < 3; ++c) ingest_store<T, PX>(row + ((int64_t)c * P + i) * P + jg * PX, v[c]);
    if (i == 0 && jg == 0) {
      const float zero[2] = {0.f, 0.f};
      for (int64_t col = kcols; col < ld; col += 2) ingest_store<T, 2>(row + col, zero);      // kcols and ld are even
    }
  }
}

inline unsigned ingest_grid(int64_t total) {
  int64_t g = (total + kIngestBlock - 1) / kIngestBlock;
  if (g > kIngestMaxBlocks) g = kIngestMaxBlocks;
  if (g < 1) g = 1;
  return (unsigned)g;
}

// what both entry points require of the source description; fills `a`
int ingest_args(const char* who, IngestArgs& a, const void* frames, const int32_t* params, const int32_t* flip,
                const void* out, int B, int F, int H, int W, int S, int64_t clip_stride, int64_t frame_stride,
                int64_t row_stride, const float (&mean)[3], const float (&stdv)[3]) {
  LVL_REQUIRE(frames && params && out, "%s: null pointer", who);
  LVL_REQUIRE(B >= 0 && F > 0 && H > 0 && W > 0 && S > 0 && S % 2 == 0, "%s: bad shape B=%d F=%d H=%d W=%d S=%d (S even)",
              who, B, F, H, W, S);
  const int64_t frame_bytes = (int64_t)(H - 1) * row_stride + (int64_t)W * 3;
  LVL_REQUIRE(row_stride >= (int64_t)W * 3 && frame_stride >= frame_bytes &&
                  (B <= 1 || clip_stride >= (int64_t)(F - 1) * frame_stride + frame_bytes),
              "%s: strides (clip %lld, frame %lld, row %lld bytes) overlap for F=%d H=%d W=%d", who, (long long)clip_stride,
              (long long)frame_stride, (long long)row_stride, F, H, W);
  LVL_REQUIRE(lvl_aligned16(params) && lvl_aligned16(out), "%s: params and the output must be 16-byte aligned", who);
  for (int c = 0; c < 3; ++c)
    LVL_REQUIRE(mean[c] == mean[c] && stdv[c] > 0.f && stdv[c] <= 3.0e38f, "%s: std[%d] must be positive and finite", who, c);
  a.frames = (const uint8_t*)frames;
  a.params = params;
  a.flip = flip;
  a.B = B; a.F = F; a.H = H; a.W = W; a.S = S;
  a.clip_stride = clip_stride; a.frame_stride = frame_stride; a.row_stride = row_stride;
  for (int c = 0; c < 3; ++c) { a.mean[c] = mean[c]; a.stdv[c] = stdv[c]; }
  return LVL_OK;
}

template <typename T, int PX>
void launch_clip_px(const IngestArgs& a, void* clip, hipStream_t st) {
  const unsigned grid = ingest_grid((int64_t)a.B * a.F * a.S * a.S / PX);
  if (a.W >= 3)
    hipLaunchKernelGGL((clip_ingest_kernel<T, PX, true>), dim3(grid), dim3(kIngestBlock), 0, st, a, (T*)clip);
  else
    hipLaunchKernelGGL((clip_ingest_kernel<T, PX, false>), dim3(grid), dim3(kIngestBlock), 0, st, a, (T*)clip);
}

template <typename T>
void launch_clip(const IngestArgs& a, void* clip, hipStream_t st) {
  if (a.S % 8 == 0) launch_clip_px<T, 8>(a, clip, st);
  else if (a.S % 4 == 0) launch_clip_px<T, 4>(a, clip, st);
  else launch_clip_px<T, 2>(a, clip, st);
}

template <typename T, int PX>
void launch_patches_px(const IngestArgs& a, void* patches, int P, int64_t ld, hipStream_t st) {
  const unsigned grid = ingest_grid((int64_t)a.B * a.F * a.S * a.S / PX);
  if (a.W >= 3)
    hipLaunchKernelGGL((clip_ingest_patches_kernel<T, PX, true>), dim3(grid), dim3(kIngestBlock), 0, st, a, (T*)patches, P,
                       ld);
  else
    hipLaunchKernelGGL((clip_ingest_patches_kernel<T, PX, false>), dim3(grid), dim3(kIngestBlock), 0, st, a, (T*)patches, P,
                       ld);
}

template <typename T>
void launch_patches(const IngestArgs& a, void* patches, int P, int64_t ld, hipStream_t st) {
  if (P % 8 == 0 && ld % 8 == 0) launch_patches_px<T, 8>(a, patches, P, ld, st);
  else if (P % 4 == 0 && ld % 4 == 0) launch_patches_px<T, 4>(a, patches, P, ld, st);
  else if (P == 14) launch_patches_px<T, 14>(a, patches, P, ld, st);      // a whole patch row per thread, 4- / 8-byte stores
  else launch_patches_px<T, 2>(a, patches, P, ld, st);
}

}  // namespace

extern "C" int lvl_clip_ingest(const void* frames, const int32_t* params, const int32_t* flip, void* clip, int B, int F,
                               int H, int W, int S, int64_t clip_stride, int64_t frame_stride, int64_t row_stride,
                               float mean0, float mean1, float mean2, float std0, float std1, float std2, int dtype,
                               void* stream) {
  IngestArgs a;
  const float mean[3] = {mean0, mean1, mean2}, stdv[3] = {std0, std1, std2};
  const int rc = ingest_args("clip_ingest", a, frames, params, flip, clip, B, F, H, W, S, clip_stride, frame_stride,
                             row_stride, mean, stdv);
  if (rc != LVL_OK) return rc;
  LVL_REQUIRE(dtype == LVL_F32 || dtype == LVL_BF16 || dtype == LVL_F16, "clip_ingest: unknown dtype %d", dtype);
  if (B == 0) return LVL_OK;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == LVL_F32) launch_clip<float>(a, clip, st);
  else if (dtype == LVL_BF16) launch_clip<bf16_t>(a, clip, st);
  else launch_clip<f16_t>(a, clip, st);
  LVL_CHECK_LAUNCH("clip_ingest");
  return LVL_OK;
}

extern "C" int lvl_clip_ingest_patches(const void* frames, const int32_t* params, const int32_t* flip, void* patches,
                                       int B, int F, int H, int W, int S, int P, int64_t ld, int64_t clip_stride,
                                       int64_t frame_stride, int64_t row_stride, float mean0, float mean1, float mean2,
                                       float std0, float std1, float std2, int dtype, void* stream) {
  IngestArgs a;
  const float mean[3] = {mean0, mean1, mean2}, stdv[3] = {std0, std1, std2};
  const int rc = ingest_args("clip_ingest_patches", a, frames, params, flip, patches, B, F, H, W, S, clip_stride,
                             frame_stride, row_stride, mean, stdv);
  if (rc != LVL_OK) return rc;
  LVL_REQUIRE(P > 0 && P % 2 == 0 && S % P == 0, "clip_ingest_patches: S=%d must be a multiple of an even P=%d", S, P);
  LVL_REQUIRE(ld >= (int64_t)3 * P * P && ld % 2 == 0, "clip_ingest_patches: ld=%lld must be even and at least 3*P*P=%d",
              (long long)ld, 3 * P * P);
  LVL_REQUIRE(dtype == LVL_F32 || dtype == LVL_BF16, "clip_ingest_patches: dtype %d (float32 or bf16, the GEMM's operands)",
              dtype);
  if (B == 0) return LVL_OK;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == LVL_F32) launch_patches<float>(a, patches, P, ld, st);
  else launch_patches<bf16_t>(a, patches, P, ld, st);
  LVL_CHECK_LAUNCH("clip_ingest_patches");
  return LVL_OK;
}
