// Packed caption rows (the narrator's teacher-forced decoder pass on the rows that carry a label), gfx950:
//   lvl_rows_pack     dst[cu[b] + i, 0:D] = src[b, i, 0:D] for i < len_b                    [B, L, D] (strided) -> [R, D]
//   lvl_rows_unpack   dst[b, i, 0:D] = i < len_b ? src[cu[b] + i, 0:D] : 0 for every i < L  [R, D] -> [B, L, D] (strided)
// with len_b = cu[b + 1] - cu[b]. Each is the other's adjoint. Pure copies: rows move as 16-byte words, bit for bit (no
// conversion, a NaN keeps its payload). Every thread of a group of TPR = min(256, next power of two >= words per row)
// lanes walks one row; a workgroup of 256 threads holds 256 / TPR rows; the grid is capped at PACK_MAX_GRID workgroups, which
// stride over the row groups. Memory safety does not rest on `cu`: len_b is clamped into [0, L] and cu[b] into [0, b L] (what
// valid offsets satisfy), so a read or write never leaves the first B L rows of the packed side or the strided rectangle.
#include "common.h"

namespace {

constexpr int PACK_MAX_GRID = 4096;

// PACK: strided rectangle -> packed rows; otherwise packed rows -> strided rectangle (zeros behind len_b)
template <bool PACK>
__global__ __launch_bounds__(256) void rows_kernel(const char* __restrict__ src, char* __restrict__ dst,
                                                   const int32_t* __restrict__ cu, int rows, int L, int words,
                                                   int64_t batch_bytes, int64_t row_bytes, int tpr_log2) {
  const int tpr = 1 << tpr_log2;
  const int lane = threadIdx.x & (tpr - 1);
  const int rows_per_block = 256 >> tpr_log2;
  const int64_t packed_row_bytes = (int64_t)words * 16;
  for (int64_t r0 = (int64_t)blockIdx.x * rows_per_block; r0 < rows; r0 += (int64_t)gridDim.x * rows_per_block) {
    const int64_t r = r0 + (threadIdx.x >> tpr_log2);
    if (r >= rows) continue;
    const int b = (int)(r / L), i = (int)(r - (int64_t)b * L);
    const int c0 = cu[b];
    const int len = min(max(cu[b + 1] - c0, 0), L);
    const int start = min(max(c0, 0), b * L);
    char* rect = const_cast<char*>(PACK ? src : dst) + b * batch_bytes + i * row_bytes;
    char* packed = const_cast<char*>(PACK ? dst : src) + (start + i) * packed_row_bytes;
    if (PACK) {
      if (i >= len) continue;
      for (int w = lane; w < words; w += tpr)
        reinterpret_cast<uint4*>(packed)[w] = reinterpret_cast<const uint4*>(rect)[w];
    } else {
      for (int w = lane; w < words; w += tpr)
        reinterpret_cast<uint4*>(rect)[w] = i < len ? reinterpret_cast<const uint4*>(packed)[w] : make_uint4(0, 0, 0, 0);
    }
  }
}

template <bool PACK>
int launch(const void* src, void* dst, const int32_t* cu, int B, int L, int D, int64_t batch_stride, int64_t row_stride,
           int dtype, void* stream, const char* name) {
  LVL_REQUIRE(dtype == LVL_F32 || dtype == LVL_BF16, "%s: unknown dtype %d", name, dtype);
  LVL_REQUIRE(B >= 0 && L >= 0 && D > 0 && D % 8 == 0, "%s: B = %d, L = %d, D = %d (D must be a positive multiple of 8)", name,
              B, L, D);
  LVL_REQUIRE((int64_t)B * L <= INT32_MAX, "%s: B * L = %lld rows exceed 2^31 - 1", name, (long long)B * L);
  if (B == 0 || L == 0) return LVL_OK;
  LVL_REQUIRE(src && dst && cu, "%s: null pointer", name);
  LVL_REQUIRE(batch_stride >= 0 && row_stride >= D && batch_stride % 8 == 0 && row_stride % 8 == 0,
              "%s: strides (%lld, %lld) must be multiples of 8 elements, the row stride at least D", name,
              (long long)batch_stride, (long long)row_stride);
  LVL_REQUIRE(PACK || B == 1 || batch_stride >= (int64_t)L * row_stride, "%s: destination batches overlap (stride %lld)",
              name, (long long)batch_stride);
  LVL_REQUIRE(lvl_aligned16(src) && lvl_aligned16(dst) && (reinterpret_cast<uintptr_t>(cu) & 3) == 0,
              "%s: src / dst must be 16-byte aligned", name);
  const int esize = dtype == LVL_BF16 ? 2 : 4;
  const int words = D * esize / 16;
  int tpr_log2 = 0;
  while ((1 << tpr_log2) < words && tpr_log2 < 8) ++tpr_log2;
  const int rows = B * L, rows_per_block = 256 >> tpr_log2;
  const int64_t blocks = ((int64_t)rows + rows_per_block - 1) / rows_per_block;
  hipLaunchKernelGGL((rows_kernel<PACK>), dim3((unsigned)(blocks > PACK_MAX_GRID ? PACK_MAX_GRID : blocks)), dim3(256), 0,
                     (hipStream_t)stream, (const char*)src, (char*)dst, cu, rows, L, words, batch_stride * esize,
                     row_stride * esize, tpr_log2);
  LVL_CHECK_LAUNCH(name);
  return LVL_OK;
}

}  // namespace

extern "C" int lvl_rows_pack(const void* src, int64_t src_batch_stride, int64_t src_row_stride, const int32_t* cu, int B,
                             int L, int D, void* dst, int dtype, void* stream) {
  return launch<true>(src, dst, cu, B, L, D, src_batch_stride, src_row_stride, dtype, stream, "rows_pack");
}

extern "C" int lvl_rows_unpack(const void* src, const int32_t* cu, int B, int L, int D, void* dst, int64_t dst_batch_stride,
                               int64_t dst_row_stride, int dtype, void* stream) {
  return launch<false>(src, dst, cu, B, L, D, dst_batch_stride, dst_row_stride, dtype, stream, "rows_unpack");
}
