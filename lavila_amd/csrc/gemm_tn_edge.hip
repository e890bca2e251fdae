// Edge kernel of the ragged TN GEMM (lvl_linear_tn_ragged, gemm_tn_mfma.hip): the columns behind the last full
// 256-column tile of
//
//     Y[M,N] = X[M,K] . W[N,K]^T (+ bias),   bf16 operands, f32 accumulation, bf16 result,
//
// i.e. Y[:, n_first:N] for a remainder N - n_first of 64, 128 or 192 columns (GPT-2 XL's 1600 = 6*256 + 64,
// 4800 = 18*256 + 192, 3200 = 12*256 + 128). The persistent 256x256 kernel computes the full tiles on the same
// stride-N output and is not touched: it has no registers left for a column mask and its K-loop waits count the
// epilogue's stores (see its header), so a second, small kernel takes the remainder instead.
//
// The remainder is at most 12 % of a decoder GEMM (192 of 1600 columns) and usually 4 %, on a few thousand rows: far too
// little work to fill the device by output tiles alone, so the launch is LATENCY-bound -- what matters is how many loads
// are in flight on the whole chip, not the MFMA rate. (A first version, one wave per 32x32 output tile walking all of K with
// two blocks of prefetch, ran at ~1 us per 64-deep K block: 24 us for K = 1600, 715 us for K = 50432.) So:
//   * one workgroup of 8 waves per 32x32 output tile, the contraction SPLIT over the waves: wave q multiplies the K blocks
//     [q nb / 8, (q + 1) nb / 8) of the nb = K / 64 blocks into its own 32x32 f32 accumulator. 2464 rows x 64 columns are
//     154 workgroups = 1232 waves, each with up to three K blocks of fragments in flight;
//   * no operand staging: a v_mfma_f32_32x32x16_bf16 operand is, per lane, 16 contiguous bytes of one row (row = lane & 31,
//     contraction elements 8*(lane>>5)..+7 of the K=16 slice), so every fragment is one global_load_dwordx4 straight into
//     the operand registers; a wave's next two K blocks are in flight while one is multiplied (three register sets, indices
//     static after unrolling by three);
//   * the eight partial tiles meet in 32 KiB of LDS ([wave][accumulator register][lane]: conflict-free) and are added by
//     waves 0-3 in the FIXED order bias, wave 0, wave 1, ... wave 7: no atomics, bit-identical repeats;
//   * operands SWAPPED like the main kernel's (A = weight rows, B = activation rows): a lane ends up with 4 consecutive
//     output columns of one row per accumulator quad -> 8-byte stores, bias read as float4;
//   * rows at or behind M (last row tile): the LOADS re-read row M-1 (clamped row index, as the main kernel's xclamp
//     does), the STORES are skipped. W rows and bias entries are always inside [n_first, N): N % 64 == 0.
// Resources (gfx950, hipcc -O3): see DESIGN.md, "Ragged widths"; no scratch.
#include "internal.h"

typedef __attribute__((ext_vector_type(8))) __bf16 ge_bf16x8;
typedef __attribute__((ext_vector_type(16))) float ge_f32x16;

namespace {

constexpr int EK = 64;          // contraction elements per K block
constexpr int ET = 32;          // workgroup tile: ET rows x ET columns (one MFMA tile)
constexpr int NWK = 8;          // waves of a workgroup = splits of the contraction

__global__ __launch_bounds__(64 * NWK) void gemm_tn_edge_kernel(const uint16_t* __restrict__ X,
                                                                const uint16_t* __restrict__ W,
                                                                const float* __restrict__ bias,
                                                                uint16_t* __restrict__ Y, int64_t M, int N, int K,
                                                                int n_first) {
  __shared__ float part[NWK * 16 * 64];      // [wave][accumulator register][lane]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r5 = lane & 31, hi = lane >> 5;
  const int64_t m = (int64_t)blockIdx.x * ET + r5;                // this lane's output row (and B-operand row)
  const int n0 = n_first + (int)blockIdx.y * ET;                  // first of the tile's 32 output columns (< N)
  const int64_t mc = m < M ? m : M - 1;
  const int nb = K / EK;
  const int b0 = (int)((int64_t)wave * nb / NWK), cnt = (int)((int64_t)(wave + 1) * nb / NWK) - b0;      // this wave's K blocks
  // uint4 units: a K block is 8 of them, a K=16 slice 2, the lane's half of a slice 1
  const uint4* const xp = reinterpret_cast<const uint4*>(X + mc * K) + hi + (int64_t)b0 * 8;
  const uint4* const wp = reinterpret_cast<const uint4*>(W + (int64_t)(n0 + r5) * K) + hi + (int64_t)b0 * 8;

  ge_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  uint4 xf[3][4], wf[3][4];
  auto load = [&](int buf, int j) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      xf[buf][kk] = xp[j * 8 + kk * 2];
      wf[buf][kk] = wp[j * 8 + kk * 2];
    }
  };
  if (cnt > 0) load(0, 0);
  if (cnt > 1) load(1, 1);
  for (int j = 0; j < cnt; j += 3) {
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      if (j + s < cnt) {
        if (j + s + 2 < cnt) load((s + 2) % 3, j + s + 2);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(ge_bf16x8, wf[s][kk]),
                                                        __builtin_bit_cast(ge_bf16x8, xf[s][kk]), acc, 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) part[(wave * 16 + r) * 64 + lane] = acc[r];
  __syncthreads();

  // accumulator register 4*rq + e = output row r5, column 8*rq + 4*hi + e of the tile; wave rq < 4 finishes quad rq
  if (wave < 4) {
    const int rq = wave;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (bias != nullptr) {
      const float4 b = *reinterpret_cast<const float4*>(bias + n0 + 8 * rq + 4 * hi);
      v[0] = b.x;
      v[1] = b.y;
      v[2] = b.z;
      v[3] = b.w;
    }
#pragma unroll
    for (int q = 0; q < NWK; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += part[(q * 16 + 4 * rq + e) * 64 + lane];
    if (m < M)
      *reinterpret_cast<uint2*>(Y + m * (int64_t)N + n0 + 8 * rq + 4 * hi) =
          make_uint2(f32x2_to_bf16x2(v[0], v[1]), f32x2_to_bf16x2(v[2], v[3]));
  }
}

}  // namespace

// Y[:, n_first:N] = X . W[n_first:N]^T (+ bias[n_first:N]); the caller (lvl_linear_tn_ragged) has checked the shapes:
// M >= 1, K % 64 == 0, n_first % 256 == 0, N - n_first in {64, 128, 192}, operands below 4 GiB, 16-byte alignment.
int lvl_launch_tn_edge(const void* x, const void* w, const float* bias, void* y, int64_t M, int N, int K, int n_first,
                       hipStream_t st) {
  const dim3 grid((unsigned)((M + ET - 1) / ET), (unsigned)((N - n_first) / ET));
  hipLaunchKernelGGL(gemm_tn_edge_kernel, grid, dim3(64 * NWK), 0, st, (const uint16_t*)x, (const uint16_t*)w, bias,
                     (uint16_t*)y, M, N, K, n_first);
  LVL_CHECK_LAUNCH("linear_tn_ragged (edge)");
  return LVL_OK;
}
