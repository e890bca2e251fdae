// Weight gradient of the token-major Linear layers: dW[N,K] = dY[M,N]^T X[M,K] (+ dbias[N] = column sums of dY),
// bf16 operands, f32 accumulation, gfx950 MFMA.
//
// Shape of the problem on this path: M = B*T ~ 2e5 rows, N,K in {768, 2304, 3072}: a tiny output contracted over
// a huge row count, with BOTH operands stored row-major over the contraction index (the layout a library GEMM
// likes least: every MFMA fragment needs a transpose). Here:
//   * the output is cut into tiles, the rows into S splits; one workgroup of WN*WK waves per (tile, split), all of
//     them resident at once. A wave owns TA x TB MFMA tiles in registers: 6x6 (96x96; workgroup tile 384x192,
//     192x384, 288x192 ... for the 768-family widths) or 8x4 (128x64; workgroup tile 256x256, 256x128, 128x256 for
//     the 512- and 1024-family widths), or 5x5 (80x80; workgroup tile 320x160, 160x320, 160x160 for the 1600-family
//     widths of the GPT-2 XL decoder: 1600 / 3200 / 4800 / 6400, none of which the other two families divide), or 8x5
//     (128x80; workgroup tile 256x160, 256x320: a vocabulary padded to 256s against such a width -- the tied lm_head
//     of a small-vocabulary decoder);
//   * blockIdx -> (split, tile) is XCD-aware: workgroup i runs on XCD i%8, and XCD x is given a contiguous range
//     of the split-major (split, tile) pairs, so the ~32 workgroups of an XCD stream the SAME dY/X rows through
//     that XCD's L2 (each row is fetched from HBM about once instead of once per tile);
//   * rows are staged 32 at a time as row-major LDS images (row stride padded by 32 B -> an odd number of 32-B
//     bank groups, conflict-free for the reads below; SQ_LDS_BANK_CONFLICT = 0) by LDS-DMA
//     (global_load_lds_dwordx4, no VGPR round trip) into a 4-deep ring: fills run 2-3 steps ahead, one bare
//     s_barrier per step placed mid-step so that neither fill nor LDS latency separates two steps' MFMAs;
//   * both MFMA operands are read with ds_read_b64_tr_b16 (the gfx950 LDS transpose read): lane c of a 16-lane
//     group receives 4 consecutive ROWS at column c, two reads give the 8 contraction elements of a
//     v_mfma_f32_16x16x32_bf16 operand. A and B use the same row permutation, so no data is ever transposed;
//   * dbias rides along: v_dot2_f32_bf16 of the A fragments with (1,1).
// Partial tiles [S,N,K] f32 are reduced by wgrad_reduce_kernel (deterministic, no atomics).
//
// Robustness against a taken compute unit (`sched`, optional): every (tile, split) unit is cut into C row CHUNKS that
// are handed out by a per-unit device counter. A workgroup claims the chunks of ITS OWN unit first -- one returning
// atomic per chunk boundary; while the replies are consecutive the row stream and the fragment pipeline run on across
// the boundary -- and when its unit is exhausted it takes unclaimed chunks of the other splits of the SAME tile into its own accumulators
// (its partial slab then simply holds more rows; the slab sum is unchanged). A workgroup whose CU is held by another
// kernel (an RCCL channel) therefore delays the launch by its tile-mates' share of its rows, not by a second round of
// the whole kernel; when it finally starts it finds its chunks gone and writes a zero slab. When nobody steals, each
// slab holds exactly the rows of the static plan, in the same order, and the result is bit-identical to the static
// schedule. That is the common case with every CU available, NOT a guarantee: a workgroup that finishes its unit takes
// chunks from a tile-mate that is merely slower by more than one chunk (XCD / HBM jitter), the slabs then hold other
// row sets and the f32 summation order of dW depends on timing (exact on integer operands, last-bit differences
// otherwise). Bit-reproducible runs: LAVILA_DYNAMIC_TILES=0 (static plan; the default on a single GPU).
#include "wgrad_kernel.h"

namespace {

// dw[e] = sum_s part[s][e] (+ the < 32 tail rows m >= M_main, which the tiled kernel skips), db[n] likewise
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part,
                                                           const float* __restrict__ bpart,
                                                           const uint16_t* __restrict__ dy,
                                                           const uint16_t* __restrict__ x, float* __restrict__ dw,
                                                           float* __restrict__ db, int64_t M_main, int64_t M, int N,
                                                           int K, int S) {
  const int64_t NK = (int64_t)N * K;
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v * 4 < NK) {
    // fixed summation order s = 0..S-1; the loads of 4 slabs are in flight together
    float4 a = *reinterpret_cast<const float4*>(part + v * 4);
    int s = 1;
    for (; s + 3 < S; s += 4) {
      const float4 b0 = *reinterpret_cast<const float4*>(part + (size_t)s * NK + v * 4);
      const float4 b1 = *reinterpret_cast<const float4*>(part + (size_t)(s + 1) * NK + v * 4);
      const float4 b2 = *reinterpret_cast<const float4*>(part + (size_t)(s + 2) * NK + v * 4);
      const float4 b3 = *reinterpret_cast<const float4*>(part + (size_t)(s + 3) * NK + v * 4);
      a.x = (((a.x + b0.x) + b1.x) + b2.x) + b3.x;
      a.y = (((a.y + b0.y) + b1.y) + b2.y) + b3.y;
      a.z = (((a.z + b0.z) + b1.z) + b2.z) + b3.z;
      a.w = (((a.w + b0.w) + b1.w) + b2.w) + b3.w;
    }
    for (; s < S; ++s) {
      const float4 b = *reinterpret_cast<const float4*>(part + (size_t)s * NK + v * 4);
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    const int n = (int)((v * 4) / K), k = (int)((v * 4) % K);
    for (int64_t m = M_main; m < M; ++m) {
      const float d = bf16_to_f32(dy[m * N + n]);
      const uint2 xr = *reinterpret_cast<const uint2*>(x + m * K + k);
      a.x = fmaf(d, __uint_as_float(xr.x << 16), a.x);
      a.y = fmaf(d, __uint_as_float(xr.x & 0xffff0000u), a.y);
      a.z = fmaf(d, __uint_as_float(xr.y << 16), a.z);
      a.w = fmaf(d, __uint_as_float(xr.y & 0xffff0000u), a.w);
    }
    *reinterpret_cast<float4*>(dw + v * 4) = a;
  }
  if (db != nullptr && v < N) {
    float a = 0.f;
    for (int s = 0; s < S; ++s) a += bpart[(size_t)s * N + v];
    for (int64_t m = M_main; m < M; ++m) a += bf16_to_f32(dy[m * N + v]);
    db[v] = a;
  }
}

// workgroup shapes: {WN, WK, TA, TB}; tile = (16*TA*WN) x (16*TB*WK)
constexpr int kCfg[][4] = {{4, 2, 6, 6}, {2, 4, 6, 6}, {3, 2, 6, 6}, {2, 3, 6, 6}, {2, 2, 6, 6},
                           {2, 4, 8, 4}, {2, 2, 8, 4}, {1, 4, 8, 4},
                           // the 1600-family (5x5 / 8x5 MFMA tiles per wave): considered only for shapes that none of the
                           // configurations above divides, so no earlier plan changes
                           {4, 2, 5, 5}, {2, 4, 5, 5}, {2, 2, 5, 5}, {2, 4, 8, 5}, {2, 2, 8, 5}};
constexpr int kNumCfg = sizeof(kCfg) / sizeof(kCfg[0]);
constexpr int kFirstCfg160 = 8;

// M > 0: the row count of the launch -- a unit keeps at least ~48 steps (1536 rows) so that a short problem (the text
// tower: 8192 rows) is not cut into 250 units whose 256-KiB partial slabs cost more than their MFMAs and which would
// hold every CU while the other tower's kernels wait. M = 0: the largest plan (workspace sizing).
Plan make_plan(int N, int K, int64_t M = 0) {
  Plan best{};
  int64_t best_score = 0;
  bool older_divides = false;
  for (int ci = 0; ci < kFirstCfg160; ++ci)
    older_divides = older_divides || (N % (16 * kCfg[ci][2] * kCfg[ci][0]) == 0 && K % (16 * kCfg[ci][3] * kCfg[ci][1]) == 0);
  for (int ci = older_divides ? 0 : kFirstCfg160; ci < (older_divides ? kFirstCfg160 : kNumCfg); ++ci) {
    const int* c = kCfg[ci];
    const int tn = 16 * c[2] * c[0], tk = 16 * c[3] * c[1];
    if (N % tn || K % tk) continue;
    const int ntiles = (N / tn) * (K / tk);
    const int cus = lvl_persistent_cus();
    if (ntiles > cus) continue;
    // one resident workgroup per CU: S * ntiles <= CUs and a multiple of 8 (XCD mapping)
    const int smax = cus / ntiles;
    int S = smax;
    if (M > 0) {
      const int64_t cap = (M / MS) / 48;
      if (S > cap) S = cap < 1 ? 1 : (int)cap;
    }
    const int want = S;
    const bool any_pairs = ci >= kFirstCfg160;      // the 160-family kernels map any number of (split, tile) pairs onto the XCDs
    while (!any_pairs && S > 1 && (ntiles * S) % 8) --S;
    if (!any_pairs && (ntiles * S) % 8) {    // nothing at or below the cap maps onto whole XCD rounds: go up instead
      S = want;
      while (S <= smax && (ntiles * S) % 8) ++S;
      if (S > smax) continue;
    }
    // score = busy SIMD slots x tile area: 6 waves load the 4 SIMDs 2:2:1:1, 4 waves leave every SIMD one wave
    const int waves = c[0] * c[1];
    const int64_t eff = waves % 4 == 0 ? (waves >= 8 ? 4 : 3) : 3;
    const int64_t score = (int64_t)ntiles * S * eff * 1000 + (int64_t)tn * tk / 64;
    if (score > best_score) {
      best_score = score;
      best = Plan{ci, K / tk, ntiles, S, true};
    }
  }
  return best;
}

}  // namespace

int64_t lvl_wgrad_workspace_floats(int64_t N, int64_t K) {
  const Plan p = make_plan((int)N, (int)K);
  if (!p.ok) return -1;
  return (int64_t)p.S * N * K + (int64_t)p.S * N;
}

// Host-only view of what a launch would run: the make_plan / row_plan results of lvl_linear_wgrad itself (no device code)
extern "C" int lvl_linear_wgrad_plan(int64_t M, int N, int K, int* out) {
  LVL_REQUIRE(out != nullptr, "linear_wgrad_plan: null pointer");
  LVL_REQUIRE(M >= 0 && N > 0 && K > 0, "linear_wgrad_plan: M >= 0 and N, K > 0 needed");
  const Plan p = make_plan(N, K, M);
  if (!p.ok) return lvl_fail(LVL_ENOSYS, "linear_wgrad: no tiling for N=%d K=%d (multiples of 192/288/384, 128/256 or 160/320 needed)", N, K);
  RowPlan rp{};
  if (M > 0) rp = row_plan(M, p.S);
  const int v[9] = {p.cfg, p.tiles_k, p.ntiles, p.S, rp.base, rp.rem, rp.L, rp.nch0, rp.nch1};
  for (int i = 0; i < 9; ++i) out[i] = v[i];
  return LVL_OK;
}

extern "C" int lvl_linear_wgrad_pair_of_block(int cfg, int pairs, int bid) {
  LVL_REQUIRE(cfg >= 0 && cfg < kNumCfg, "linear_wgrad_pair_of_block: unknown configuration %d", cfg);
  LVL_REQUIRE(pairs > 0 && bid >= 0 && bid < pairs, "linear_wgrad_pair_of_block: block %d of %d", bid, pairs);
  return (kCfg[cfg][2] == 5 || kCfg[cfg][3] == 5) ? pair_of_block<true>(pairs, bid) : pair_of_block<false>(pairs, bid);
}

extern "C" int lvl_linear_wgrad(const void* dy, const void* x, float* dw, float* dbias, float* ws, uint32_t* sched,
                                int64_t M, int N, int K, int dtype, void* stream) {
  LVL_REQUIRE(dy && x && dw && ws, "linear_wgrad: null pointer");
  LVL_REQUIRE(dtype == LVL_BF16, "linear_wgrad: bf16 operands only (dtype=%d)", dtype);
  LVL_REQUIRE(M > 0 && N > 0 && K > 0, "linear_wgrad: empty problem");
  LVL_REQUIRE(lvl_aligned16(dy) && lvl_aligned16(x) && lvl_aligned16(dw) && lvl_aligned16(ws),
              "linear_wgrad: pointers must be 16-byte aligned");
  const Plan p = make_plan(N, K, M);
  if (!p.ok) return lvl_fail(LVL_ENOSYS, "linear_wgrad: no tiling for N=%d K=%d (multiples of 192/288/384, 128/256 or 160/320 needed)", N, K);
  hipStream_t st = (hipStream_t)stream;
  float* part = ws;
  float* bpart = dbias ? ws + (size_t)p.S * N * K : nullptr;
  int rc = LVL_OK;
  switch (p.cfg) {
    case 0: rc = launch<4, 2, 6, 6>(p, dy, x, part, bpart, M, N, K, sched, st); break;
    case 1: rc = launch<2, 4, 6, 6>(p, dy, x, part, bpart, M, N, K, sched, st); break;
    case 2: rc = launch<3, 2, 6, 6>(p, dy, x, part, bpart, M, N, K, sched, st); break;
    case 3: rc = launch<2, 3, 6, 6>(p, dy, x, part, bpart, M, N, K, sched, st); break;
    case 4: rc = launch<2, 2, 6, 6>(p, dy, x, part, bpart, M, N, K, sched, st); break;
    case 5: rc = launch<2, 4, 8, 4>(p, dy, x, part, bpart, M, N, K, sched, st); break;
    case 6: rc = launch<2, 2, 8, 4>(p, dy, x, part, bpart, M, N, K, sched, st); break;
    case 7: rc = launch<1, 4, 8, 4>(p, dy, x, part, bpart, M, N, K, sched, st); break;
    default:
      rc = lvl_launch_wgrad_160(p.cfg - kFirstCfg160, p.tiles_k, p.ntiles, p.S, dy, x, part, bpart, M, N, K, sched, st);
      break;
  }
  if (rc != LVL_OK) return rc;
  const int64_t NK = (int64_t)N * K;
  int64_t nthreads = (NK + 3) / 4;
  if (nthreads < N) nthreads = N;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, st, part, bpart,
                     (const uint16_t*)dy, (const uint16_t*)x, dw, dbias, (M / MS) * MS, M, N, K, p.S);
  LVL_CHECK_LAUNCH("linear_wgrad_reduce");
  return LVL_OK;
}
