// Forward and input-gradient GEMMs of the token-major Linear layers, with the element-wise neighbours of the
// reference fused into the epilogue:
//
//     Y[M,N] = epilogue( X[M,K] . W[N,K]^T ),   bf16 operands (both contraction-contiguous), f32 accumulation.
//
//   forward          y  = x W^T + b                    (W = the layer's weight [out,in])
//   input gradient   dx = dy Wt^T                      (Wt = the transposed bf16 weight copy [in,out] that
//                                                       lvl_cast_transpose writes beside the forward's cast)
// Epilogues (template EPI):
//   0  y = acc (+ bias)                                                    qkv / proj / fc2 / patch embed / dgrads
//   1  u = acc + bias -> aux_out ; y = u * sigmoid(1.702 u)                Mlp.fc1 + QuickGELU (timesformer.py:52-54)
//   2  y = acc * quickgelu'(aux_in) ; column sums of y -> partial slab     backward of the same: fc2's input gradient
//                                                                          becomes d(fc1 output); sums = d(fc1 bias)
//   3  y = acc (+ bias) + aux_in                                           proj / fc2 + residual: the block's
//                                                                          `x + attn(...)`, `x + mlp(...)` adds
//                                                                          (timesformer.py:183-196) leave the GEMM as
//                                                                          the new residual stream
//   4  u = acc + bias ; y = u * sigmoid(1.702 u) ; aux_out = quickgelu'(u) epilogue 1 for training (bf16 only): the
//                                                                          backward needs the DERIVATIVE, and the forward
//                                                                          has sigmoid(1.702 u) in a register already
//   5  y = acc * aux_in ; column sums of y -> partial slab                 epilogue 2 on the stored derivative: no
//                                                                          transcendental in the backward (epilogue 2
//                                                                          is VALU-bound: +6 us per 28-us tile)
//   6  u = acc + bias -> aux_out ; y = gelu(u)                             epilogue 1 with the exact (erf) GELU of
//                                                                          gelu_erf.h: the reference's default
//                                                                          SpaceTimeTransformer (act_layer=nn.GELU)
//   7  y = acc * gelu'(aux_in) ; column sums of y -> partial slab          epilogue 2 for the same
//   8  u = acc + bias ; y = gelu(u) ; aux_out = gelu'(u)                   epilogue 4 for the same (bf16 only): one erf
//                                                                          serves both; the backward is epilogue 5
//      (6-8 are instantiated in gemm_tn_gelu.hip from the same template, gemm_tn_kernel.h: lvl_launch_tn_gelu)
//
// f32-CLASS MODE (template F32O, C-ABI dtype LVL_F32): the SAME kernel -- tile walk, LDS-DMA ring, swizzle, MFMA phases,
// bias image, epilogue arithmetic -- with float32 results. The operands are bf16 TERM IMAGES of float32 matrices
// (lvl_split_bf16x3, elementwise.hip): x = xh + xl (+ O(2^-18 x)), xh = bf16(x), xl = bf16(x - xh), laid out along the
// contraction as X3 = [xh | xh | xl], W3 = [wh | wl | wh], so that one pass over K' = 3K accumulates
// xh.wh + xh.wl + xl.wh in the f32 accumulators: every product is exact, what is dropped is xl.wl and the second-order
// remainders (~2^-17 relative per product). y / aux_out / aux_in are float32; the QuickGELU epilogues see the unrounded
// f32 pre-activation. This is the parity configuration's GEMM (north_star: "within 1e-3 fp32"): it puts the benched
// kernel itself, not a library GEMM, under the f32 tolerance.
//
// Shape of the problem on this path: M = B*T ~ 2e5 rows, N,K in {768, 2304, 3072}. Measured facts that shaped it
// (profiles/r02_pmc_gemm_tn_v1_qkv.txt, tools/probe_gemm_trace.py): (1) what the L2 can serve is a number of
// REQUESTS, so every request must be a full 128-byte line (a K step of 32 = 64-byte rows doubled the requests and
// ran at 650-930 TF/s); (2) a workgroup that ends after one tile pays ~17 us of launch + first-fetch + store drain
// per 20-us tile; (3) under this load the chip clocks at 1.3-1.7 GHz (power), so instruction and LDS economy matter
// as much as stalls. Design:
//   * PERSISTENT workgroups (one per CU) of 8 waves (2 along M x 4 along N) walk 256x256 output tiles; the K loop
//     never drains at a tile boundary: the first blocks of the next tile are in flight, and its first operands
//     already in registers, while the finished tile is stored;
//   * v_mfma_f32_32x32x16_bf16 with SWAPPED operands (A = weight rows, B = activation rows): the accumulator then
//     holds, per lane, 4 consecutive output columns of one row, so bias / activation / aux tensors are read and
//     written as 8- and 16-byte vectors without an LDS transpose of the tile;
//   * MFMA SHAPE. The bf16 epilogues 0-5 also exist on v_mfma_f32_16x16x32_bf16 (gemm_tn_mfma16<EPI>, the same body with
//     MS = 16): the same 128x64 block per wave as 8 x 4 accumulators of 16 x 16, twice the MFMAs at half the cycles, the
//     same 24 fragment reads, fills, barriers and waits per K block, the same operand swap (a lane holds 4 consecutive
//     columns of row lane & 15; the four 16-lane groups hold adjacent 8-byte pieces of a row and permlane16_swap widens
//     them to the same 16 16-byte stores per wave). The loop is bound by the clock the chip holds under MFMA load, and it
//     holds a higher one on this shape (profiles/gemm_mfma_shape.txt); which shape a launch takes: mfma_shape() below,
//     lvl_set_gemm_mfma_shape. The f32-class mode and the exact-GELU unit stay on 32x32x16;
//   * K is walked in blocks of 64 (one 128-byte line per operand row). The 128 KiB of LDS are a ring of 8 SLOTS of
//     128 rows x 128 B: a K block is four slots (X rows 0-127 | X rows 128-255 | W half 0 | W half 1), two blocks are
//     resident. LDS is only a transit buffer: a wave's share of a slot is read ONCE into registers (X: 64 rows = 8
//     fragments, W: 32 rows = 4 fragments) and the slot is refilled by LDS-DMA (global_load_lds_dwordx4, no VGPR round
//     trip) as soon as every wave has consumed it -- 5-6 phases before it is read again;
//   * a K block is four PHASES, one output quadrant (64 x 32 per wave, 8 MFMAs) each, ordered so that every phase
//     needs exactly one new operand: P0 X0.W0, P1 X0.W1, P2 X1.W1, P3 X1.W0. All waves run in step with ONE bare
//     s_barrier per phase; the reads of the NEXT phase's operand and the refill DMAs ride between the MFMAs (one
//     per MFMA), so no LDS or DMA latency separates two phases and the two waves of a SIMD cover each other;
//   * the eight 16-byte chunks of a row are XOR-permuted inside a slot (chunk ^ ((row>>1) & 7), applied to the per-lane
//     SOURCE address of the DMA and to the fragment reads): every ds_read_b128 lane group touches 16 distinct 16-byte
//     slots of the 256-byte bank row (SQ_LDS_BANK_CONFLICT = 0), and the 8 lanes of a row still fetch one whole line;
//   * the tile's bias values travel by LDS-DMA too, so the epilogue issues no vector-memory load; its stores stay in
//     flight across the next tile's first blocks (the vmcnt allowances account for them);
//   * blockIdx -> tile is XCD-aware (workgroup i runs on XCD i % 8): each XCD owns a contiguous range of the
//     N-fastest tile order, so the N/256 tiles that read the same 256 rows of X sit behind one L2 and X comes from
//     HBM once; W (<= 4.7 MB) lives in L2 / Infinity Cache;
//   * inside an XCD's range the tiles are handed out by a DEVICE TILE COUNTER (one word per XCD, `sched`): a
//     workgroup takes the next tile of its XCD's queue with one returning atomic add, issued in front of the
//     result stores of the tile before the tile before, so that its latency never shows (the reply is parked in a register, published to the other waves
//     through an LDS mailbox two K blocks later -- by then the counted vmcnt waits of the K loop have covered it --
//     and read by the fetch cursor when it wraps to the next tile, three K blocks before the end).
//     A compute unit that another kernel holds (an RCCL channel during the gradient all-reduce) therefore costs
//     the launch one tile's worth of throughput, not a static range of tiles: its workgroup starts late, finds
//     the queues drained and leaves. The last workgroup out zeroes the counters again.
//
// N IS A STRIDE. The kernel uses N only as the row stride of Y (and of aux / the column partials); the column tiles it
// walks are `tiles_n`, which launch_tn computes as N / 256 rounded DOWN. Launched on an output whose width is not a
// multiple of 256 it computes the first 256 * (N / 256) columns exactly as it would for W[:256 * (N / 256)] and never
// reads or writes the columns behind them. lvl_linear_tn keeps refusing such an N (its epilogues 2 / 5 / 7 reduce column
// partials over all N columns); lvl_linear_tn_ragged (bottom of this file) uses the property for N % 64 == 0: this
// kernel for the full tiles, gemm_tn_edge.hip's small kernel for the 64 / 128 / 192 columns behind them. The kernel has
// no column mask and gets none: it sits at 248-252 VGPRs, and its K-loop waits COUNT the epilogue's stores (NS below),
// which a sometimes-skipped store would break.
#include "gemm_tn_kernel.h"

// ---- MFMA shape of the bf16 launches (epilogues 0-5) -------------------------------------------------------------------
// 0 = the table below; 16 / 32 force a shape (lvl_set_gemm_mfma_shape: the tests run every check under both, the probes
// time both). The GM_AUDIT build compiles this file alone and so carries the same setter and the same table.
static std::atomic<int> g_mfma_shape{0};
extern "C" int lvl_set_gemm_mfma_shape(int shape) {
  if (shape != 0 && shape != 16 && shape != 32)
    return lvl_fail(LVL_EINVAL, "set_gemm_mfma_shape: %d is not 0 (default), 16 or 32", shape);
  g_mfma_shape.store(shape, std::memory_order_relaxed);
  return LVL_OK;
}
// The default, from interleaved timings of both shapes on random data at the step's shapes (profiles/gemm_mfma_shape.txt):
// v_mfma_f32_16x16x32_bf16 for every (N, K, epilogue) -- the table is this one line.
static int mfma_shape(int /*epilogue*/, int /*N*/, int /*K*/) {
  const int forced = g_mfma_shape.load(std::memory_order_relaxed);
  return forced ? forced : 16;
}

// This unit's kernels: epilogues 0-5 of the table (gemm_tn_kernel.h: kTnEpilogues) in the modes it gives them, on MFMA shape
// `ms` in bf16 (the f32-class mode runs 32x32x16). The one switch over epilogue codes of this file: lvl_linear_tn, the audit
// and the trace entries launch through it. -1: not instantiated here.
static int tn_launch(int epilogue, bool f32, int ms, const TnCall& c) {
  switch (epilogue) {
    case LVL_EPI_BIAS: return launch_tn_mode<0, true>(f32, ms, c);
    case LVL_EPI_BIAS_QUICKGELU: return launch_tn_mode<1, true>(f32, ms, c);
    case LVL_EPI_QUICKGELU_BWD: return launch_tn_mode<2, true>(f32, ms, c);
    case LVL_EPI_BIAS_RESIDUAL: return launch_tn_mode<3, true>(f32, ms, c);
    case LVL_EPI_BIAS_QUICKGELU_DERIV: return launch_tn_mode<4, true>(f32, ms, c);
    case LVL_EPI_MUL_AUX_COLSUM: return launch_tn_mode<5, true>(f32, ms, c);
  }
  return -1;
}

int64_t lvl_linear_tn_workspace_floats(int64_t M, int64_t N) {
  return (2 * ((M + TM - 1) / TM) + lvl_colsum_mid_rows()) * N;      // column partials + the reducer's intermediate rows
}

#ifdef GM_TRACE
extern "C" int lvl_linear_tn_trace(const void* x, const void* w, const float* bias, void* y, void* trace, int64_t M,
                                   int N, int K, void* stream) {
  return launch_tn<0>(x, w, bias, y, nullptr, nullptr, (float*)trace, M, N, K, nullptr, (hipStream_t)stream);
}
// the same with an epilogue (0, 1, 3, 4, 5), on 32x32x16; epilogue 5: `trace` starts with room for the column partials
extern "C" int lvl_linear_tn_trace_epi(const void* x, const void* w, const float* bias, void* y, void* aux_out,
                                       const void* aux_in, void* trace, int64_t M, int N, int K, int epilogue, void* stream) {
  if (epilogue == LVL_EPI_QUICKGELU_BWD) return -1;
  return tn_launch(epilogue, false, 32, {x, w, bias, y, aux_out, aux_in, (float*)trace, M, N, K, nullptr, (hipStream_t)stream});
}
#endif

#ifdef GM_AUDIT
// lvl_linear_tn's launch (bf16 epilogues 0-5, f32-class 0-3; epilogues 6-8: the same entry of gemm_tn_gelu.hip's audit build, static or dynamic schedule) with the store-count records of
// every wave in `audit` (layout at the kernel's GM_AUDIT block; epilogues 2 / 5: behind their [2 * tiles_m][N] column
// partials, which are left unreduced)
extern "C" int lvl_linear_tn_audit_cap() { return GM_AUDIT_CAP; }
extern "C" int lvl_linear_tn_audit(const void* x, const void* w, const float* bias, void* y, void* aux_out,
                                   const void* aux_in, void* audit, uint32_t* sched, int64_t M, int N, int K, int epilogue,
                                   int dtype, void* stream) {
  return tn_launch(epilogue, dtype == LVL_F32, mfma_shape(epilogue, N, K),
                   {x, w, bias, y, aux_out, aux_in, (float*)audit, M, N, K, sched, (hipStream_t)stream});
}
#endif

extern "C" int lvl_linear_tn(const void* x, const void* w, const float* bias, void* y, void* aux_out,
                             const void* aux_in, float* colsum, float* ws, uint32_t* sched, int64_t M, int N, int K,
                             int epilogue, int dtype, void* stream) {
  TnCall c{x, w, bias, y, aux_out, aux_in, nullptr, M, N, K, sched, (hipStream_t)stream};
  const int bad = tn_check_args("linear_tn", c, TN, epilogue, dtype, false);
  if (bad != LVL_OK) return bad;
  const bool f32 = dtype == LVL_F32;      // f32-class mode: bf16 term images in (K = 3 x the layer's width), float32 out
  LVL_REQUIRE(!f32 || K % (3 * BK) == 0, "linear_tn (f32 class): K = %d is not 3 x a multiple of 64", K);
  LVL_REQUIRE(tn_epilogue_known(epilogue), "linear_tn: unknown epilogue %d", epilogue);
  const TnEpilogue& e = kTnEpilogues[epilogue];
  if (f32 && !e.f32)
    return lvl_fail(LVL_ENOSYS, "linear_tn: epilogue %d is a bf16 epilogue (the f32-class mode keeps the pre-activation: "
                                "LVL_EPI_BIAS_QUICKGELU / LVL_EPI_QUICKGELU_BWD, LVL_EPI_BIAS_GELU / LVL_EPI_GELU_BWD)",
                    epilogue);
  LVL_REQUIRE(!e.aux_out || aux_out != nullptr, "linear_tn: the %s epilogue writes to aux_out", e.name);
  if (e.colpart)
    LVL_REQUIRE(aux_in != nullptr && colsum != nullptr && ws != nullptr && lvl_aligned16(ws),
                "linear_tn: the %s epilogue needs aux_in, colsum and a workspace", e.name);
  LVL_REQUIRE(!e.aux_in || aux_in != nullptr, "linear_tn: the %s epilogue reads aux_in", e.name);
  if (e.colpart) c.colpart = ws;
  const int rc = e.unit == TN_UNIT_GELU ? lvl_launch_tn_gelu(x, w, bias, y, aux_out, aux_in, c.colpart, M, N, K, sched, epilogue, f32, c.st)
                                        : tn_launch(epilogue, f32, mfma_shape(epilogue, N, K), c);
  if (rc != LVL_OK || !e.colpart) return rc;
  const int P = (int)(2 * ((M + TM - 1) / TM));      // the column partials -> colsum
  return lvl_launch_column_reduce(ws, P, N, N, ws + (size_t)P * N, colsum, nullptr, nullptr, c.st);
}

// Plain GEMM (+ bias) for any N % 64 == 0 (the decoder widths of the GPT-2 XL narrators: 1600, 3200, 4800): the full
// 256-column tiles by the persistent kernel above -- the launch, grid and schedule lvl_linear_tn issues for W[:N0],
// N0 = 256 * (N / 256), with N as the output stride -- and the N - N0 columns behind them by the edge kernel
// (gemm_tn_edge.hip) on the same stream. The two launches write disjoint columns of y.
extern "C" int lvl_linear_tn_ragged(const void* x, const void* w, const float* bias, void* y, uint32_t* sched, int64_t M,
                                    int N, int K, int epilogue, int dtype, void* stream) {
  const TnCall c{x, w, bias, y, nullptr, nullptr, nullptr, M, N, K, sched, (hipStream_t)stream};
  const int bad = tn_check_args("linear_tn_ragged", c, 64, epilogue, dtype, true);
  if (bad != LVL_OK) return bad;
  const int N0 = N / TN * TN;
  if (N0 > 0) {
    const int rc = tn_launch(LVL_EPI_BIAS, false, mfma_shape(LVL_EPI_BIAS, N, K), c);
    if (rc != LVL_OK) return rc;
  }
  if (N0 < N) return lvl_launch_tn_edge(x, w, bias, y, M, N, K, N0, c.st);
  return LVL_OK;
}
