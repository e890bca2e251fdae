// Backward of the decoder cross-attention (lvl_cross_attn_rows_bwd), bf16, gfx950: the structure of the forward
// (cross_attn_mfma.hip). One workgroup per (context, head) stages the head's keys and values (<= 256 x 64 each) ONCE into
// the swizzled LDS images of attn_mfma_common.h and walks the context's `qrep` query rows in rounds of 64 (16 per wave).
//
// Phase A of a round, per wave on its 16 query rows (the forward's operand layout: scores transposed, a lane owns one query):
//   S^T  = K . Q^T, exact single-pass softmax over the 16 key tiles held in registers -> P
//   dP^T = V . dO^T;  delta = rowsum(P o dP);  dS = P o (dP - delta)
//   dQ   = 0.125 dS . K       (dS packed to bf16 in registers, K through the LDS transpose read)
//   P^T and dS^T (bf16) go to two [256 keys][64 queries] LDS images, Q and dO of the 16 rows to two [64][64] images.
// Phase B, per wave on the 64 keys it OWNS (key tiles 4 wave .. 4 wave + 3), over the round's 64 query rows:
//   dV += P^T . dO,  dK += dS^T . Q      (two full 32-deep contractions each; operands from the images above)
// Every key row is accumulated by one wave, in f32 registers, rounds in order: there is nothing to combine across waves or
// workgroups, no atomics, and two runs are bit-identical. dK (x 0.125) and dV are rounded once to bf16 at the end.
// Tails: key rows >= Tk are zero in the images and masked in the softmax; query rows >= qrep are never read (zero operands,
// so they add exact zeros in phase B) and never written.
//
// The kernel is a template over DROP and CAUSAL like the forward's (lvl_attn_rows_drop_bwd; <false, false> is
// lvl_cross_attn_rows_bwd's kernel to the bit), with the same pointer + stride operands, so that dq / dk / dv of the causal
// self-attention land in the thirds of dqkv [B L, 3D]. DROP regenerates the forward's mask (dropout.h) once per round into
// 64 bits per lane (16 fragments x 4 keys; the kernel already holds 4 x 64 accumulator registers per lane):
//   dPd = dO . V^T,  dP = keep ? dPd / (1 - p) : 0,  delta = sum_j P dP (= dO . O),  dS = P o (dP - delta),
//   dV += Pd^T . dO with Pd = keep ? P / (1 - p) : 0 (the P^T image holds Pd);  dQ, dK from dS as before.
//
// Host side: lvl_launch_rows_attn_mfma_bwd is the one launch site, behind the backward entries of all four rows-attention
// pairs; they describe their call as a RowsAttn and share lvl_rows_attn_check (internal.h, cross_attn_mfma.hip).
#include "attn_mfma_common.h"
#include "dropout.h"
#include "internal.h"
#include "keymask.h"

using namespace attn_mfma;

namespace {

constexpr int XW = 4;          // waves per workgroup
constexpr int NKT = 16;        // key tiles of 16: up to 256 keys
constexpr int QR = 16 * XW;    // query rows per round

struct AttnDrop {
  uint64_t seed;
  uint32_t site, thr;
  float scale;
  int idx_qrep;                // query rows per context in the element index (the forward's)
};

// q / dq rows `qs` elements apart, keys / values / dk / dv rows `kvs` apart and contexts `kvctx` apart; dout [rows, D]
// KEYMASK (lvl_keymask_attn_bwd): the forward's key mask; hidden keys have P = dS = 0, so their dk / dv rows are sums of
// exact zeros; a context with no visible key has the uniform P and dS = 0
template <bool DROP, bool CAUSAL, bool KEYMASK = false>
__global__ __launch_bounds__(64 * XW) void cross_attn_bwd_mfma_kernel(const uint16_t* __restrict__ q, size_t qs,
                                                                      const uint16_t* __restrict__ kp,
                                                                      const uint16_t* __restrict__ vp, size_t kvs,
                                                                      size_t kvctx, const uint16_t* __restrict__ dout,
                                                                      uint16_t* __restrict__ dq,
                                                                      uint16_t* __restrict__ dk,
                                                                      uint16_t* __restrict__ dv, int Tk, int H,
                                                                      int qrep, AttnDrop drop,
                                                                      const uint8_t* __restrict__ mask = nullptr,
                                                                      size_t mctx = 0) {
  extern __shared__ __align__(16) uint16_t xb_smem[];
  uint16_t* Ks = xb_smem;
  uint16_t* Vs = Ks + NKT * 16 * RS;
  uint16_t* Pi = Vs + NKT * 16 * RS;        // P^T  [key][query of the round]
  uint16_t* Di = Pi + NKT * 16 * RS;        // dS^T [key][query of the round]
  uint16_t* Qi = Di + NKT * 16 * RS;        // Q  [query of the round][channel]
  uint16_t* Oi = Qi + QR * RS;              // dO [query of the round][channel]
  uint16_t* Ot = Oi + QR * RS;              // per-wave output transposition tiles
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int h = blockIdx.x % H, ctx = blockIdx.x / H;
  const int D = H * 64;
  const size_t kvoff = (size_t)ctx * kvctx + h * 64;
  stage_rows2<PrecBf16, 64 * XW, NKT / 2>(Ks, kp + kvoff, kvs, nullptr, Vs, vp + kvoff, kvs, nullptr, NKT * 16, Tk, tid, 0);
  __syncthreads();
  constexpr float kExp2 = 0.125f * 1.4426950408889634f;
  const FragOff fo = frag_offsets(lane);
  uint16_t* ot = Ot + wave * 16 * OS;
  f32x4 dV[4][4], dK[4][4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      dV[kk][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
      dK[kk][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  const int nrounds = (qrep + QR - 1) / QR;
  const int qcol = wave * 16 + c;             // this lane's query as a column of the P^T / dS^T images
  const KeyVis kv = key_visibility<KEYMASK>(mask, (size_t)ctx * mctx, Tk, g);
#pragma unroll 1
  for (int rd = 0; rd < nrounds; ++rd) {
    // ---- phase A -------------------------------------------------------------------------------------------------
    const int q0 = rd * QR + wave * 16;
    const int qrow = q0 + c;
    uint4 qf0 = make_uint4(0, 0, 0, 0), qf1 = qf0, df0 = qf0, df1 = qf0;
    if (qrow < qrep) {
      const size_t off = ((size_t)ctx * qrep + qrow) * D + h * 64 + g * 8;
      const size_t qoff = ((size_t)ctx * qrep + qrow) * qs + h * 64 + g * 8;
      qf0 = *reinterpret_cast<const uint4*>(q + qoff);
      qf1 = *reinterpret_cast<const uint4*>(q + qoff + 32);
      df0 = *reinterpret_cast<const uint4*>(dout + off);
      df1 = *reinterpret_cast<const uint4*>(dout + off + 32);
    }
    *reinterpret_cast<uint4*>(Qi + img_off(qcol, g)) = qf0;
    *reinterpret_cast<uint4*>(Qi + img_off(qcol, 4 + g)) = qf1;
    *reinterpret_cast<uint4*>(Oi + img_off(qcol, g)) = df0;
    *reinterpret_cast<uint4*>(Oi + img_off(qcol, 4 + g)) = df1;
    f32x4 acc[NKT], dp[NKT];
#pragma unroll
    for (int k = 0; k < NKT; ++k) acc[k] = mfma(tile_frag(Ks, k, fo.a[0]), qf0, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
    for (int k = 0; k < NKT; ++k) acc[k] = mfma(tile_frag(Ks, k, fo.a[1]), qf1, acc[k]);
#pragma unroll
    for (int k = 0; k < NKT; ++k) dp[k] = mfma(tile_frag(Vs, k, fo.a[0]), df0, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
    for (int k = 0; k < NKT; ++k) dp[k] = mfma(tile_frag(Vs, k, fo.a[1]), df1, dp[k]);
    // acc[k][r] = raw S[query c][key k*16 + g*4 + r], dp[k][r] = dP of the same element
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < NKT; ++k) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = k * 16 + g * 4 + r;
        if constexpr (KEYMASK)
          acc[k][r] = ((kv.bits >> (4 * k + r)) & 1ull) ? (kv.uniform ? 0.f : acc[k][r]) : -INFINITY;
        else
          acc[k][r] = (key < Tk && (!CAUSAL || key <= qrow)) ? acc[k][r] : -INFINITY;
        m = fmaxf(m, acc[k][r]);
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    const float mk = m * kExp2;                    // key 0 always exists (KEYMASK: a visible key): m is finite
    float l = 0.f;
#pragma unroll
    for (int k = 0; k < NKT; ++k) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f(fmaf(acc[k][r], kExp2, -mk));
        acc[k][r] = p;
        l += p;
      }
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float linv = 1.f / l;
    uint64_t keep = 0;                             // DROP: bit 4 k + r = keep of key k*16 + g*4 + r for this lane's query
    if constexpr (DROP) {
      const uint64_t dgrp = (((uint64_t)(ctx * H + h) * drop.idx_qrep + qrow) << 6) | (uint64_t)g;
#pragma unroll
      for (int k = 0; k < NKT; ++k) {
        const uint32_t kb = lvl_drop::group_keep(drop.seed, drop.site, dgrp + 4 * k, drop.thr);
        keep |= (uint64_t)kb << (4 * k);
#pragma unroll
        for (int r = 0; r < 4; ++r) dp[k][r] = ((kb >> r) & 1u) ? drop.scale * dp[k][r] : 0.f;     // dPd -> dP
      }
    }
    float delta = 0.f;
#pragma unroll
    for (int k = 0; k < NKT; ++k) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[k][r] *= linv;
        delta = fmaf(acc[k][r], dp[k][r], delta);
      }
    }
    delta += __shfl_xor(delta, 16, 64);
    delta += __shfl_xor(delta, 32, 64);
#pragma unroll
    for (int k = 0; k < NKT; ++k) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        dp[k][r] = acc[k][r] * (dp[k][r] - delta);            // dS; masked keys: P = 0
        if constexpr (KEYMASK) dp[k][r] = kv.uniform ? 0.f : dp[k][r];      // the uniform row does not depend on the scores
        const int key = k * 16 + g * 4 + r;
        const int off = key * RS + ((((qcol >> 3) ^ (key & 7)) << 3) | (qcol & 7));
        if constexpr (DROP)
          Pi[off] = f32_to_bf16(((keep >> (4 * k + r)) & 1ull) ? drop.scale * acc[k][r] : 0.f);      // Pd
        else
          Pi[off] = f32_to_bf16(acc[k][r]);
        Di[off] = f32_to_bf16(dp[k][r]);
      }
    }
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NKT / 2; ++j) {
      uint4 pa;
      pa.x = pack_bf16x2(dp[2 * j][0], dp[2 * j][1]);
      pa.y = pack_bf16x2(dp[2 * j][2], dp[2 * j][3]);
      pa.z = pack_bf16x2(dp[2 * j + 1][0], dp[2 * j + 1][1]);
      pa.w = pack_bf16x2(dp[2 * j + 1][2], dp[2 * j + 1][3]);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const uint2 lo = tile_frag_tr(Ks, 2 * j, fo.tr[dt]);
        const uint2 hi = tile_frag_tr(Ks, 2 * j + 1, fo.tr[dt]);
        o[dt] = mfma(pa, make_uint4(lo.x, lo.y, hi.x, hi.y), o[dt]);
      }
    }
    // o[dt][r] = dQ[query g*4+r][channel dt*16 + c] / 0.125
    store_tile_rows<PrecBf16>(
        ot, o, 0.125f, lane, [&](int row) { return dq + ((size_t)ctx * qrep + q0 + row) * qs + h * 64; },
        [&](int row) { return q0 + row < qrep; });
    __syncthreads();
    // ---- phase B: the wave's own 64 keys against the round's 64 query rows -------------------------------------------
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int kt = wave * 4 + kk;
      if (kt * 16 < Tk) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const uint4 aP = tile_frag(Pi, kt, fo.a[ks]);       // key row c of the tile, queries ks*32 + g*8 .. +7
          const uint4 aD = tile_frag(Di, kt, fo.a[ks]);
          const int r0 = ks * 32 + g * 8;
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) {
            const uint2 olo = img_frag_tr(Oi, r0, dt * 16, lane), ohi = img_frag_tr(Oi, r0 + 4, dt * 16, lane);
            dV[kk][dt] = mfma(aP, make_uint4(olo.x, olo.y, ohi.x, ohi.y), dV[kk][dt]);
            const uint2 qlo = img_frag_tr(Qi, r0, dt * 16, lane), qhi = img_frag_tr(Qi, r0 + 4, dt * 16, lane);
            dK[kk][dt] = mfma(aD, make_uint4(qlo.x, qlo.y, qhi.x, qhi.y), dK[kk][dt]);
          }
        }
      }
    }
    __syncthreads();                               // the next round overwrites the images
  }
  // dK[kk][dt][r] = dK[key (wave*4+kk)*16 + g*4 + r][channel dt*16 + c] / 0.125, dV alike
  uint16_t* okb = dk + kvoff;
  uint16_t* ovb = dv + kvoff;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const int k0 = (wave * 4 + kk) * 16;
    if (k0 < Tk) {
      store_tile_rows<PrecBf16>(
          ot, dK[kk], 0.125f, lane, [&](int row) { return okb + (size_t)(k0 + row) * kvs; },
          [&](int row) { return k0 + row < Tk; });
      store_tile_rows<PrecBf16>(
          ot, dV[kk], 1.f, lane, [&](int row) { return ovb + (size_t)(k0 + row) * kvs; },
          [&](int row) { return k0 + row < Tk; });
    }
  }
}

template <bool DROP, bool CAUSAL, bool KEYMASK>
int launch_bwd(const RowsAttn& r, const void* dout, void* dq, void* dk, void* dv, hipStream_t st) {
  const size_t lds = ((size_t)4 * NKT * 16 * RS + (size_t)2 * QR * RS + (size_t)XW * 16 * OS) * sizeof(uint16_t);
  const AttnDrop drop = DROP ? AttnDrop{r.seed, r.site, lvl_drop::threshold(r.p), lvl_drop::scale_of(r.p), r.idx_qrep}
                             : AttnDrop{};
  if (int rc = lvl_allow_lds<cross_attn_bwd_mfma_kernel<DROP, CAUSAL, KEYMASK>>()) return rc;
  hipLaunchKernelGGL((cross_attn_bwd_mfma_kernel<DROP, CAUSAL, KEYMASK>), dim3((unsigned)(r.contexts * r.H)), dim3(64 * XW),
                     lds, st, (const uint16_t*)r.q, (size_t)r.q_stride, (const uint16_t*)r.k, (const uint16_t*)r.v,
                     (size_t)r.kv_stride, (size_t)r.kv_ctx_stride, (const uint16_t*)dout, (uint16_t*)dq, (uint16_t*)dk,
                     (uint16_t*)dv, r.Tk, r.H, r.qrep, drop, r.mask, (size_t)r.mask_ctx_stride);
  LVL_CHECK_LAUNCH("rows attention backward (mfma)");
  return LVL_OK;
}

}  // namespace

// The one launch site of cross_attn_bwd_mfma_kernel: the six instantiations the entries reach.
int lvl_launch_rows_attn_mfma_bwd(const RowsAttn& r, const void* dout, void* dq, void* dk, void* dv, hipStream_t st) {
  if (r.Tk > NKT * 16 || (r.causal && r.keymasked))
    return lvl_fail(LVL_EINVAL, "rows attention backward (mfma): Tk = %d beyond %d keys, or causal with a key mask", r.Tk,
                    NKT * 16);
  const bool drop = r.p > 0.f;
  if (r.keymasked)
    return drop ? launch_bwd<true, false, true>(r, dout, dq, dk, dv, st) : launch_bwd<false, false, true>(r, dout, dq, dk, dv, st);
  if (r.causal)
    return drop ? launch_bwd<true, true, false>(r, dout, dq, dk, dv, st) : launch_bwd<false, true, false>(r, dout, dq, dk, dv, st);
  return drop ? launch_bwd<true, false, false>(r, dout, dq, dk, dv, st) : launch_bwd<false, false, false>(r, dout, dq, dk, dv, st);
}

extern "C" int lvl_cross_attn_rows_bwd(const void* q, const void* kv, const void* dout, void* dq, void* dkv, int rows,
                                       int qrep, int Tk, int H, int dtype, void* stream) {
  LVL_REQUIRE(rows == 0 || (q && kv && dout && dq && dkv), "cross_attn_rows_bwd: null pointer");
  LVL_REQUIRE(rows >= 0 && qrep > 0 && rows % qrep == 0, "cross_attn_rows_bwd: bad shape rows=%d qrep=%d Tk=%d H=%d", rows,
              qrep, Tk, H);
  const int64_t D = (int64_t)H * 64;             // the image layout kv [ctx, Tk, 2D] = k | v as strides
  const RowsAttn r{q, kv, (const uint16_t*)kv + D, rows / qrep, qrep, Tk, H, D, 2 * D, (int64_t)Tk * 2 * D,
                   /*keymasked, mask, mask_ctx_stride*/ false, nullptr, 0, /*causal*/ false, /*seed, site, p*/ 0, 0, 0.f,
                   /*idx_qrep*/ qrep};
  if (int rc = lvl_rows_attn_check("cross_attn_rows_bwd", r)) return rc;
  LVL_REQUIRE(lvl_aligned16(q) && lvl_aligned16(kv) && lvl_aligned16(dout) && lvl_aligned16(dq) && lvl_aligned16(dkv),
              "cross_attn_rows_bwd: pointers must be 16-byte aligned");
  if (dtype != LVL_BF16 || Tk > NKT * 16)
    return lvl_fail(LVL_ENOSYS, "cross_attn_rows_bwd: built for bf16 and 1 <= Tk <= %d keys per context (got dtype %d, Tk=%d)",
                    NKT * 16, dtype, Tk);
  if (rows == 0) return LVL_OK;
  return lvl_launch_rows_attn_mfma_bwd(r, dout, dq, dkv, (uint16_t*)dkv + D, (hipStream_t)stream);
}

// backward of lvl_attn_rows_drop_fwd: dq laid out as q, dk and dv as k and v (same strides); dout [rows, H*64]
extern "C" int lvl_attn_rows_drop_bwd(const void* q, const void* k, const void* v, const void* dout, void* dq, void* dk,
                                      void* dv, int contexts, int qrep, int Tk, int H, int64_t q_stride, int64_t kv_stride,
                                      int64_t kv_ctx_stride, int causal, uint64_t seed, uint32_t site, float p, int dtype,
                                      void* stream) {
  LVL_REQUIRE(contexts == 0 || (q && k && v && dout && dq && dk && dv), "attn_rows_drop_bwd: null pointer");
  const RowsAttn r{q, k, v, contexts, qrep, Tk, H, q_stride, kv_stride, kv_ctx_stride,
                   /*keymasked, mask, mask_ctx_stride*/ false, nullptr, 0, causal != 0, seed, site, p, /*idx_qrep*/ qrep};
  if (int rc = lvl_rows_attn_check("attn_rows_drop_bwd", r)) return rc;
  LVL_REQUIRE(lvl_aligned16(q) && lvl_aligned16(k) && lvl_aligned16(v) && lvl_aligned16(dout) && lvl_aligned16(dq) &&
                  lvl_aligned16(dk) && lvl_aligned16(dv), "attn_rows_drop_bwd: pointers must be 16-byte aligned");
  if (dtype != LVL_BF16 || Tk > NKT * 16)
    return lvl_fail(LVL_ENOSYS, "attn_rows_drop_bwd: built for bf16 and 1 <= Tk <= %d keys per context (got dtype %d, Tk=%d)",
                    NKT * 16, dtype, Tk);
  if (contexts == 0) return LVL_OK;
  return lvl_launch_rows_attn_mfma_bwd(r, dout, dq, dk, dv, (hipStream_t)stream);
}
