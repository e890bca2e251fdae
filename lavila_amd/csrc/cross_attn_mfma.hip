// Decoder cross-attention for SEVERAL query rows per context on MFMA, bf16, gfx950 (lvl_cross_attn_rows_fwd, qrep >= 2:
// the sampled captions of one clip while decoding, or the positions of a teacher-forced caption;
// gpt2_gated.py:206-238,327-334 without a mask). One workgroup per (context, head): the head's keys and values
// (<= 256 x 64 each) are staged ONCE into the swizzled LDS images of the training kernels (attn_mfma_common.h), then
// each wave takes 16 query rows at a time:
//   S^T = K . Q^T      v_mfma_f32_16x16x32_bf16, K fragments from LDS, Q fragments straight from memory; all 16 key tiles
//                      stay in registers (64 VGPRs), so the softmax is exact single-pass
//   O   = P . V        P packed to bf16 in registers (two key tiles = one 32-deep contraction), V through the LDS
//                      transpose read (ds_read_tr16_b64): no transposed copy is staged
// The VALU form (cls_attn.hip) spends 1.3 us per extra query row on 8-lane dot products; here a row tile costs 64 MFMAs.
//
// The kernel is a template over DROP and CAUSAL (lvl_attn_rows_drop_fwd, the training decoder with attn_pdrop > 0); the
// <false, false> instantiation is lvl_cross_attn_rows_fwd's kernel, to the bit. Keys and values come through two pointers
// with a row and a context stride, so they are either the image keys | values [ctx, Tk, 2D] or the k and v thirds of the
// decoder's own qkv [B L, 3D] (qrep = Tk = L, CAUSAL: key j <= query i, masked like the Tk tail).
//   DROP: P = softmax(S) over all unmasked keys, Pd = keep ? P / (1 - p) : 0 rounded to bf16 where P is, O = Pd . V.
//         The mask is dropout.h's over e = (((ctx * H + h) * qrep + i) << 8) | j: the four keys a lane holds in one score
//         fragment (j = k*16 + g*4 + r) share one Philox call, generated where the fragment is packed; nothing is stored.
//         (The index takes drop.idx_qrep for qrep: the same number, except when a key-masked call computes a subset of
//         the query rows of a larger one.)
//
// Host side: every entry point of the rows attention (lvl_cross_attn_rows_*, lvl_attn_rows_drop_*, lvl_keymask_attn_*,
// lvl_keymask_attn_drop_*) describes its call as a RowsAttn (internal.h), runs lvl_rows_attn_check below and comes to
// lvl_launch_rows_attn_mfma_fwd, the one launch site of the kernel: it picks among the six instantiations that exist
// (<DROP> x <plain, CAUSAL, KEYMASK>). The backward has the same pair in cross_attn_bwd_mfma.hip.
#include "attn_mfma_common.h"
#include "dropout.h"
#include "internal.h"
#include "keymask.h"

using namespace attn_mfma;

namespace {

constexpr int XW = 4;          // waves per workgroup
constexpr int NKT = 16;        // key tiles of 16: up to 256 keys (the narrator pools every clip onto 256 image tokens)

struct AttnDrop {
  uint64_t seed;
  uint32_t site, thr;
  float scale;
  int idx_qrep;                // query rows per context in the element index: qrep, or the full call's when this call
                               // computes a subset of its rows (lvl_keymask_attn_drop_fwd)
};

// q rows at q + row * qs, keys at kp + ctx * kvctx + j * kvs (+ head), values at vp alike; out [rows, D]
// KEYMASK (lvl_keymask_attn_fwd): keys of a context are hidden by mask[ctx * mctx + key] == 0 (mask NULL: none); a context
// with no visible key gets the uniform distribution over its Tk keys
template <bool DROP, bool CAUSAL, bool KEYMASK = false>
__global__ __launch_bounds__(64 * XW) void cross_attn_mfma_kernel(const uint16_t* __restrict__ q, size_t qs,
                                                                  const uint16_t* __restrict__ kp,
                                                                  const uint16_t* __restrict__ vp, size_t kvs,
                                                                  size_t kvctx, uint16_t* __restrict__ out, int Tk, int H,
                                                                  int qrep, AttnDrop drop,
                                                                  const uint8_t* __restrict__ mask = nullptr,
                                                                  size_t mctx = 0) {
  extern __shared__ __align__(16) uint16_t xa_smem[];
  uint16_t* Ks = xa_smem;
  uint16_t* Vs = Ks + NKT * 16 * RS;
  uint16_t* Ot = Vs + NKT * 16 * RS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int h = blockIdx.x % H, ctx = blockIdx.x / H;
  const int D = H * 64;
  const size_t kvoff = (size_t)ctx * kvctx + h * 64;
  stage_rows2<PrecBf16, 64 * XW, NKT / 2>(Ks, kp + kvoff, kvs, nullptr, Vs, vp + kvoff, kvs, nullptr, NKT * 16, Tk, tid, 0);
  __syncthreads();
  constexpr float kScale = 0.125f, kExp2 = 0.125f * 1.4426950408889634f;
  const FragOff fo = frag_offsets(lane);
  uint16_t* ot = Ot + wave * 16 * OS;
  const int ntiles = (qrep + 15) >> 4;
  const KeyVis kv = key_visibility<KEYMASK>(mask, (size_t)ctx * mctx, Tk, g);
#pragma unroll 1
  for (int qt = wave; qt < ntiles; qt += XW) {
    const int qrow = qt * 16 + c;
    const uint16_t* qp = q + ((size_t)ctx * qrep + (qrow < qrep ? qrow : qrep - 1)) * qs + h * 64 + g * 8;
    const uint4 qf0 = *reinterpret_cast<const uint4*>(qp);
    const uint4 qf1 = *reinterpret_cast<const uint4*>(qp + 32);
    f32x4 acc[NKT];
#pragma unroll
    for (int k = 0; k < NKT; ++k) acc[k] = mfma(tile_frag(Ks, k, fo.a[0]), qf0, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
    for (int k = 0; k < NKT; ++k) acc[k] = mfma(tile_frag(Ks, k, fo.a[1]), qf1, acc[k]);
    // acc[k][r] = raw S[query c][key k*16 + g*4 + r]
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
    const float mk = m * kExp2;                    // key 0 always exists (KEYMASK: a visible key, see key_visibility): m is finite
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
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // element group of (this query, key tile k, lane group g): e >> 2 with e = (query id << 8) | key
    const uint64_t dgrp = (((uint64_t)(ctx * H + h) * (DROP ? drop.idx_qrep : qrep) + qrow) << 6) | (uint64_t)g;
#pragma unroll
    for (int j = 0; j < NKT / 2; ++j) {
      if constexpr (DROP) {                        // l above is the sum over ALL unmasked keys
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int k = 2 * j + t;
          const uint32_t keep = lvl_drop::group_keep(drop.seed, drop.site, dgrp + 4 * k, drop.thr);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[k][r] = ((keep >> r) & 1u) ? drop.scale * acc[k][r] : 0.f;
        }
      }
      uint4 pa;
      pa.x = pack_bf16x2(acc[2 * j][0], acc[2 * j][1]);
      pa.y = pack_bf16x2(acc[2 * j][2], acc[2 * j][3]);
      pa.z = pack_bf16x2(acc[2 * j + 1][0], acc[2 * j + 1][1]);
      pa.w = pack_bf16x2(acc[2 * j + 1][2], acc[2 * j + 1][3]);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const uint2 lo = tile_frag_tr(Vs, 2 * j, fo.tr[dt]);
        const uint2 hi = tile_frag_tr(Vs, 2 * j + 1, fo.tr[dt]);
        o[dt] = mfma(pa, make_uint4(lo.x, lo.y, hi.x, hi.y), o[dt]);
      }
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    // o[dt][r] = O[query g*4+r][channel dt*16 + c]: normalise, transpose through the wave's LDS tile, store whole rows
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float linv = __builtin_amdgcn_rcpf(__shfl(l, g * 4 + r, 64));
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) ot[(g * 4 + r) * OS + dt * 16 + c] = f32_to_bf16(o[dt][r] * linv);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {                  // same wave wrote and reads: in order, no barrier
      const int row = (lane >> 3) + 8 * k, ch = lane & 7;
      const uint4 v = *reinterpret_cast<const uint4*>(ot + row * OS + ch * 8);
      const int qq = qt * 16 + row;
      if (qq < qrep) *reinterpret_cast<uint4*>(out + ((size_t)ctx * qrep + qq) * D + h * 64 + ch * 8) = v;
    }
    (void)kScale;
  }
}

template <bool DROP, bool CAUSAL, bool KEYMASK>
int launch_fwd(const RowsAttn& r, void* out, hipStream_t st) {
  const size_t lds = ((size_t)2 * NKT * 16 * RS + (size_t)XW * 16 * OS) * sizeof(uint16_t);
  const AttnDrop drop = DROP ? AttnDrop{r.seed, r.site, lvl_drop::threshold(r.p), lvl_drop::scale_of(r.p), r.idx_qrep}
                             : AttnDrop{};
  if (int rc = lvl_allow_lds<cross_attn_mfma_kernel<DROP, CAUSAL, KEYMASK>>()) return rc;
  hipLaunchKernelGGL((cross_attn_mfma_kernel<DROP, CAUSAL, KEYMASK>), dim3((unsigned)(r.contexts * r.H)), dim3(64 * XW), lds,
                     st, (const uint16_t*)r.q, (size_t)r.q_stride, (const uint16_t*)r.k, (const uint16_t*)r.v,
                     (size_t)r.kv_stride, (size_t)r.kv_ctx_stride, (uint16_t*)out, r.Tk, r.H, r.qrep, drop, r.mask,
                     (size_t)r.mask_ctx_stride);
  LVL_CHECK_LAUNCH("rows attention forward (mfma)");
  return LVL_OK;
}

}  // namespace

int lvl_rows_attn_check(const char* who, const RowsAttn& r) {
  LVL_REQUIRE(r.contexts >= 0 && r.qrep > 0 && r.Tk > 0 && r.H > 0, "%s: bad shape contexts=%d qrep=%d Tk=%d H=%d", who,
              r.contexts, r.qrep, r.Tk, r.H);
  const int64_t D = (int64_t)r.H * 64;
  LVL_REQUIRE(r.q_stride >= D && r.kv_stride >= D && r.q_stride % 8 == 0 && r.kv_stride % 8 == 0 &&
                  r.kv_ctx_stride % 8 == 0 && r.kv_ctx_stride >= 0,
              "%s: strides must be multiples of 8 elements, rows at least H*64 apart", who);
  LVL_REQUIRE(r.mask == nullptr || r.mask_ctx_stride >= r.Tk, "%s: the mask's context stride must be at least Tk bytes", who);
  LVL_REQUIRE((int64_t)r.contexts * r.qrep * r.H < (1ll << 31), "%s: rows * heads must stay below 2^31", who);
  // the shape-generic key-masked kernels also size a grid by the keys
  LVL_REQUIRE(!r.keymasked || (int64_t)r.contexts * r.Tk * r.H < (1ll << 31), "%s: keys * heads must stay below 2^31", who);
  LVL_REQUIRE(!r.causal || r.qrep == r.Tk, "%s: the causal form needs qrep == Tk (got %d, %d)", who, r.qrep, r.Tk);
  LVL_REQUIRE(r.p >= 0.f && r.p < 1.f, "%s: p = %g must be in [0, 1)", who, (double)r.p);
  LVL_REQUIRE(r.idx_qrep >= r.qrep, "%s: idx_qrep = %d must be at least qrep = %d", who, r.idx_qrep, r.qrep);
  return LVL_OK;
}

// The one launch site of cross_attn_mfma_kernel: the six instantiations the entries reach.
int lvl_launch_rows_attn_mfma_fwd(const RowsAttn& r, void* out, hipStream_t st) {
  if (r.Tk > NKT * 16 || (r.causal && r.keymasked))
    return lvl_fail(LVL_EINVAL, "rows attention forward (mfma): Tk = %d beyond %d keys, or causal with a key mask", r.Tk,
                    NKT * 16);
  const bool drop = r.p > 0.f;
  if (r.keymasked) return drop ? launch_fwd<true, false, true>(r, out, st) : launch_fwd<false, false, true>(r, out, st);
  if (r.causal) return drop ? launch_fwd<true, true, false>(r, out, st) : launch_fwd<false, true, false>(r, out, st);
  return drop ? launch_fwd<true, false, false>(r, out, st) : launch_fwd<false, false, false>(r, out, st);
}

// The dropout-capable rows attention of the training decoder: q [contexts * qrep rows, stride q_stride], keys k and values
// v [contexts][Tk rows, stride kv_stride] with contexts kv_ctx_stride apart (strides in elements), out [rows, H*64].
extern "C" int lvl_attn_rows_drop_fwd(const void* q, const void* k, const void* v, void* out, int contexts, int qrep, int Tk,
                                      int H, int64_t q_stride, int64_t kv_stride, int64_t kv_ctx_stride, int causal,
                                      uint64_t seed, uint32_t site, float p, int dtype, void* stream) {
  LVL_REQUIRE(contexts == 0 || (q && k && v && out), "attn_rows_drop_fwd: null pointer");
  const RowsAttn r{q, k, v, contexts, qrep, Tk, H, q_stride, kv_stride, kv_ctx_stride,
                   /*keymasked, mask, mask_ctx_stride*/ false, nullptr, 0, causal != 0, seed, site, p, /*idx_qrep*/ qrep};
  if (int rc = lvl_rows_attn_check("attn_rows_drop_fwd", r)) return rc;
  LVL_REQUIRE(lvl_aligned16(q) && lvl_aligned16(k) && lvl_aligned16(v) && lvl_aligned16(out),
              "attn_rows_drop_fwd: pointers must be 16-byte aligned");
  if (dtype != LVL_BF16 || Tk > NKT * 16)
    return lvl_fail(LVL_ENOSYS, "attn_rows_drop_fwd: built for bf16 and 1 <= Tk <= %d keys per context (got dtype %d, Tk=%d)",
                    NKT * 16, dtype, Tk);
  if (contexts == 0) return LVL_OK;
  // no dropout, no mask, the image layout: exactly today's call (which has a kernel of its own for qrep == 1)
  const int64_t D = (int64_t)H * 64;
  if (!causal && p == 0.f && q_stride == D && kv_stride == 2 * D && kv_ctx_stride == (int64_t)Tk * 2 * D &&
      (const uint16_t*)v == (const uint16_t*)k + D)
    return lvl_cross_attn_rows_fwd(q, k, out, contexts * qrep, qrep, Tk, H, dtype, stream);
  return lvl_launch_rows_attn_mfma_fwd(r, out, (hipStream_t)stream);
}
