// What the attention files share: the CLS-row workspace contract (host and device) and the one declaration of every
// attention function that crosses a file boundary. Included by attention.hip and by every attn_*.hip -- the defining
// file too, so a definition that drifts from its declaration does not build.
#pragma once
#include "internal.h"

// THE CLS-ROW WORKSPACE CONTRACT.
// The cls token attends to every key of the sample, the divided-attention kernels each see one group of them: every
// workgroup that meets the cls row leaves a PARTIAL, and a small second kernel merges the partials of a (b, h) in slot
// order (lvl_launch_cls_combine forward, lvl_launch_cls_grad_finalize backward). One partial per frame in the space
// kernels, one per location chunk in the time kernels; every slot is written whole by its one writer, nothing is zeroed.
//   forward   ws = [B*H][nparts][kClsRec] f32: the record (m, l, un-normalised acc[64]) of the cls query over the
//             partial's keys
//   backward  ws = delta [B*H*T] f32 (dO.O per query; the time kernels leave it unused), then [B*H][nslots][kClsSlab]
//             f32: d cls q | d cls k | d cls v, 64 floats each
// nparts, nslots <= kClsMaxParts: lvl_workspace_floats (core.hip) sizes both workspaces for the cap through the two
// *_ws_floats functions below, and every launcher checks its own count against it (LVL_REQUIRE_CLS_PARTS).
constexpr int kClsRec = 66;
constexpr int kClsSlab = 192;
constexpr int kClsMaxParts = 64;

template <typename F>       // float or const float
__host__ __device__ __forceinline__ F* lvl_cls_rec(F* ws, int b, int h, int H, int nparts, int part) {
  return ws + (((size_t)b * H + h) * nparts + part) * kClsRec;
}
template <typename F>
__host__ __device__ __forceinline__ F* lvl_cls_slab(F* slabs, int b, int h, int H, int nslots, int slot) {
  return slabs + (((size_t)b * H + h) * nslots + slot) * kClsSlab;
}
struct ClsBwdWs { float* delta; float* slabs; };
inline ClsBwdWs lvl_cls_bwd_split(float* ws, int B, int H, int T) { return {ws, ws + (size_t)B * H * T}; }

inline int64_t lvl_cls_fwd_ws_floats(int64_t BH) { return BH * kClsMaxParts * kClsRec; }
// slabs = false: delta alone (the causal kernels have no cls row)
inline int64_t lvl_cls_bwd_ws_floats(int64_t BH, int64_t T, bool slabs) {
  return BH * T + (slabs ? BH * kClsSlab * kClsMaxParts : 0);
}

#define LVL_REQUIRE_CLS_PARTS(name, n) \
  LVL_REQUIRE((n) <= kClsMaxParts, "%s: %d cls partials per (b, h), the workspace holds %d", name, (int)(n), kClsMaxParts)

// Kernel families of the divided attention (attention.hip holds the table). One function type per role, so the table
// needs no adapters: a family that has no use for an argument (dq_part without a rider, dtype in the bf16-only time MFMA
// kernels) ignores it.
//   AttnOk        can the family run this shape / dtype (streaming kernels: and is it the shipped choice)
//   AttnPartRows  rows of dq column-sum partials [rows, H*64] the backward writes to dq_part when given one (the rider of
//                 the qkv bias gradient); 0: none for this shape
// lvl_space_stream_*: attn_space_stream.hip, key-tiled streaming kernels for large space groups. lvl_space_mfma_* and
// their causal variants lvl_text_mfma_*: the LDS-resident kernels, forward attn_space_mfma.hip, backward
// attn_space_bwd.hip. lvl_time_mfma_*: attn_time_mfma.hip. lvl_time_fast_*: attn_time.hip, register-tiled, forward and
// backward take the same shapes. lvl_generic_*: attn_generic.hip, any shape.
typedef bool AttnOk(int F, int N, int H, int dtype);
typedef int AttnPartRows(int B, int F, int N, int H);
typedef int AttnFwd(const void* qkv, void* out, float* lse, float* ws, int B, int F, int N, int H, int dtype,
                    hipStream_t st);
typedef int AttnBwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* ws,
                    float* dq_part, int B, int F, int N, int H, int dtype, hipStream_t st);
AttnOk lvl_space_stream_wanted, lvl_space_mfma_supported, lvl_space_mfma_bwd_supported, lvl_time_mfma_supported,
    lvl_time_fast_supported;
AttnPartRows lvl_space_mfma_bwd_dq_part_rows, lvl_time_fast_bwd_dq_part_rows;
AttnFwd lvl_space_stream_fwd, lvl_space_mfma_fwd, lvl_time_mfma_fwd, lvl_time_fast_fwd;
AttnBwd lvl_space_stream_bwd, lvl_space_mfma_bwd, lvl_time_mfma_bwd, lvl_time_fast_bwd;
bool lvl_text_mfma_supported(int L);
bool lvl_text_mfma_bwd_supported(int L, int dtype);
int lvl_text_mfma_fwd(const void* qkv, void* out, float* lse, int B, int L, int H, int dtype, hipStream_t st);
int lvl_text_mfma_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* ws,
                      int B, int L, int H, int dtype, hipStream_t st);
int lvl_generic_divided_fwd(const void* qkv, void* out, float* lse, int B, int F, int N, int H, int mode, int dtype,
                            hipStream_t st);
int lvl_generic_divided_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                            float* ws, int B, int F, int N, int H, int mode, int dtype, hipStream_t st);
int lvl_generic_causal_fwd(const void* qkv, void* out, float* lse, int B, int L, int H, int dtype, hipStream_t st);
int lvl_generic_causal_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                           float* ws, int B, int L, int H, int dtype, hipStream_t st);

// the merge kernels of the contract above (attn_space_mfma.hip, attn_space_bwd.hip); launch + launch check
int lvl_launch_cls_combine(const float* ws, void* out, float* lse, int B, int H, int nparts, int T, int dtype,
                           hipStream_t st);
int lvl_launch_cls_grad_finalize(const float* slabs, void* dqkv, int B, int T, int H, int nslots, int dtype,
                                 hipStream_t st);
