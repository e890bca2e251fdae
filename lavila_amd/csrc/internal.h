// The one declaration of every library-internal (non-ABI) function that is defined in one .hip file and called from
// another; definer and callers both include this, so they cannot drift apart. The attention files' own cross-file
// functions are in attn_internal.h.
#pragma once
#include "common.h"

int lvl_debug_late_mod();       // core.hip: test hook of the dynamic schedules (lvl_debug_late_workgroups), 0 = off

// slab / row-block counts and sizes that lvl_workspace_floats (core.hip) answers from
int lvl_ln_bwd_parts(), lvl_dp_dy_parts(), lvl_colsum_mid_rows();      // layernorm.hip
int lvl_gelu_bwd_row_blocks(), lvl_qkv_bias_row_blocks();              // elementwise.hip
int lvl_gate_bwd_parts();                                              // decode.hip
int64_t lvl_wgrad_workspace_floats(int64_t N, int64_t K);              // wgrad_mfma.hip
int64_t lvl_linear_tn_workspace_floats(int64_t M, int64_t N);          // gemm_tn_mfma.hip

// layernorm.hip: two-stage column reduction of partial slabs; _tail: zeros / a copy ride on the second stage
int lvl_launch_column_reduce(const float* part, int nparts, int width, int seg, float* mid, float* out0, float* out1,
                             float* out2, hipStream_t st);
int lvl_launch_column_reduce_tail(const float* part, int nparts, int width, int seg, float* mid, float* out0, float* out1,
                                  float* out2, float* zero_dst, const float* copy_src, float* copy_dst, int tail_n,
                                  hipStream_t st);
// elementwise.hip: column sums behind the gradient of the qkv Linear's bias
int64_t lvl_qkv_bias_ws_floats(int D);
int lvl_qkv_bias_sources(const void* dqkv, const void* dout, float* dbias, float* ws, int64_t rows, int D, int dtype,
                         bool zero_k, const float* v_src, hipStream_t st);
// gemm_tn_gelu.hip: one launch of the persistent TN GEMM with an exact-GELU epilogue (LVL_EPI_BIAS_GELU / _GELU_BWD /
// _BIAS_GELU_DERIV; f32: the f32-class mode), for lvl_linear_tn's dispatch
int lvl_launch_tn_gelu(const void* x, const void* w, const float* bias, void* y, void* aux_out, const void* aux_in,
                       float* colpart, int64_t M, int N, int K, uint32_t* sched, int epilogue, int f32, hipStream_t st);
// gemm_tn_edge.hip: the 64 / 128 / 192 columns behind the full tiles of lvl_linear_tn_ragged
int lvl_launch_tn_edge(const void* x, const void* w, const float* bias, void* y, int64_t M, int N, int K, int n_first,
                       hipStream_t st);
// wgrad_160.hip: the 160-family instantiations of the weight-gradient kernel; cfg counts from kFirstCfg160
int lvl_launch_wgrad_160(int cfg, int tiles_k, int ntiles, int S, const void* dy, const void* x, float* part, float* bpart,
                         int64_t M, int N, int K, unsigned* sched, hipStream_t st);
// clip_loss_mfma.hip
bool lvl_clip_mfma_supported(int E);
int lvl_clip_fwd_mfma(const void* img_all, const void* txt_all, const float* scale, int B, int G, int E, int row0,
                      float* stats, int32_t* argmax, float* logits, int dtype, hipStream_t st);
// The rows attention (one workgroup per (context, head), bf16, Tk <= 256) as its eight entry points describe a call:
// lvl_cross_attn_rows_fwd / _bwd, lvl_attn_rows_drop_fwd / _bwd, lvl_keymask_attn_fwd / _bwd, lvl_keymask_attn_drop_fwd /
// _bwd. q rows q_stride apart, keys k and values v rows kv_stride apart and contexts kv_ctx_stride apart (elements); the
// image layout kv [ctx, Tk, 2D] is q_stride = D, kv_stride = 2D, kv_ctx_stride = Tk * 2D, v = k + D.
struct RowsAttn {
  const void *q, *k, *v;
  int contexts, qrep, Tk, H;
  int64_t q_stride, kv_stride, kv_ctx_stride;
  bool keymasked;               // the key-masked kernels (the lvl_keymask_attn_* entries), also when mask is NULL
  const uint8_t* mask;          // [contexts] rows of Tk bytes, mask_ctx_stride apart, non-zero = visible; NULL: none hidden
  int64_t mask_ctx_stride;
  bool causal;                  // key j <= query i; needs qrep == Tk
  // the dropout site on the probabilities, p == 0: none. The mask of dropout.h over
  // e = ((((ctx * H + h) * idx_qrep + i) << 8) | j; idx_qrep is qrep, or the full call's when this one computes a subset
  // of its query rows
  uint64_t seed;
  uint32_t site;
  float p;
  int idx_qrep;
};
// cross_attn_mfma.hip: the shape, stride, < 2^31, causal, p and idx_qrep requirements of every entry; `who` names the entry
int lvl_rows_attn_check(const char* who, const RowsAttn& r);
// cross_attn_mfma.hip / cross_attn_bwd_mfma.hip: the one launch site of each direction; out / dout [rows, H*64], dq laid
// out as q, dk and dv as k and v. The caller has run the check and refused what is not bf16 with Tk <= 256.
int lvl_launch_rows_attn_mfma_fwd(const RowsAttn& r, void* out, hipStream_t st);
int lvl_launch_rows_attn_mfma_bwd(const RowsAttn& r, const void* dout, void* dq, void* dk, void* dv, hipStream_t st);
