/*
 * lavila_hip.h -- C ABI of liblavila_hip.so: the MI355X (gfx950) hot kernels of the LaViLa
 * dual-encoder pretraining path.
 *
 * The reference (facebookresearch/LaViLa) has no native layer: every entry point below replaces a
 * span of stock torch ops inside a reference Python function (cited per function, paths relative
 * to the reference root). The host-side mirror of the reference API (the lavila_amd python package) binds these
 * through ctypes; INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers + sizes; all pointers are DEVICE pointers (HBM) unless stated otherwise
 *   - `dtype` selects the activation element type: LVL_F32 (parity path) or LVL_BF16 (perf path);
 *     statistics, parameters (gamma/beta/bias/pos-embeds) and workspaces are always float32
 *   - row-major, innermost dimension contiguous, base pointers 16-byte aligned
 *   - sizes: row counts are int64_t and every offset that grows with the rows (or with the batch) is formed in 64 bits, so
 *     a tensor may exceed 2^31 elements / 4 GiB unless the entry point names a limit; the limits that exist are listed
 *     per entry point in DESIGN.md, "Operand-size limits" (the 4 GiB inputs of lvl_linear_tn are the one on the training path)
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous and stream-ordered,
 *     never allocates, never synchronises, and is hipGraph-capturable
 *   - return value: 0 on success, negative LVL_E* otherwise (lvl_last_error() gives the text);
 *     nothing is thrown across the boundary
 *   - head dimension is fixed at 64 (all CLIP_OPENAI_TIMESFORMER_* configs: 768/12 = 1024/16 = 64)
 */
#ifndef LAVILA_HIP_H
#define LAVILA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the entry points declared here are exported. */
#pragma GCC visibility push(default)

enum { LVL_F32 = 0, LVL_BF16 = 1, LVL_F16 = 2 /* lvl_clip_ingest's output only */ };
enum { LVL_OK = 0, LVL_EINVAL = -22, LVL_ENOSYS = -38, LVL_EHIP = -5 };
enum { LVL_ATTN_SPACE = 0, LVL_ATTN_TIME = 1, LVL_ATTN_CAUSAL = 2 /* lvl_attention_fast_path only */ };
enum { LVL_EPI_BIAS = 0, LVL_EPI_BIAS_QUICKGELU = 1, LVL_EPI_QUICKGELU_BWD = 2, LVL_EPI_BIAS_RESIDUAL = 3,
       LVL_EPI_BIAS_QUICKGELU_DERIV = 4, LVL_EPI_MUL_AUX_COLSUM = 5, LVL_EPI_BIAS_GELU = 6, LVL_EPI_GELU_BWD = 7,
       LVL_EPI_BIAS_GELU_DERIV = 8 };
/* activations of the narrator decoder's MLPs (lvl_act_inplace) */
enum { LVL_ACT_GELU_NEW = 0, LVL_ACT_SQRELU = 1, LVL_ACT_GELU_ERF = 2 };

/* library identification / diagnostics (host pointers) */
const char* lvl_version(void);
/* Test hook for the dynamic schedules of lvl_linear_tn / lvl_linear_wgrad (`sched` != NULL): from now on the workgroups
 * with blockIdx % mod == 1 of every such launch behave as if their compute unit had been held by another kernel for
 * the whole launch -- they start, find nothing left to do and sign off -- so that the take-over paths (tile queue /
 * chunk stealing) can be exercised deterministically on an idle GPU. mod = 0 switches it off. Results must not change
 * as long as mod does not divide 8 (blockIdx % 8 selects the XCD tile queue: an XCD whose workgroups ALL never work has
 * nobody to serve its queue -- a workgroup that is merely late serves it when it starts). */
int lvl_debug_late_workgroups(int mod);
/* Compute units the two persistent GEMM kernels (lvl_linear_tn, lvl_linear_wgrad: one workgroup per CU holding the
 * whole register file) size their grids for. 0 (default) = every CU of the device; a multiple of 8 below that leaves
 * the remaining CUs to whatever runs beside the step (e.g. the channel workgroups of an RCCL collective), which
 * otherwise force a whole extra round of tiles (tools/probe_cu_contention.py). Process-wide; call before sizing
 * workspaces (lvl_workspace_floats("linear_wgrad") depends on it). Nothing in the reference corresponds to it. */
int lvl_set_compute_units(int n);
/* MFMA shape of lvl_linear_tn's K loop for bf16 results, epilogues 0-5 (lvl_linear_tn_ragged included): 32 =
 * v_mfma_f32_32x32x16_bf16, 16 = v_mfma_f32_16x16x32_bf16, 0 (default) = the library's own choice per (N, K, epilogue),
 * taken from measurement (profiles/gemm_mfma_shape.txt). Anything else is refused with LVL_EINVAL and changes nothing.
 * Process-wide. The f32-class mode (LVL_F32) and the exact-GELU epilogues 6-8 run on 32x32x16 whatever is set. The two
 * shapes return the same results, bit for bit: the MFMAs of both give the same accumulators for a K block (measured on
 * gfx950, tests/test_gpu_gemm_mfma_shape.py), and the column sums of epilogues 2 / 5 are formed in one order. */
int lvl_set_gemm_mfma_shape(int shape);
const char* lvl_last_error(void);
/* number of float32 workspace elements a call needs (host-side query, no device work) */
int64_t lvl_workspace_floats(const char* op, int64_t rows, int64_t cols);

/* ---- LayerNorm (optionally fused with the residual add that feeds it) ------------------------------
 * replaces F.layer_norm in ln_pre (timesformer.py:263-264,365-366; eps 1e-5), norm1/2/3 + norm
 * (timesformer.py:247,153,166,169,277,377; eps 1e-6), text ln_1/ln_2/ln_final
 * (openai_model.py:187,193; models.py:106,156; eps 1e-5), and -- when x2/xbias are given -- the
 * residual adds of SpaceTimeBlock.forward (timesformer.py:183,192,196) and
 * ResidualAttentionBlock.forward (openai_model.py:206-216) that produce the LayerNorm input.
 *
 * forward:  s = x (+ x2) (+ xbias);  y = (s - mean(s)) * rstd(s) * gamma + beta
 *   x, x2 (nullable), y: [rows, cols] dtype; xbias (nullable), gamma, beta: [cols] f32;
 *   s_out (nullable): [rows, cols] dtype, receives s (rounded to dtype; the statistics then use the
 *   rounded value so forward and backward agree); mean, rstd (nullable): [rows] f32.
 * backward: with s recomputed as x (+ x2) (+ xbias) exactly as in forward (pass the saved s_out as x
 *   and x2 = xbias = NULL when it was kept):
 *   dx = rstd * (dy*gamma - mean(dy*gamma) - shat * mean(dy*gamma*shat)) (+ dadd)
 *   dgamma = sum_rows dy*shat, dbeta = sum_rows dy, dxsum (nullable) = sum_rows dx (= d xbias).
 *   dadd (nullable): [rows, cols] dtype, extra gradient arriving at s through s_out.
 *   dx_plain (nullable): when given, receives the normalisation's own input gradient WITHOUT dadd (and dxsum sums
 *   that one), while dx = dx_plain + dadd: the two-consumer case of the odd residual wiring of SpaceTimeBlock
 *   (timesformer.py:183-196: x feeds x + time_out AND x + space_out), one pass instead of a separate add.
 * cols % 8 == 0, cols <= 4096. bwd workspace: lvl_workspace_floats("layernorm_bwd", rows, cols). */
int lvl_layernorm_fwd(const void* x, const void* x2, const float* xbias, const float* gamma,
                      const float* beta, void* s_out, void* y, float* mean, float* rstd,
                      int64_t rows, int cols, float eps, int dtype, void* stream);
int lvl_layernorm_bwd(const void* dy, const void* x, const void* x2, const float* xbias,
                      const float* gamma, const float* mean, const float* rstd, const void* dadd,
                      void* dx, void* dx_plain, float* dgamma, float* dbeta, float* dxsum, float* ws,
                      int64_t rows, int cols, int dtype, void* stream);

/* ---- LayerNorm on the float32 residual stream under autocast: every operand in the dtype it has -------
 * The two calls above on a float32 stream x (s_out, dadd, dx: float32) whose branch x2 and normalised rows are bf16:
 * what `lvl_layernorm_fwd(LVL_F32)` on the widened branch followed by one rounding of y to bf16 gives, and what
 * `lvl_layernorm_bwd(LVL_F32)` on the widened dy followed by one rounding of the branch gradient gives -- to the bit,
 * without the widening and narrowing passes (the reference's AMP keeps the stream float32: timesformer.py:183-196,
 * 353-366).
 * forward:  x f32, x2 (nullable) bf16, xbias (nullable), gamma, beta f32; the row is x, += x2, += xbias in f32;
 *   s_out (nullable) f32 receives it, y bf16 is the f32 result rounded once (nearest even); mean, rstd as above.
 * backward: dy bf16, x f32, x2 (nullable) bf16, dadd (nullable) f32; dx f32 = the normalisation's input gradient
 *   (+ dadd); dx2 (nullable) bf16 = dx rounded once, or with LVL_LN_PLAIN that gradient WITHOUT dadd rounded once
 *   (dx_plain above; dxsum then sums that one). dgamma, dbeta, dxsum (nullable) sum the float32 values, over the same
 *   partial slabs as lvl_layernorm_bwd: bit-equal to its LVL_F32 results. ws: lvl_workspace_floats("layernorm_bwd").
 * flags: LVL_LN_GENERAL sends the call to the general kernel where an exact-width one exists (512, 768, 1024
 *   columns; the two agree to the bit); LVL_LN_PLAIN (backward only, needs dx2) as above.
 * cols, alignment and rows == 0 as lvl_layernorm_fwd / lvl_layernorm_bwd. */
enum { LVL_LN_PLAIN = 1, LVL_LN_GENERAL = 2 };
int lvl_layernorm_fwd_mixed(const float* x, const void* x2, const float* xbias, const float* gamma,
                            const float* beta, float* s_out, void* y, float* mean, float* rstd,
                            int64_t rows, int cols, float eps, int flags, void* stream);
int lvl_layernorm_bwd_mixed(const void* dy, const float* x, const void* x2, const float* xbias,
                            const float* gamma, const float* mean, const float* rstd, const float* dadd,
                            float* dx, void* dx2, float* dgamma, float* dbeta, float* dxsum, float* ws,
                            int64_t rows, int cols, int flags, void* stream);

/* ---- Stochastic depth: per-sample scaled residual add + LayerNorm ------------------------------------
 * replaces `x = x + self.drop_path(branch)` followed by the next LayerNorm in SpaceTimeBlock.forward
 * (timesformer.py:192,196; timm's DropPath: branch * bernoulli(keep) / keep, one draw per sample).
 *
 * forward:  s = res + c_b * (y + ybias), c_b = scale[row / rows_per_sample];  h = LayerNorm(s) * gamma + beta
 *   res, y, s_out, h_out: [rows, cols] dtype; ybias (nullable), gamma, beta: [cols] f32; scale:
 *   [rows / rows_per_sample] f32 (device memory; the values the caller drew, 0 or 1 / keep); mean, rstd: [rows] f32.
 *   Per element v = fma(c, y, res); v = fma(c, ybias, v), rounded once to dtype when stored to s_out; the
 *   statistics are those of the rounded value (as lvl_layernorm_fwd with s_out). Hence c = 1 gives
 *   lvl_layernorm_fwd(res, y, ybias)'s s, h, mean and rstd to the bit, and c = 0 gives s = res to the bit and
 *   the plain LayerNorm of res. Rows of dropped samples are read like any other row.
 * backward: from dh, the kept s, the statistics and an optional dadd (the gradient reaching s through s_out):
 *   ds [rows, cols] = d res, dgamma, dbeta: lvl_layernorm_bwd(dh, s, dadd)'s dx, dgamma, dbeta to the bit;
 *   dy [rows, cols] = c_b * ds (the stored ds, rounded once more); dysum (nullable) [cols] f32 = the column
 *   sums of dy as stored (= d ybias, and the column-sum token of y), from partial slabs in a fixed order.
 *   ws: lvl_workspace_floats("droppath_add_layernorm_bwd", rows, cols).
 * cols % 8 == 0, cols <= 4096, rows % rows_per_sample == 0, rows < 2^32; rows == 0 is a no-op (the backward then zeroes
 * dgamma, dbeta and dysum). No allocation, no synchronisation, no atomics; hipGraph-capturable. */
int lvl_droppath_add_layernorm_fwd(const void* res, const void* y, const float* ybias, const float* scale,
                                   const float* gamma, const float* beta, void* s_out, void* h_out, float* mean,
                                   float* rstd, int64_t rows, int64_t rows_per_sample, int cols, float eps,
                                   int dtype, void* stream);
int lvl_droppath_add_layernorm_bwd(const void* dh, const void* s, const float* gamma, const float* mean,
                                   const float* rstd, const float* scale, const void* dadd, void* ds, void* dy,
                                   float* dgamma, float* dbeta, float* dysum, float* ws, int64_t rows,
                                   int64_t rows_per_sample, int cols, int dtype, void* stream);

/* ---- LayerNorm output, rebuilt (selective activation recompute) -----------------------------------
 * y = (s - mean[row]) * rstd[row] * gamma + beta with s = x (+ x2) (+ xbias) formed as lvl_layernorm_fwd
 * forms it, and mean / rstd the statistics that call returned: y equals that call's y to the bit (pass
 * its s_out as x and x2 = xbias = NULL when the sum was kept). No reductions: one read of the operands,
 * one write of y. Operand conventions, alignment and cols limits of lvl_layernorm_fwd; mean, rstd: [rows]
 * f32, required. Used in backward in front of the weight-gradient GEMM that reads a LayerNorm output which
 * the forward did not keep (norm3 / norm1 / norm2 of SpaceTimeBlock, timesformer.py:183-196). */
int lvl_layernorm_apply(const void* x, const void* x2, const float* xbias, const float* gamma,
                        const float* beta, const float* mean, const float* rstd, void* y,
                        int64_t rows, int cols, int dtype, void* stream);

/* ---- QuickGELU of a kept pre-activation (selective activation recompute) ----------------------------
 * a = u * sigmoid(1.702 u) with the arithmetic of lvl_linear_tn's LVL_EPI_BIAS_QUICKGELU epilogue, whose
 * aux_out is u: a equals that call's y to the bit (bf16: the activation of the bf16 value; f32: of the
 * f32 value). Mlp.act of timesformer.py:52-54, rebuilt in front of fc2's weight-gradient GEMM instead of
 * kept. u, a: [rows, cols] dtype, 16-byte aligned; cols % 8 == 0. Not lvl_bias_quickgelu_fwd, whose
 * sigmoid is a different expression. */
int lvl_quickgelu_apply(const void* u, void* a, int64_t rows, int cols, int dtype, void* stream);

/* ---- bias + QuickGELU --------------------------------------------------------------------------
 * a = (u + bias) * sigmoid(1.702 (u + bias)); replaces the bias add of Mlp.fc1 / mlp.c_fc and
 * QuickGELU.forward (openai_model.py:177-179; timesformer.py:52-54). u,a,da,du: [rows, cols] dtype;
 * bias,dbias: [cols] f32 (bias may be NULL -> treated as 0, dbias may be NULL). cols % 8 == 0.
 * bwd workspace: lvl_workspace_floats("bias_quickgelu_bwd", rows, cols). */
int lvl_bias_quickgelu_fwd(const void* u, const float* bias, void* a, int64_t rows, int cols,
                           int dtype, void* stream);
int lvl_bias_quickgelu_bwd(const void* da, const void* u, const float* bias, void* du, float* dbias,
                           float* ws, int64_t rows, int cols, int dtype, void* stream);

/* ---- patch embedding, gather side ----------------------------------------------------------------
 * video [B,C,F,H,W] f32 (frame_major = 0: the batch contract of datasets.py:360-387, what
 * SpaceTimeTransformer.forward receives, timesformer.py:384-390) or [B,F,C,H,W] f32 (frame_major = 1:
 * what forward_features receives, timesformer.py:345-348, the narrator's entry narrator.py:74)
 * -> patch matrix [B*F*N, C*P*P] dtype, rows frame-major then (py,px), columns (c,i,j) = Conv2d weight
 * flattening. Replaces permute(0,2,1,3,4).contiguous() (timesformer.py:387) and the im2col half of
 * nn.Conv2d(k=stride=P) (timesformer.py:77,79-84); the contraction with the [D, C*P*P] weight is a
 * plain GEMM. H % P == 0, W % P == 0. */
int lvl_patchify(const float* video, void* patches, int B, int C, int F, int H, int W, int P,
                 int frame_major, int dtype, void* stream);

/* ---- clip ingest: decoded uint8 frames -> the model's input ---------------------------------------------
 * Replaces the per-sample host transform of the reference drivers (main_pretrain.py:269-283: Permute([3,0,1,2]) ->
 * RandomResizedCrop, or Resize + CenterCrop -> NormalizeVideo, on float frames holding the integers 0..255) and the
 * float32 clip that crosses PCIe behind it; torchvision 0.11.2 semantics for tensors: bilinear, half-pixel centres,
 * align_corners=False, NO antialiasing.
 * frames: uint8, logical [B,F,H,W,3] (RGB, channel last), pixel stride 3 bytes; clip_stride / frame_stride / row_stride
 *   are byte strides (row >= 3 W, frame >= one frame's extent, clip >= one clip's extent; no alignment is required and
 *   offsets are 64-bit, so a clip may begin beyond 2^31 bytes).
 * params: int32 [B,8] = {top, left, h, w, Ry, Rx, sy, sx} per sample (16-byte aligned): the region
 *   [top, top+h) x [left, left+w) of every frame of clip b is resized to Ry x Rx and the S x S window at (sy, sx) of
 *   that is taken. flip (nullable): int32 [B], non-zero mirrors the window along x. Per axis, in float32 with every
 *   operation rounded on its own (n = region extent, R = resized extent, o = output index, sh = window offset):
 *     scale = (float)n / (float)R;  s = max(scale * ((float)(o + sh) + 0.5f) - 0.5f, 0)
 *     i0 = min((int)s, n-1);  i1 = min(i0+1, n-1);  lam = s - (float)i0
 *     v = (1-lam_y) * ((1-lam_x) p00 + lam_x p01) + lam_y * ((1-lam_x) p10 + lam_x p11);  y = (v - mean_c) / std_c
 *   (IEEE subtraction, correctly rounded division), stored round-to-nearest-even. The blocks live on the device, so the
 *   library cannot refuse a malformed one: the kernel forces every block into the frame (memory safety only) and the host
 *   layer (lavila_amd.ingest.validate_params) refuses it before the launch. Refused here (LVL_EINVAL): S odd or not a
 *   multiple of P, P odd, overlapping strides, std <= 0, ld odd or below 3 P P, unknown dtype.
 * lvl_clip_ingest: clip [B,3,F,S,S], dtype LVL_F32 / LVL_BF16 / LVL_F16.
 * lvl_clip_ingest_patches: patches [B*F*(S/P)^2, ld], dtype LVL_F32 / LVL_BF16: bit for bit what lvl_patchify writes from
 *   lvl_clip_ingest's float32 clip, in columns 0 .. 3 P P; columns 3 P P .. ld are written as zeros (ld = 640 gives the
 *   14 x 14 towers' GEMM operand without a pad copy). Both share one device function per value. */
int lvl_clip_ingest(const void* frames, const int32_t* params, const int32_t* flip, void* clip, int B, int F, int H, int W,
                    int S, int64_t clip_stride, int64_t frame_stride, int64_t row_stride, float mean0, float mean1,
                    float mean2, float std0, float std1, float std2, int dtype, void* stream);
int lvl_clip_ingest_patches(const void* frames, const int32_t* params, const int32_t* flip, void* patches, int B, int F,
                            int H, int W, int S, int P, int64_t ld, int64_t clip_stride, int64_t frame_stride,
                            int64_t row_stride, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                            int dtype, void* stream);

/* ---- token assembly: cls concat + positional/temporal embedding add --------------------------------
 * x[b,0,:] = cls + pos[0];  x[b,1+f*N+n,:] = pe[b,f*N+n,:] + pos[1+n] + temporal[f]
 * (timesformer.py:353-364). pe: [B,F*N,D] dtype; cls: [D], pos: [N+1,D], temporal: [>=F,D] f32;
 * x: [B,1+F*N,D] dtype. D % 8 == 0. */
int lvl_embed_tokens_fwd(const void* pe, const float* cls, const float* pos, const float* temporal,
                         void* x, int B, int F, int N, int D, int dtype, void* stream);
/* lvl_embed_tokens_bwd (round 5): the parameter gradients of the token assembly from dx [B, 1 + F N, D] (autograd of
 * timesformer.py:353-366): dpos [N + 1, D] f32 (row 0 = the cls position = d cls_token, row 1 + n summed over batch and
 * frames), dtem [tem_rows, D] f32 (row f summed over batch and locations; rows >= F zero). One pass over dx + a small
 * second stage; d(patch embeddings) is dx[:, 1:] itself. ws: lvl_embed_tokens_bwd_ws(F, N, D) floats. */
int64_t lvl_embed_tokens_bwd_ws(int F, int N, int D);
int lvl_embed_tokens_bwd(const void* dx, float* dpos, float* dtem, float* ws, int B, int F, int N, int D, int tem_rows,
                         int dtype, void* stream);

/* ---- text tower: token + positional embedding (round 6) ------------------------------------------------
 * x[b, l, :] = table[tokens[b, l], :] + pos[l, :]   (CLIP.encode_text, models.py:152-153: `self.token_embedding(text)`
 * + `self.positional_embedding`; under autocast the sum is rounded once to `dtype`). tokens: int64, row stride
 * tok_stride elements (a `text[:, :L]` view of the [B, 77] batch is read in place), ids clamped to [0, V); table [V, W],
 * pos [>= L, W] f32; x [B, L, W] dtype. W % 4 == 0 (forward), W % 8 == 0 (backward). B * L < 2^31 token rows (both calls:
 * LVL_EINVAL otherwise); x and dx may exceed 2^31 elements.
 * lvl_text_embed_bwd: autograd of the same two lines -- d table [V, W] f32 (= nn.Embedding's dense backward: row v is the
 * sum of the dx rows whose token is v, added in a fixed order -- eight contiguous row ranges, ascending inside each; rows of
 * unused ids zero) and d pos [ctx, W] f32
 * (row l = sum over the batch, rows >= L zero) -- without a sort, without float atomics and without memset nodes (torch's
 * embedding_dense_backward sorts with rocPRIM above 3072 rows, whose histogram memsets become unreliable memset NODES in a
 * replayed hipGraph). ws: lvl_text_embed_bwd_ws(B, L, V) int32 words. W <= 2048.
 * dtable or dpos may be NULL (a frozen parameter): a NULL dtable skips the [V, W] zero-fill, the census and the table
 * kernel (ws is then unused and may be NULL too), a NULL dpos skips the positional kernel; both NULL is LVL_EINVAL. */
int lvl_text_embed_fwd(const int64_t* tokens, int64_t tok_stride, const float* table, const float* pos, void* x, int B,
                       int L, int W, int V, int dtype, void* stream);
int64_t lvl_text_embed_bwd_ws(int B, int L, int V);
int lvl_text_embed_bwd(const void* dx, const int64_t* tokens, int64_t tok_stride, float* dtable, float* dpos, int* ws,
                       int B, int L, int W, int V, int ctx, int dtype, void* stream);

/* ---- divided space-time attention core ---------------------------------------------------------------
 * Everything in VarAttention.forward between the qkv Linear and the proj Linear
 * (timesformer.py:110-140 incl. attn() :35-39): head split, q *= 64^-0.5, CLS query over all T
 * keys, patch queries grouped per frame (LVL_ATTN_SPACE: N queries x [cls + N] keys) or per
 * location (LVL_ATTN_TIME: F queries x [cls + F] keys), softmax in f32, heads merged.
 * qkv: [B,T,3*H*64] dtype (T = 1+F*N; q|k|v thirds, head-major inside each third);
 * out/dout: [B,T,H*64] dtype; lse: [B,H,T] f32 (log-sum-exp of every query row, saved for backward);
 * dqkv: [B,T,3*H*64] dtype. Workspaces (f32): fwd lvl_workspace_floats("divided_attn_fwd", B*H, T)
 * (partial records of the CLS row), bwd lvl_workspace_floats("divided_attn_bwd", B*H, T) (delta + up to 64 partial
 * records [192] f32 per (b, h) of the cls token's d(q|k|v), one per frame / location chunk, summed in slot order: the
 * backward has no floating-point atomics and is run-to-run bit-identical since round 6). */
int lvl_divided_attn_fwd(const void* qkv, void* out, float* lse, float* ws, int B, int F, int N,
                         int H, int mode, int dtype, void* stream);
int lvl_divided_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse,
                         void* dqkv, float* ws, int B, int F, int N, int H, int mode, int dtype,
                         void* stream);
/* Every attention entry point of this header (divided, causal, cls-only, rows / cross, pooler, decode, key-masked) is
 * pinned by tests/test_gpu_attention_shift.py to finite and accurate results for any finite bf16 or f32 scores -- rows
 * shifted by up to +-120 over key staircases, lse from below -89 to above +280 -- padded and hidden keys included. */

/* host-side query: 1 if a bf16 call of this shape runs on the MFMA / register-tiled attention kernels (forward and
 * backward), 0 if it falls to the shape-generic kernels (any shape, correct, much slower). mode: LVL_ATTN_SPACE /
 * LVL_ATTN_TIME with (F, N, H), or LVL_ATTN_CAUSAL with N = L. The Python layer logs one warning per slow shape. */
int lvl_attention_fast_path(int mode, int F, int N, int H);
/* The same query for FLOAT32 tensors (the parity configuration, north_star "within 1e-3 fp32"): 1 if the call runs on
 * the f32-class instantiations of the fast kernels -- the MFMA kernels with every operand as hi/lo bf16 images and three
 * MFMAs per product (space groups up to 272 / 288 keys forward / backward, causal text up to 272 / 256 tokens), the
 * register-tiled time kernels with float32 rows (1-4, 8, 16 frames) -- 0 if it falls to the shape-generic kernels.
 * lvl_debug_f32_generic(1) (or LAVILA_F32_GENERIC=1 in the environment) sends every float32 attention call to the
 * generic kernels: the A/B switch of the parity tests. */
int lvl_attention_fast_path_f32(int mode, int F, int N, int H);
int lvl_debug_f32_generic(int on);
/* Space groups of more than 288 keys (TSF-L/14 at 336: 577 per frame; float32: more than 272) run on KEY-TILED STREAMING
 * kernels (csrc/attn_space_stream.hip: a workgroup owns 128 queries -- or keys, in the dK/dV kernel -- and streams the
 * other side through double-buffered 64-row LDS images; online softmax forward, lse-recomputed P backward) instead of
 * keeping the whole group LDS-resident with one workgroup per compute unit. Test / measurement hook: mode 1 = streaming
 * kernels for EVERY space group, -1 = never (the LDS-resident kernels as in round 3: forward up to 592 keys, backward up
 * to 577, larger groups on the generic kernels), 0 = the shipped choice. Results agree to rounding (bf16) / f32
 * summation order. */
int lvl_debug_space_stream(int mode);
/* Measurement hook, bf16 streaming kernels: bit 0 = the forward's 3-workgroup cut with a three-stage LDS-DMA ring (default:
 * 4 workgroups per compute unit, two stages); bit 2 = register staging instead of the LDS-DMA rings (all three kernels;
 * bit 0 then selects the forward's 4-workgroup register-staged cut). Same results. */
int lvl_debug_stream_variant(int v);
/* The "fp8 MFMA QK^T path" BASELINE.json names for TSF-L/14 at 336 (configs[3]): on = the streaming space kernels (bf16
 * tensors) compute their score products q.k with v_mfma_f32_16x16x32_fp8_fp8 on q / k fragments rounded to OCP e4m3 in
 * registers (saturating at +-448), forward AND the backward's recomputation of P, so lse and P stay consistent; every
 * other product (P V, dP, dQ, dK, dV) stays a bf16 MFMA, tensors stay bf16. Off by default (LAVILA_FP8_QK=1 in the
 * environment turns it on at first use): e4m3 scores cost accuracy and, at head dim 64, buy no time.
 * Groups the streaming kernels do not take (<= 288 keys, unless lvl_debug_space_stream(1)) and float32 tensors are
 * unaffected. */
int lvl_set_fp8_qk(int on);
/* Test hook: how many lvl_divided_attn_* / lvl_causal_attn_* calls of this process were served by the shape-generic
 * kernels so far (reset != 0: read and clear). */
int lvl_debug_generic_attention_calls(int reset);

/* ---- causal self-attention core of the text tower -------------------------------------------------------
 * nn.MultiheadAttention core with the additive causal mask (openai_model.py:196-198,
 * models.py:131-137) on packed qkv [B,L,3*H*64] (batch-major; the reference's LND permutes
 * models.py:153,155 are folded away). out: [B,L,H*64]; lse: [B,H,L].
 * bwd workspace: lvl_workspace_floats("causal_attn_bwd", B*H, L). */
int lvl_causal_attn_fwd(const void* qkv, void* out, float* lse, int B, int L, int H, int dtype,
                        void* stream);
int lvl_causal_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse,
                        void* dqkv, float* ws, int B, int L, int H, int dtype, void* stream);

/* ---- contrastive (InfoNCE) head ------------------------------------------------------------------------------
 * Slab formulation of CLIPLoss.forward (loss.py:69-118): this rank owns global rows
 * [row0, row0+B). Direction 0: logits_per_image rows = (scale*img_local) @ txt_all^T; direction 1:
 * logits_per_text rows = (scale*txt_local) @ img_all^T (loss.py:78-79,92-93).
 * img_all/txt_all: [G,E] dtype (rank-ordered all-gather, distributed_utils.py:88); the local slabs
 * are rows [row0,row0+B) of them. E % 8 == 0. scale: DEVICE pointer to exp(logit_scale) (1 float, so
 * the host never synchronises on it).
 * stats: [2,B,4] f32 = {lse, diag logit, sum_j softmax_j * logit_j, max logit};
 * argmax: [2,B] int32 (first maximal column -- torch.argmax tie rule; loss.py:113);
 * logits (optional, may be NULL): [2,B,G] f32 slab of the scaled logits (for parity checks).
 * bwd: lse_all [2,G] f32 = gathered row LSEs of both directions; upstream (nullable): DEVICE pointer
 * to d(objective)/d(loss); coef: host factor mult/(2G). Writes coef*upstream*d(sum of both CE
 * sums)/d(img_local | txt_local): [B,E] f32. No gradient collective is needed.
 * rows_only != 0: CLIPLoss(local_loss=True) without gather_with_grad (loss.py:34-43,86-88): the gathered
 * partner rows are constants, so each local row receives only the gradient of its own two cross-entropies
 * (only the local entries of lse_all are read; coef = 1/(2B)). */
int lvl_clip_loss_fwd(const void* img_all, const void* txt_all, const float* scale, int B, int G,
                      int E, int row0, float* stats, int32_t* argmax, float* logits, int dtype,
                      void* stream);
int lvl_clip_loss_bwd(const void* img_all, const void* txt_all, const float* lse_all,
                      const float* scale, const float* upstream, float coef, int B, int G, int E,
                      int row0, int rows_only, float* dimg, float* dtxt, int dtype, void* stream);

/* ---- contrastive head with per-pair temperature (SSLCLIPLoss, loss.py:121-217) ---------------------------
 * Same slab structure as lvl_clip_loss_*; ind_all: [G] int32 gt_indicators in rank order (1 = ground-truth
 * narration, 0 = pseudo-label); scales3: DEVICE pointer to {pseudo, sqrt(pseudo*real), real}; the pair (i,j)
 * uses scales3[ind[i] + ind[j]] (loss.py:160-166,172-178). Every indicator is read as ind[x] != 0: any non-zero
 * value counts as 1, so no value can index scales3 out of range.
 * stats: [2,B,8] f32 = {lse, diag logit, E0, E1, E2, diag dot, max logit, 0} with
 * Ek = sum_{j: ind[i]+ind[j]==k} softmax_j * (a_i . b_j): d(loss)/d(scales3[k]) follows without another pass. */
int lvl_ssl_clip_loss_fwd(const void* img_all, const void* txt_all, const int32_t* ind_all,
                          const float* scales3, int B, int G, int E, int row0, float* stats,
                          int32_t* argmax, float* logits, int dtype, void* stream);
int lvl_ssl_clip_loss_bwd(const void* img_all, const void* txt_all, const int32_t* ind_all,
                          const float* lse_all, const float* scales3, const float* upstream, float coef,
                          int B, int G, int E, int row0, float* dimg, float* dtxt, int dtype,
                          void* stream);

/* ---- max-margin ranking losses of the retrieval fine-tune (loss.py:256-367) ---------------------------------
 * MaxMarginRankingLoss (loss.py:267-312) and AdaptiveMaxMarginRankingLoss (loss.py:315-367) in slab form. With
 * x[i,j] = cos(txt_i, img_j) (sim_matrix, loss.py:256-264: rows divided by max(norm, 1e-8)), d_i = x[i,i],
 * m_i = margin * weight_i (weight NULL: 1) and c_i = m_i - d_i the loss is
 *   (1/N) sum_i sum_j relu(c_i + x[i,j]) + relu(c_i + x[j,i]),
 * over j != i with N = 2G(G-1) (fix_norm, loss.py:297-307) or over all j with N = 2G^2.
 * img_all/txt_all: [G,E] dtype, the rank-ordered gathered RAW (un-normalised) rows; this rank owns rows
 * [row0, row0+B). E in {64,128,256,512}; another width is an error.
 * prepare (replaces loss.py:260-262,285 and the weight expansion :340-343) over all G rows:
 *   prep [7,G] f32 = {1/max(|img_j|,1e-8), 1/max(|txt_j|,1e-8), d_j, c_j, m_j, max(|img_j|,1e-8), max(|txt_j|,1e-8)}.
 * fwd (replaces loss.py:281-307 / :330-362: the G x G matrix, its four index-selected copies and the nonzero):
 *   direction 0 sweeps the own text rows against all image rows (terms relu(c_i + x[i,j])), direction 1 the own image
 *   rows against all text rows (terms relu(c_i + x[j,i])), the diagonal left out. hinge [2,B] f32: the row's hinge sum
 *   (+ relu(m_i) when with_diag != 0: the diagonal term of fix_norm=False); count [2,B] int32: its active terms.
 *   The loss is sum(hinge over all ranks) / N.
 * bwd (replaces autograd through loss.py:256-312 and GatherLayer.backward's all-reduce): recomputes the scores and
 *   writes coef * upstream * d(sum of all hinge terms)/d(RAW img_local | txt_local): [B,E] f32, normalisation
 *   backward included; upstream (nullable): DEVICE pointer to d(objective)/d(loss); coef: host factor mult/N.
 * Results are bit-reproducible and do not depend on how the G rows are split into slabs. */
int lvl_margin_loss_prepare(const void* img_all, const void* txt_all, const float* weight, float margin, int G,
                            int E, float* prep, int dtype, void* stream);
int lvl_margin_loss_fwd(const void* img_all, const void* txt_all, const float* prep, int B, int G, int E,
                        int row0, int with_diag, float* hinge, int32_t* count, int dtype, void* stream);
int lvl_margin_loss_bwd(const void* img_all, const void* txt_all, const float* prep, const float* upstream,
                        float coef, int B, int G, int E, int row0, float* dimg, float* dtxt, int dtype,
                        void* stream);

/* ---- vocabulary cross-entropy of the narrator's criterion (CaptionLoss, loss.py:220-253) -----------------------
 * Row form of F.cross_entropy(logits [B,V,T], labels [B,T], ignore_index=pad_id, reduction='none') and the metric
 * loop of loss.py:234-252. The logits are rows = B*T rows of `vocab` elements of dtype: row r starts at
 * logits + r*row_stride ELEMENTS (row_stride >= vocab), class stride 1. Nothing is assumed about the alignment of a
 * row beyond the element size; columns [vocab, row_stride) are never read. labels: int64, row r at
 * labels[r*label_stride]. All arithmetic is float32.
 * fwd, one pass over each row, per row:
 *   lse     [rows] f32    log sum_j exp(x[r,j]); -inf entries are allowed anywhere in a row;
 *   nll     [rows] f32    lse - x[r,label], exactly 0 when label == pad_id; the pad id is compared first and may lie
 *                         outside [0,vocab); any other label outside [0,vocab) forms no address and gives NaN;
 *   pred    [rows] int32  the FIRST index of the row's maximum (torch.argmax's tie rule, loss.py:239);
 *   correct [rows] int32  (pred == label) & (label != pad_id);   counted [rows] int32  (label != pad_id).
 * reduce, one workgroup, fixed summation order (no atomics; bit-reproducible), out3 [3] f32:
 *   out3[0] = sum(nll) / (B*T)                                (reduction='none' then .mean(): pads count below)
 *   out3[1] = 100 * sum(correct) / (sum(counted) + 1e-8)      (caption_acc, loss.py:252)
 *   out3[2] = mean_b exp(sum_t nll[b,t] / sum_t counted[b,t]) (ppl, loss.py:243,253; a caption without a counted
 *                                                              label gives 0/0 = NaN, as there)
 * bwd, one pass: dlogits [rows, Vp] dtype, Vp = vocab rounded up to 8, 16-byte aligned:
 *   dlogits[r,j] = coef * (*upstream) * (exp(x[r,j] - lse[r]) - [j == label_r])   for j < vocab, one rounding to dtype;
 *   rows whose label is pad_id are exact zeros, rows whose label is out of range are NaN, and the columns
 *   [vocab, Vp) of every row are written as zeros: every element of dlogits is written on every call.
 *   upstream (nullable): DEVICE pointer to d(objective)/d(loss); coef: host factor 1/(B*T). */
int lvl_token_xent_fwd(const void* logits, int64_t row_stride, const int64_t* labels, int64_t label_stride,
                       int64_t rows, int vocab, int64_t pad_id, float* lse, float* nll, int32_t* pred,
                       int32_t* correct, int32_t* counted, int dtype, void* stream);
int lvl_token_xent_reduce(const float* nll, const int32_t* correct, const int32_t* counted, int B, int T,
                          float* out3, void* stream);
int lvl_token_xent_bwd(const void* logits, int64_t row_stride, const int64_t* labels, int64_t label_stride,
                       const float* lse, const float* upstream, float coef, int64_t rows, int vocab, int64_t pad_id,
                       void* dlogits, int dtype, void* stream);

/* ---- cls-only attention (last block of a cls-pooled forward) ---------------------------------------------------
 * When only `norm(x)[:, 0]` leaves the tower (SpaceTimeTransformer.forward, timesformer.py:377,384-390) the last
 * block's space attention is needed for its cls query alone, which attends to all T tokens (timesformer.py:116-119):
 *   out[b,h,:] = softmax_j(0.125 * q[b,h,:] . k[b,j,h,:]) v[b,j,h,:]
 * q: [B, H*64] (the q third of the qkv Linear applied to the cls rows), kv: [B, T, 2*H*64] (its k and v thirds applied
 * to all rows), out: [B, H*64], lse: [B, H] f32 (natural log of the softmax denominator of the scaled scores).
 * Backward: dq [B, H*64] f32, dkv [B, T, 2*H*64] dtype, from dout [B, H*64]. */
int lvl_cls_attn_fwd(const void* q, const void* kv, void* out, float* lse, int B, int T, int H, int dtype, void* stream);
int lvl_cls_attn_bwd(const void* q, const void* kv, const void* out, const void* dout, const float* lse, float* dq,
                     void* dkv, int B, int T, int H, int dtype, void* stream);

/* ---- narrator seam: multi-query cross-attention pooling ----------------------------------------------------------
 * The core of coca.py's CrossAttention (lavila/models/coca.py:93-123) between to_q / to_kv and to_out, as
 * VCLM_HF.encode_image runs it on the tower's token features (narrator.py:44-49,88-90): NQ x H query rows of 64
 * channels attend to the Tk context tokens through ONE shared key/value head:
 *   out[b,n,h,:] = softmax_j(0.125 * q[b,n,h,:] . k[b,j,:]) v[b,j,:]   (q * dim_head^-0.5, max-subtracted softmax)
 * q: [B or 1, NQ, H*64] with batch stride q_batch_stride elements (0 = the same queries for every clip: the narrator
 * repeats its learned img_queries); kv: [B, Tk, 128] = k | v as to_kv writes them; out: [B, NQ, H*64].
 * Backward, from q, kv and dout [B, NQ, H*64] alone (the softmax is recomputed): dq [B, NQ, H*64], or [NQ, H*64] when
 * q_batch_stride is 0 -- the per-clip gradients of shared queries are then added in clip order -- and dkv [B, Tk, 128].
 * f32 accumulation, no atomics, bit-reproducible. ws: lvl_mq_cross_attn_bwd_ws(B, NQ, H, q_batch_stride == 0) floats
 * (host-side query; -1 for a shape with a non-positive extent). */
int lvl_mq_cross_attn_fwd(const void* q, int64_t q_batch_stride, const void* kv, void* out, int B, int NQ, int H,
                          int Tk, int dtype, void* stream);
int64_t lvl_mq_cross_attn_bwd_ws(int B, int NQ, int H, int shared_q);
int lvl_mq_cross_attn_bwd(const void* q, int64_t q_batch_stride, const void* kv, const void* dout, void* dq, void* dkv,
                          float* ws, int B, int NQ, int H, int Tk, int dtype, void* stream);

/* ---- narrator decoder: gated-cross-attention GPT-2 ---------------------------------------------------------------
 * The row passes of lavila/models/gpt2_gated.py's GPT2LMHeadModel around its Conv1D GEMMs (which run on lvl_linear_tn
 * against [out,in] bf16 copies of the [in,out] Conv1D weights). The reference's VCLM_HF.generate re-runs the whole prefix
 * for every token (narrator.py:118-143, use_cache=False); this ABI decodes ONE row per sequence and step against a
 * key/value cache whose fill level `pos_dev` is an int32 in DEVICE memory, so one captured hipGraph serves every step.
 * dtype = element type of activations, caches and embedding tables (LVL_F32 / LVL_BF16); arithmetic is f32.
 *
 * lvl_gpt2_embed (gpt2_gated.py:892-895): out[r,:] = wte[ids[r],:] + wpe[p0 + r % L,:], p0 = *pos_dev (0 when NULL);
 *   ids [rows] int64 (clamped into the table), wte [vocab, D], wpe [positions, D], D % 8 == 0.
 * lvl_gated_add_layernorm: s = res + (*gate) * y (gate NULL = 1, y NULL = no add), h = LayerNorm(s) * gamma + beta with
 *   biased variance over the D channels -- the residual adds of GPT2Block.forward (gpt2_gated.py:442-458 with the
 *   tanh(alpha) gates, :475, :483-487) fused with the LayerNorm that reads the sum next (ln_2_crossattention, ln_1, ln_2,
 *   the next block's first norm, ln_f). res / y / s / h: [rows, D]; s may be res (in place) or NULL; gate: one f32
 *   (tanh(alpha), computed by the caller); gamma / beta [D] f32; D % 8 == 0, D <= 4096.
 * lvl_act_inplace (gpt2_gated.py:363-396): u <- gelu_new(u) = 0.5 u (1 + tanh(sqrt(2/pi) (u + 0.044715 u^3))) or
 *   relu(u)^2 (mlp_crossattention), n % 8 == 0.
 * lvl_decode_self_attn (gpt2_gated.py:206-238,337-345 for one new token): qkv [B, 3*H*64] = q | k | v of the new token;
 *   cache [B, Tcap, 2*H*64] = k | v rows of the tokens so far. p = *pos_dev: row p of the cache is WRITTEN with this
 *   step's k | v, then out[b,h,:] = softmax_{j<=p}(0.125 q . k_j) v_j (the causal mask of a last-row query = all rows
 *   so far). The caller advances *pos_dev after the last layer.
 * lvl_cross_attn_rows_fwd (gpt2_gated.py:327-334 + _attn without a mask): multi-head attention of `rows` independent
 *   query rows q [rows, H*64] over per-context keys / values kv [rows/qrep, Tk, 2*H*64] = k | v (the cross-attention
 *   c_attn applied to the image tokens once per clip); qrep consecutive query rows share one context (the L positions
 *   of a teacher-forced caption, or the num_return_sequences samples of a clip). out [rows, H*64]. */
/* lvl_linear_skinny: y[M,N] = act(x[M,K] . w[N,K]^T + bias) for FEW rows -- the decoder's Conv1Ds while decoding
 * (M = captions in flight; gpt2_gated.py:327-334,337,354,392-394) and its lm_head. bf16 x / w / y, f32 bias (nullable)
 * and accumulation; act: -1 none, LVL_ACT_GELU_NEW, LVL_ACT_SQRELU (applied to the f32 sum before the bf16 store).
 * Up to 128 rows: one workgroup per 16 rows x 16 (N < 2048) or 32 x 64 columns, its 8 waves splitting K, fragments
 * straight from memory (lvl_linear_tn gives a 256-column panel to one compute unit, which at M <= 64 leaves the chip idle).
 * Beyond 128 rows, and for N >= 8192 (lm_head), K % 64 == 0: LDS-staged 64 x 64 / 64 x 128 tiles (whole-line loads, three K
 * blocks in flight). N % 16 == 0 and K % 32 == 0, else LVL_ENOSYS; any M >= 0. */
int lvl_linear_skinny(const void* x, const void* w, const float* bias, void* y, int M, int N, int K, int act, void* stream);
/* lvl_linear_skinny_f32c (round 5): the same product for FLOAT32 operands in f32-class mode -- x3 [M, K3] and w3 [N, K3]
 * are the bf16 term images of the float32 x [M, K] / w [N, K] (K3 = 3 K; lvl_split_bf16x3 role 0 for x, role 1 for w:
 * h|h|l against h|l|h, so one pass over K3 accumulates h.h' + h.l' + l.h'), y [M, N] float32, bias float32, activation on
 * the unrounded sum. Replaces the float32 `x @ W + b` of the reference's Conv1D / nn.Linear (gpt2_gated.py:184-188,
 * 383-384,1010; coca.py:78-88) where the widths are not multiples of 256 (lvl_linear_tn's f32-class mode takes those):
 * the narrator's float32 decoder, its lm_head and the float32 inference Linears of small towers. ~2^-17 relative per
 * product. N % 16 == 0 and K % 32 == 0, else LVL_ENOSYS. */
int lvl_linear_skinny_f32c(const void* x3, const void* w3, const float* bias, float* y, int M, int N, int K3, int act,
                           void* stream);
/* lvl_linear_skinny_ln: out[M,N] = act(LayerNorm(res + (*gate) * y) . w^T + bias), res_out = bf16(res + (*gate) * y) --
 * lvl_gated_add_layernorm folded into the prologue of the Conv1D that consumes it (q_attn / c_attn / the two c_fc of a
 * GPT2Block, gpt2_gated.py:441-487): a workgroup of lvl_linear_skinny owns whole rows of its input, so it forms the sum,
 * the row statistics and the normalised operand in registers before its first MFMA. y NULL = no add (res_out unused);
 * gate NULL = 1; res_out must NOT be res (other column strips are still reading it). gamma / beta [K] f32.
 * N % 16 == 0, K % 32 == 0, K <= 1792, else LVL_ENOSYS; meant for M <= 128 (decoding). */
int lvl_linear_skinny_ln(const void* res, const void* y, const float* gate, const float* gamma, const float* beta,
                         float eps, void* res_out, const void* w, const float* bias, void* out, int M, int N, int K,
                         int act, void* stream);
int lvl_gpt2_embed(const int64_t* ids, const void* wte, const void* wpe, const int* pos_dev, void* out, int rows, int L,
                   int D, int vocab, int positions, int dtype, void* stream);
int lvl_gated_add_layernorm(const void* res, const void* y, const float* gate, const float* gamma, const float* beta,
                            float eps, void* sum_out, void* h_out, int rows, int D, int dtype, void* stream);
int lvl_act_inplace(void* u, int64_t n, int act, int dtype, void* stream);
int lvl_decode_self_attn(const void* qkv, void* cache, const int* pos_dev, void* out, int B, int Tcap, int H, int dtype,
                         void* stream);
int lvl_cross_attn_rows_fwd(const void* q, const void* kv, void* out, int rows, int qrep, int Tk, int H, int dtype,
                            void* stream);
/* Training forms of the row passes above (bf16 training of the decoder; the inference entry points keep their signatures).
 * lvl_gated_add_layernorm_train: lvl_gated_add_layernorm (the same kernel: s and h equal its results to the bit) that also
 *   returns the row statistics mean, rstd [rows] f32 of the stored sum.
 * lvl_gated_add_layernorm_bwd: from dh [rows, D], the kept sum s, the statistics and an optional dadd [rows, D] (the
 *   gradient that reaches the sum from the residual stream): ds [rows, D] = d res (lvl_layernorm_bwd on s, dadd added),
 *   dgamma, dbeta [D] f32 and -- when y and gate are given -- dy [rows, D] = (*gate) * ds and ONE f32
 *   *dgate = sum ds * y (per-workgroup partials added in slot order: no atomics, bit-reproducible); the caller turns it into
 *   d alpha = dgate * (1 - tanh^2 alpha). Without a gate the gradient of y is ds itself and dy / dgate are not written.
 *   ws: lvl_workspace_floats("gated_add_layernorm_bwd", rows, D). rows > 0.
 * lvl_act_fwd: a = act(u), out of place (u is kept for the backward); lvl_act_bwd: du = da * act'(u) with the forward's
 *   tanh expression for gelu_new and 2 relu(u) for relu^2 (exact zeros where u <= 0). n % 8 == 0. All three entry points
 *   also take LVL_ACT_GELU_ERF, the exact GELU of DistilBERT's FFN (transformers' activation "gelu"):
 *   a = 0.5 u (1 + erf(u / sqrt 2)), du = da (Phi(u) + u phi(u)). The skinny GEMMs' fused activations do not.
 * lvl_cross_attn_rows_bwd: from q, kv and dout [rows, H*64] (softmax recomputed): dq [rows, H*64] and
 *   dkv [rows/qrep, Tk, 2*H*64], the latter accumulated in f32 over the qrep rows of a context inside one workgroup and
 *   rounded once. Every element of dq and dkv is written. bf16 and 1 <= Tk <= 256 only, else LVL_ENOSYS; any qrep >= 1.
 *   No workspace, no atomics, bit-reproducible. */
int lvl_gated_add_layernorm_train(const void* res, const void* y, const float* gate, const float* gamma,
                                  const float* beta, float eps, void* sum_out, void* h_out, float* mean, float* rstd,
                                  int rows, int D, int dtype, void* stream);
int lvl_gated_add_layernorm_bwd(const void* dh, const void* s, const void* y, const float* gate, const float* gamma,
                                const float* mean, const float* rstd, const void* dadd, void* ds, void* dy, float* dgamma,
                                float* dbeta, float* dgate, float* ws, int rows, int D, int dtype, void* stream);
int lvl_act_fwd(const void* u, void* a, int64_t n, int act, int dtype, void* stream);
int lvl_act_bwd(const void* u, const void* da, void* du, int64_t n, int act, int dtype, void* stream);
int lvl_cross_attn_rows_bwd(const void* q, const void* kv, const void* dout, void* dq, void* dkv, int rows, int qrep,
                            int Tk, int H, int dtype, void* stream);

/* Dropout of the narrator decoder in training (gpt2_gated.py:186-187, 230, 354, 389-395, 737, 899), generated INSIDE the
 * kernels that already touch the data: no mask tensor is stored, the backward regenerates the mask. ONE definition
 * (csrc/dropout.h): Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl increments 0x9E3779B9 / 0xBB67AE85); for a
 * 64-bit seed, a 32-bit site, a 64-bit element index e and p in [0, 1):
 *   g = e >> 2, ctr = (g & 0xffffffff, g >> 32, site, 0), key = (seed & 0xffffffff, seed >> 32),
 *   w = philox4x32_10(ctr, key)[e & 3], T = min(2^32 - 1, floor(p * 2^32 + 0.5)), keep iff w >= T, scale = 1.0f / (1.0f - p).
 * p = 0 keeps everything with scale 1. Row sites over [rows, D]: e = row * D + col. Attention sites:
 * e = (((ctx * H + h) * qrep + i) << 8) | j for query i of its context and key j < 256. Sites follow the reference's
 * execution order: 0 = embedding; block i: 1 + 6 i + {0 cross-attention probabilities, 1 cross c_proj output,
 * 2 mlp_crossattention output, 3 self-attention probabilities, 4 self c_proj output, 5 mlp output}.
 *
 * lvl_dropout_mask: out[i] = keep(elem0 + i) as a byte, i < n -- the masks of the fused kernels (same device function),
 *   for tests and golden tools.
 * lvl_dropout_apply: out = keep ? scale * x : 0 over n elements (e = index; n % 8 == 0); out may be x. The embedding site,
 *   and its own backward when applied to the gradient.
 * lvl_gated_add_layernorm_train_drop: lvl_gated_add_layernorm_train with dropout on y: c = (*gate) * scale (gate NULL = 1),
 *   s = round(fma(keep ? c : 0, y, res)), h = LayerNorm(s); a dropped element leaves s == res to the bit; p = 0 gives the
 *   bits of lvl_gated_add_layernorm_train. y and sum_out are required.
 * lvl_gated_add_layernorm_bwd_drop: ds, dgamma, dbeta as lvl_gated_add_layernorm_bwd; dy = (keep ? c : 0) * ds is written
 *   for ungated sites too (gate NULL); with a gate, *dgate = sum ds * (keep ? scale * y : 0) over ordered partial slots
 *   (no atomics). ws: lvl_workspace_floats("gated_add_layernorm_bwd", rows, D).
 * lvl_attn_rows_drop_fwd / _bwd: the rows attention of lvl_cross_attn_rows_fwd / _bwd (one workgroup per (context, head),
 *   single-pass softmax over <= 256 keys) with dropout on the probabilities and an optional causal mask. q: contexts * qrep
 *   rows q_stride elements apart; k, v: per context Tk rows kv_stride apart, contexts kv_ctx_stride apart -- the image
 *   keys | values [ctx, Tk, 2D] (v = k + D, strides 2D and Tk * 2D) or the k and v thirds of qkv [B L, 3D] (q_stride =
 *   kv_stride = 3D, kv_ctx_stride = L * 3D, qrep = Tk = L, causal = 1: key j <= query i). out, dout: [rows, H*64]
 *   contiguous; dq is laid out as q, dk / dv as k / v. P = softmax(S) over all unmasked keys, Pd = keep ? scale * P : 0
 *   (rounded to bf16 where P is), O = Pd V; backward: dP = keep ? scale * (dO V^T) : 0, delta = sum_j P dP,
 *   dS = P o (dP - delta), dV = Pd^T dO. Non-causal with p == 0 on the image layout IS lvl_cross_attn_rows_fwd / _bwd (same
 *   kernels, same bits). bf16 and 1 <= Tk <= 256 only, else LVL_ENOSYS. No workspace, no atomics, bit-reproducible. */
int lvl_dropout_mask(uint8_t* out, int64_t n, uint64_t elem0, uint64_t seed, uint32_t site, float p, void* stream);
int lvl_dropout_apply(const void* x, void* out, int64_t n, uint64_t seed, uint32_t site, float p, int dtype, void* stream);
int lvl_gated_add_layernorm_train_drop(const void* res, const void* y, const float* gate, const float* gamma,
                                       const float* beta, float eps, void* sum_out, void* h_out, float* mean, float* rstd,
                                       int rows, int D, uint64_t seed, uint32_t site, float p, int dtype, void* stream);
int lvl_gated_add_layernorm_bwd_drop(const void* dh, const void* s, const void* y, const float* gate, const float* gamma,
                                     const float* mean, const float* rstd, const void* dadd, void* ds, void* dy,
                                     float* dgamma, float* dbeta, float* dgate, float* ws, int rows, int D, uint64_t seed,
                                     uint32_t site, float p, int dtype, void* stream);
int lvl_attn_rows_drop_fwd(const void* q, const void* k, const void* v, void* out, int contexts, int qrep, int Tk, int H,
                           int64_t q_stride, int64_t kv_stride, int64_t kv_ctx_stride, int causal, uint64_t seed,
                           uint32_t site, float p, int dtype, void* stream);
int lvl_attn_rows_drop_bwd(const void* q, const void* k, const void* v, const void* dout, void* dq, void* dk, void* dv,
                           int contexts, int qrep, int Tk, int H, int64_t q_stride, int64_t kv_stride,
                           int64_t kv_ctx_stride, int causal, uint64_t seed, uint32_t site, float p, int dtype,
                           void* stream);

/* Key-masked bidirectional attention: the self-attention of a padded text batch (DistilBERT's MultiHeadSelfAttention
 * under an attention_mask), head dim 64, scale 1/8. Operands as lvl_attn_rows_drop_fwd / _bwd: q: contexts * qrep rows
 * q_stride elements apart; k, v: per context Tk rows kv_stride apart, contexts kv_ctx_stride apart (three tensors, or the
 * thirds of a packed qkv); out, dout: [rows, H*64] contiguous; dq is laid out as q, dk / dv as k / v. qrep = 1 with
 * q_stride = L * D is the row-0 form (only the first position of every sample asks).
 * keymask: [contexts, Tk] bytes, contexts mask_ctx_stride bytes apart, non-zero = visible; NULL = all visible (the bits
 *   of an all-ones mask).
 * P = softmax over the visible keys of the context, the row maximum taken over visible keys only; a hidden key has
 *   probability exactly 0 and dS exactly 0: its k / v rows do not reach any result and its dk / dv rows are exact zeros.
 *   A context with NO visible key gets the uniform distribution over its Tk keys (what transformers' finite fill gives):
 *   out = mean_j v_j, dv_j = sum_i dout_i / Tk, dq = dk = 0; always finite.
 * bf16 with 1 <= Tk <= 256: the MFMA rows attention of lvl_attn_rows_drop_fwd / _bwd with a key-mask flag (one workgroup per
 *   (context, head), exact single-pass softmax, P rounded to bf16 for P V; hidden rows of k / v are staged but enter every
 *   product with a factor of exactly 0, so they must be finite). float32, and bf16 with Tk > 256 (DistilBERT allows 512
 *   positions): shape-generic kernels in f32 arithmetic, one wave per (query row, head) with an online softmax over 64-key
 *   chunks, hidden rows never read; their backward recomputes the softmax and keeps (lse, delta) per (row, head) in ws.
 *   ws: lvl_workspace_floats("keymask_attn_bwd", contexts * qrep * H, Tk) floats, required by every call of _bwd. Every
 *   addressed element of out / dq / dk / dv is written on every call. No atomics, bit-reproducible. Tk <= 0, strides that are
 *   not multiples of 8, pointers off 16 bytes and unknown dtypes return LVL_EINVAL without a launch. */
int lvl_keymask_attn_fwd(const void* q, const void* k, const void* v, const uint8_t* keymask, void* out, int contexts,
                         int qrep, int Tk, int H, int64_t q_stride, int64_t kv_stride, int64_t kv_ctx_stride,
                         int64_t mask_ctx_stride, int dtype, void* stream);
int lvl_keymask_attn_bwd(const void* q, const void* k, const void* v, const uint8_t* keymask, const void* dout, void* dq,
                         void* dk, void* dv, float* ws, int contexts, int qrep, int Tk, int H, int64_t q_stride,
                         int64_t kv_stride, int64_t kv_ctx_stride, int64_t mask_ctx_stride, int dtype, void* stream);

/* ---- dropout of the DistilBERT text tower (opt-in, distilbert.TEXT_DROPOUT) -------------------------------------------
 * transformers' modeling_distilbert.py calls dropout 1 + 2 n_layers times per forward: on the embedding behind
 * embeddings.LayerNorm [B, L, D]; per layer on the attention probabilities behind the masked softmax [B, H, L, L]
 * (attention_dropout) and on the output of ffn.lin2 with its bias, before + sa_output and output_layer_norm [B, L, D]
 * (dropout). Nothing is dropped behind out_lin.
 * THE MASK CONTRACT. The generator is the decoder's (csrc/dropout.h, above): same Philox, threshold and float32 scale.
 *   Sites: 0 = the embedding; layer n: 1 + 2 n = attention probabilities, 2 + 2 n = FFN output.
 *   Row sites over [B, L, D]: e = (b * L + i) * D + c, L = the positions the tower runs on (after the trim).
 *   Attention sites: e = ((((b * H + h) * L + i) << s) | j for query position i and key j; s = 8 for Tk <= 256 (the decoder's
 *   mapping), else the smallest s with 2^s >= Tk (9 for DistilBERT's 512 positions).
 *   A call that computes a SUBSET of the rows addresses the elements of the full call: the row entry points take
 *   row_index_stride (row r of the call has e = r * row_index_stride + c: D for all rows, L * D for row 0 of every sample),
 *   the attention entry points take idx_qrep (query i of context b is row b * idx_qrep + i of the index: L when qrep == 1).
 *   P is the softmax over the visible keys exactly as in lvl_keymask_attn_fwd, the row sum runs over ALL visible keys;
 *   Pd = keep ? scale * P : 0 (rounded to bf16 where P is), O = Pd V. A hidden key keeps P = dS = 0 and exact-zero dk / dv
 *   rows; a context with no visible key gets the uniform distribution and THEN dropout. Backward: dP = keep ? scale *
 *   (dO V^T) : 0, delta = sum_j P dP (= dO . O), dS = P o (dP - delta), dV = Pd^T dO.
 * lvl_keymask_attn_drop_fwd / _bwd: the operands of lvl_keymask_attn_fwd / _bwd plus idx_qrep (>= qrep), seed, site, p in
 *   [0, 1). p == 0 runs lvl_keymask_attn_fwd / _bwd (same kernels, same bits). bf16 with Tk <= 256: the <DROP, KEYMASK>
 *   instantiations of the MFMA rows attention; float32, and bf16 with Tk > 256: the shape-generic kernels, whose (m, l) and
 *   (lse, delta) are those of the undropped softmax and whose backward passes regenerate keep from the index. One Philox
 *   call serves four consecutive keys. Same workspace as lvl_keymask_attn_bwd, every addressed element written on every
 *   call, no atomics, bit-reproducible.
 * lvl_dropout_add_layernorm_fwd / _bwd: the FFN site. s = round(fma(keep ? scale : 0, y, res)), h = LayerNorm(s); returns
 *   the kept sum, mean and rstd (lvl_gated_add_layernorm_train_drop with gate NULL and a row index stride: with
 *   row_index_stride == D its bits; p = 0: the bits of lvl_gated_add_layernorm_train). _bwd writes ds and dy = (keep ?
 *   scale : 0) * ds, dgamma, dbeta; dadd nullable; ws: lvl_workspace_floats("gated_add_layernorm_bwd", rows, D). bf16 and
 *   float32; D % 8 == 0, D <= 4096, row_index_stride % 8 == 0 and >= D.
 * The embedding site is lvl_dropout_apply over the [B L, D] rows (it always runs on all rows). */
int lvl_keymask_attn_drop_fwd(const void* q, const void* k, const void* v, const uint8_t* keymask, void* out, int contexts,
                              int qrep, int Tk, int H, int64_t q_stride, int64_t kv_stride, int64_t kv_ctx_stride,
                              int64_t mask_ctx_stride, int idx_qrep, uint64_t seed, uint32_t site, float p, int dtype,
                              void* stream);
int lvl_keymask_attn_drop_bwd(const void* q, const void* k, const void* v, const uint8_t* keymask, const void* dout,
                              void* dq, void* dk, void* dv, float* ws, int contexts, int qrep, int Tk, int H,
                              int64_t q_stride, int64_t kv_stride, int64_t kv_ctx_stride, int64_t mask_ctx_stride,
                              int idx_qrep, uint64_t seed, uint32_t site, float p, int dtype, void* stream);
int lvl_dropout_add_layernorm_fwd(const void* res, const void* y, const float* gamma, const float* beta, float eps,
                                  void* sum_out, void* h_out, float* mean, float* rstd, int rows, int D,
                                  int64_t row_index_stride, uint64_t seed, uint32_t site, float p, int dtype, void* stream);
int lvl_dropout_add_layernorm_bwd(const void* dh, const void* s, const float* gamma, const float* mean, const float* rstd,
                                  const void* dadd, void* ds, void* dy, float* dgamma, float* dbeta, float* ws, int rows,
                                  int D, int64_t row_index_stride, uint64_t seed, uint32_t site, float p, int dtype,
                                  void* stream);

/* ---- packed caption rows: the narrator's teacher-forced pass on the rows that carry a label -------------------------
 * A batch of B captions of up to L positions keeps len_b = cu[b + 1] - cu[b] leading rows each; cu [B + 1] int32 (device),
 * cu[0] = 0, R = cu[B] packed rows.
 *   lvl_rows_pack:   dst[cu[b] + i, 0:D] = src[b, i, 0:D] for i < len_b. src element (b, i, c) at b * src_batch_stride +
 *                    i * src_row_stride + c; dst [R, D] contiguous.
 *   lvl_rows_unpack: dst[b, i, 0:D] = i < len_b ? src[cu[b] + i, 0:D] : 0 for EVERY b < B, i < L (every addressed element is
 *                    written on every call; nothing outside columns [0, D) of a row, nothing behind row B L - 1). src [R, D]
 *                    contiguous, dst strided like lvl_rows_pack's src; its batches must not overlap.
 * Each is the other's adjoint: the backward of one is the other on the gradient. dtype LVL_BF16 or LVL_F32; rows move as
 * 16-byte words, bit for bit: D % 8 == 0, strides multiples of 8 elements, src / dst 16-byte aligned, B L <= 2^31 - 1.
 * The host validates the lengths (it holds them); for memory safety the kernel clamps len_b into [0, L] and cu[b] into
 * [0, b L], so no access leaves the first B L packed rows or the rectangle whatever `cu` holds. Plain vector loads and
 * stores, no atomics, no workspace; the grid is capped at 4096 workgroups of 256 threads that stride over the rows. */
int lvl_rows_pack(const void* src, int64_t src_batch_stride, int64_t src_row_stride, const int32_t* cu, int B, int L, int D,
                  void* dst, int dtype, void* stream);
int lvl_rows_unpack(const void* src, const int32_t* cu, int B, int L, int D, void* dst, int64_t dst_batch_stride,
                    int64_t dst_row_stride, int dtype, void* stream);

/* lvl_sample_next_token: everything VCLM_HF.generate does with one step's logits (narrator.py:122-137 and the warpers
 * of :368-389 = transformers' Temperature / TopK / TopP logits warpers with min_tokens_to_keep = 1), one workgroup per
 * caption, the row resident in LDS as 16-bit keys -- no sort, no [rows, vocab] temporaries:
 *   nll[r]     = target ? (target[r] == pad_id ? 0 : logsumexp(l_r) - l_r[target[r]])      F.cross_entropy(ignore_index=pad)
 *                       : entropy of softmax(l_r)                                          torch.special.entr(softmax).sum()
 *   counted[r] = target ? (target[r] != pad_id) : 1
 *   next_token[r] ~ softmax(warp(l_r)): l / temperature; keep the top_k largest (0 = off; ties with the k-th stay);
 *                drop the ascending-probability tail whose cumulative mass is <= 1 - top_p (1 = off), always keeping
 *                the largest; inverse CDF over the kept entries in index order at uniform[r] (in [0,1), e.g. torch.rand).
 *                top_k = 1 is greedy: the first maximum, whatever the uniform.
 * logits: [rows, >= vocab] bf16, row stride row_stride elements (a multiple of 8, rows 16-byte aligned, >= vocab rounded
 * up to 8: the padded product the lm_head GEMM leaves). vocab <= lvl_sample_max_vocab() (the row must fit 160 KB of
 * LDS; GPT-2's 50257 does), else LVL_ENOSYS. target / dbg nullable; dbg [rows,12] f32 = (lowest kept value, ties dropped
 * at the top-p boundary, kept mass relative to e^max, top-p boundary value; microseconds spent in the kernel's 5 phases,
 * start time) for tests and tools/probe_narrator.py. */
int lvl_sample_max_vocab(void);
int lvl_sample_next_token(const void* logits, int64_t row_stride, int rows, int vocab, float temperature, int top_k,
                          float top_p, const float* uniform, const int64_t* target, int64_t pad_id, int64_t* next_token,
                          float* nll, float* counted, float* dbg, void* stream);

/* ---- Linear layers: forward and input-gradient GEMMs with fused epilogues -------------------------------------
 * y[M,N] = epilogue(x[M,K] . w[N,K]^T): both operands bf16, row-major, contraction-contiguous; f32 accumulation.
 * Forward of every nn.Linear on the path (qkv/proj timesformer.py:95-96,110,142; Mlp fc1/fc2 timesformer.py:47-58;
 * the Conv2d(k=s=P) contraction timesformer.py:77,83; text in_proj/out_proj/c_fc/c_proj openai_model.py:186-192)
 * with w = the bf16 weight [out,in]; input gradient dx = dy . wt^T with wt = the transposed bf16 copy [in,out]
 * that lvl_cast_transpose writes (what autograd computes for the Linear input when loss.backward() runs,
 * main_pretrain.py:520). bias: [N] f32, nullable. Epilogues:
 *   LVL_EPI_BIAS             y = acc + bias
 *   LVL_EPI_BIAS_QUICKGELU   aux_out = u = bf16(acc + bias); y = u * sigmoid(1.702 u)     (fc1 + QuickGELU,
 *                            timesformer.py:52-54, openai_model.py:177-179; u is kept for the backward)
 *   LVL_EPI_QUICKGELU_BWD    y = acc * d quickgelu(aux_in); colsum[N] f32 = column sums of y (= d fc1.bias);
 *                            acc = dA = dY . W2 is the input gradient of fc2, y = d(fc1 output)
 *   LVL_EPI_BIAS_RESIDUAL    y = acc + bias + aux_in: the Linear's output added to the residual stream, in f32 before the
 *                            one rounding of the sum -- `x + attn(norm1(x))`, `x + mlp(norm2(x))` (timesformer.py:183-196;
 *                            openai_model.py:199-200) leave proj / fc2 as the new stream; aux_in [M,N], y's dtype
 *   LVL_EPI_BIAS_QUICKGELU_DERIV   (bf16 only) u = acc + bias (f32, not rounded); y = u * sigmoid(1.702 u);
 *                            aux_out = d quickgelu(u) = s (1 + 1.702 u (1 - s)), s = sigmoid(1.702 u): the training form of
 *                            LVL_EPI_BIAS_QUICKGELU -- autograd's backward of timesformer.py:52-54 needs the derivative,
 *                            not u, and the forward holds s in a register (one exp2 + one reciprocal serve both outputs)
 *   LVL_EPI_MUL_AUX_COLSUM   (bf16 only) y = acc * aux_in; colsum[N] f32 = column sums of y: LVL_EPI_QUICKGELU_BWD on the
 *                            stored derivative (no transcendental in the backward's epilogue)
 *   LVL_EPI_BIAS_GELU        LVL_EPI_BIAS_QUICKGELU with the exact GELU y = 0.5 u (1 + erf(u / sqrt 2)) (nn.GELU(), the default
 *                            act_layer of the reference's SpaceTimeTransformer): aux_out = u = bf16(acc + bias), y = gelu(u) on
 *                            the ROUNDED u with the arithmetic of lvl_act_fwd(LVL_ACT_GELU_ERF), which rebuilds y from the kept
 *                            u to the bit
 *   LVL_EPI_GELU_BWD         LVL_EPI_QUICKGELU_BWD for the same: y = acc * gelu'(aux_in), gelu'(u) = Phi(u) + u phi(u) (the
 *                            arithmetic of lvl_act_bwd); colsum as there
 *   LVL_EPI_BIAS_GELU_DERIV  (bf16 only) LVL_EPI_BIAS_QUICKGELU_DERIV for the same: u = acc + bias (f32, not rounded);
 *                            y = gelu(u); aux_out = gelu'(u), in [-0.129, 1.129]; one erf serves both outputs. The backward
 *                            is LVL_EPI_MUL_AUX_COLSUM on the stored derivative
 * aux_out / aux_in: [M,N] bf16. N % 256 == 0 and K % 64 == 0, else LVL_ENOSYS. Workspace (QUICKGELU_BWD /
 * MUL_AUX_COLSUM / GELU_BWD only): lvl_workspace_floats("linear_tn", M, N) floats.
 * Sizes: the two INPUT operands must stay below 4 GiB each -- M*K*2 < 2^32 and N*K*2 < 2^32 bytes (K as passed, i.e. 3*K0 in
 * the f32-class mode), else LVL_ENOSYS before anything is launched: the kernel fetches x and w with 32-bit byte offsets. The
 * largest M is therefore floor((2^32 - 1) / (2 K)). y, aux_out and aux_in have NO such limit (64-bit row offsets; M*N*2, or
 * M*N*4 in the f32-class mode, may exceed 4 GiB and M*N may exceed 2^31 elements); ceil(M / 256) * (N / 256) must stay below
 * 2^31 tiles (LVL_EINVAL).
 * dtype = LVL_F32 selects the F32-CLASS MODE of the same kernel (the parity configuration, north_star "within 1e-3
 * fp32"): x [M, 3K0] and w [N, 3K0] are the bf16 term images lvl_split_bf16x3 writes (role 0 for x, role 1 for w;
 * K = 3*K0, K0 % 64 == 0), so that one pass accumulates xh.wh + xh.wl + xl.wh in f32 (~2^-17 relative per product);
 * y, aux_out and aux_in are FLOAT32 [M,N] and the QuickGELU / GELU epilogues see the unrounded pre-activation
 * (the two *_DERIV epilogues and MUL_AUX_COLSUM are bf16 only: LVL_ENOSYS). Same tiling,
 * LDS-DMA ring, MFMA schedule, bias path and tile schedule as the bf16 mode.
 * sched (nullable): the launch's TILE-COUNTER block, 16 x uint32 (64-byte aligned), ZERO on entry; the kernel leaves it
 * zero again when its last workgroup exits, so a caller may hand the same block to the next launch on the SAME stream
 * (launches that can run concurrently -- other streams, graph branches -- need distinct blocks). With it the persistent
 * workgroups take their 256x256 tiles from per-XCD device counters instead of static ranges: a compute unit held by
 * another kernel (an RCCL channel during DDP's gradient all-reduce, main_pretrain.py:180-183) then costs one tile, not
 * a range. NULL = static ranges (identical results: the schedule does not change any tile's arithmetic). */
int lvl_linear_tn(const void* x, const void* w, const float* bias, void* y, void* aux_out, const void* aux_in,
                  float* colsum, float* ws, uint32_t* sched, int64_t M, int N, int K, int epilogue, int dtype,
                  void* stream);

/* ---- Plain Linear GEMM on ragged widths ------------------------------------------------------------------------
 * y[M,N] = x[M,K] . w[N,K]^T (+ bias) for N % 64 == 0, K % 64 == 0, M >= 1: the Conv1D GEMMs (forward and input gradient)
 * of a GPT-2 decoder whose widths are multiples of 64 but not of 256 (gpt2_gated.py's GPT-2 XL: 1600, 3200, 4800). bf16
 * operands and result, f32 accumulation, bias [N] f32 nullable, y row stride N. Two launches on `stream`: lvl_linear_tn's
 * persistent kernel over the N / 256 full column tiles (the launch it issues for w[:256 * (N / 256)], with N as the output
 * stride; `sched` as there) and an edge kernel for the 64 / 128 / 192 columns behind them (alone when N < 256). No atomics,
 * fixed summation order: repeats are bit-identical. epilogue must be LVL_EPI_BIAS and dtype LVL_BF16 (others: LVL_ENOSYS;
 * unknown values LVL_EINVAL); x and w below 4 GiB each (LVL_ENOSYS otherwise), no limit on y, and 16-byte aligned pointers as
 * for lvl_linear_tn. */
int lvl_linear_tn_ragged(const void* x, const void* w, const float* bias, void* y, uint32_t* sched, int64_t M, int N,
                         int K, int epilogue, int dtype, void* stream);

/* ---- Linear-layer weight gradient ------------------------------------------------------------------------
 * dW[N,K] = dY[M,N]^T X[M,K], dbias[N] (nullable) = column sums of dY: what torch.autograd computes for the weight
 * and bias of every nn.Linear on the path (qkv/proj: timesformer.py:96-99, Mlp fc1/fc2: timesformer.py:47-50) when
 * `loss.backward()` runs (main_pretrain.py:520). dy: [M,N], x: [M,K] bf16 row-major; dw: [N,K] f32; dbias: [N] f32.
 * Tiled for N, K multiples of 192/288/384 (TSF-B/L widths) or 128/256, and -- where none of those divides the shape --
 * of 160/320 (the GPT-2 XL decoder's 1600-family); other shapes return LVL_ENOSYS and the caller keeps the library GEMM. Workspace: lvl_workspace_floats("linear_wgrad", N, K) floats (-1 = unsupported shape).
 * sched (nullable): CHUNK-COUNTER block of the launch, 1024 x uint32 (64-byte aligned), ZERO on entry, zero again when
 * the launch has drained (same reuse rule as lvl_linear_tn's block). With it every (tile, row split) unit is cut into
 * row chunks handed out by device counters: a workgroup works through its own unit and then takes unclaimed chunks of
 * the other splits of its tile, so a compute unit held by another kernel delays the launch by a fraction of a unit
 * instead of a second round. With all CUs available nobody steals and the result is bit-identical to the static plan
 * (NULL). f32-class weight gradients use the same entry with row-STACKED term images (lvl_split_bf16x3 with
 * dst_term_stride = rows_padded * cols): dy3 [3M,N] = (h; h; l), x3 [3M,K] = (h; l; h); dw is float32 either way.
 * Sizes: no limit on dy or x (64-bit row pointers per lane; M / 32 < 2^31 row blocks): both may exceed 4 GiB. */
int lvl_linear_wgrad(const void* dy, const void* x, float* dw, float* dbias, float* ws, uint32_t* sched, int64_t M,
                     int N, int K, int dtype, void* stream);
/* What lvl_linear_wgrad would launch for (M, N, K) under the current lvl_set_compute_units limit (host-side query, no
 * device work; without a device the plan is the one of 256 compute units). out[9] = {cfg, tiles_k, ntiles, S, base, rem,
 * L, nch0, nch1}: tile configuration (index into the kernel's table of workgroup shapes), tiles along K, output tiles,
 * row splits (ntiles * S workgroups); the M / 32 full row blocks are dealt to the splits as `base` each, the first `rem`
 * splits one more; with `sched` a unit is claimed in chunks of L row blocks, nch0 / nch1 of them for a unit of base /
 * base + 1 blocks. M = 0: the plan the workspace is sized for (the largest S), row fields zero. LVL_ENOSYS where
 * lvl_linear_wgrad has no tiling. */
int lvl_linear_wgrad_plan(int64_t M, int N, int K, int* out);
/* The (split, tile) pair = split * ntiles + tile that workgroup `bid` of a launch of `pairs` = ntiles * S workgroups
 * computes under configuration `cfg` (the kernel's own block decode); negative for arguments out of range. */
int lvl_linear_wgrad_pair_of_block(int cfg, int pairs, int bid);

/* ---- bias gradient of the qkv Linear that feeds an attention core ------------------------------------------------
 * dbias[3D] = column sums over all rows of the dqkv an attention backward produced (what autograd computes for
 * `qkv.bias`, timesformer.py:96 / `in_proj_bias`, openai_model.py:196-198) without reading the k and v thirds:
 * every softmax row sums to 1, so sum_rows(dv) = sum_rows(dout); the scores are invariant to a constant added to
 * every key, so sum_rows(dk) = 0; only the q third of dqkv is reduced. dqkv: [rows, 3D], dout: [rows, D] dtype;
 * dbias: [3D] f32. Workspace: lvl_workspace_floats("qkv_bias_grad", rows, D). */
int lvl_qkv_bias_grad(const void* dqkv, const void* dout, float* dbias, float* ws, int64_t rows, int D, int dtype,
                      void* stream);
/* lvl_divided_attn_bwd_bias (round 5): lvl_divided_attn_bwd AND the qkv-bias gradient of the same Linear in one call,
 * without the pass over dqkv / dout where the kernels can avoid it (autograd of timesformer.py:96,110-140 wrt qkv.bias):
 *   q third -- the LDS-resident fused space kernel and the register-tiled time kernels hold the dQ accumulators / dq
 *              rows in registers: they write per-workgroup column sums (a [B F, D] / [B chunks, D] f32 slab) on the way
 *              and a two-stage column reduce finishes them; other kernel families reduce the q third of dqkv afterwards;
 *   k third -- exactly 0;
 *   v third -- `dout_colsum` [D] f32 when the caller has it (dout is the input gradient dy.W of the projection Linear:
 *              sum_rows(dout) = sum_rows(dy).W = d(b_proj).W, lvl_vec_mat_f32), else (NULL) reduced here from dout.
 * dbias [3D] f32; ws as for lvl_divided_attn_bwd; ws2: lvl_divided_attn_bwd_bias_ws(...) floats. */
int64_t lvl_divided_attn_bwd_bias_ws(int B, int F, int N, int H, int mode, int dtype);
int lvl_divided_attn_bwd_bias(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* ws,
                              const float* dout_colsum, float* dbias, float* ws2, int B, int F, int N, int H, int mode,
                              int dtype, void* stream);
/* Measurement / selection hook: bias-gradient rider of the register-tiled time backward kernels -- 0 none (the q third is
 * reduced from dqkv afterwards), 1 column sums in registers at the kernels' usual occupancy, 2 at one wave per SIMD less
 * (no spills), -1 (default) the measured choice per shape. Results are identical up to f32 summation order. */
int lvl_debug_time_bwd_rider(int mode);
/* lvl_vec_mat_f32: out[K] = v[N] . W[N, K] (float32, row-major W) -- column sums of a Linear's input gradient from the
 * column sums of its output gradient: dx = dy W  =>  sum_rows(dx) = sum_rows(dy) W (what feeds `dout_colsum` above). */
int lvl_vec_mat_f32(const float* v, const float* W, float* out, int N, int K, void* stream);

/* ---- weight staging of a Linear layer under bf16 autocast ----------------------------------------------------
 * dst[n,k] = bf16(src[n,k]), dst_t[k,n] = bf16(src[n,k]): the cast autocast applies to nn.Linear weights
 * (main_pretrain.py:491 `amp.autocast`) plus the transposed copy the input-gradient GEMM wants, in one pass.
 * src: [N,K] f32; dst: [N,K] bf16; dst_t: [K,N] bf16. */
int lvl_cast_transpose(const float* src, void* dst, void* dst_t, int N, int K, void* stream);
/* The same for MANY weights in one launch (every Linear weight of both towers is re-cast once per optimizer step:
 * main_pretrain.py:520-533 `optimizer.step()` then the next `model(...)`): desc = DEVICE array of `count` records of 40 bytes
 * { const float* src; void* dst; void* dst_t; uint32_t N; uint32_t K; int64_t tile0; }, tile0 = number of 64 x 64 tiles of
 * the records in front (tile0 of record 0 = 0, ascending), total_tiles = their sum over all records. */
int lvl_cast_transpose_multi(const void* desc, int count, int64_t total_tiles, void* stream);

/* ---- f32-class operands for the MFMA GEMMs (parity configuration) ----------------------------------------------
 * Writes a float32 matrix src [rows, cols] (row stride src_row_stride elements) as three bf16 TERM images:
 * h = bf16(x), l = bf16(x - h) (x = h + l up to 2^-18 |x|); image t of element (r, c) goes to
 * dst[r * dst_row_stride + t * dst_term_stride + c], t = 0..2, with the terms (h, h, l) for role 0 (the x / dy side of a
 * product) and (h, l, h) for role 1 (the w / x side): contracting image against image gives h.h' + h.l' + l.h'.
 * Replaces nothing in the reference: it is what lets `F.linear` on float32 tensors (the reference's CPU / fp32 path,
 * timesformer.py:47-58,95-99) run on lvl_linear_tn / lvl_linear_wgrad instead of a library GEMM. cols % 4 == 0. */
int lvl_split_bf16x3(const float* src, void* dst, int64_t rows, int cols, int64_t src_row_stride,
                     int64_t dst_row_stride, int64_t dst_term_stride, int role, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* LAVILA_HIP_H */
