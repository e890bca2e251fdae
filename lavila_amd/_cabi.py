"""ctypes binding of liblavila_hip.so (the C ABI declared in include/lavila_hip.h).

There is NO fallback: if the library is missing or a tensor is not on an MI355X device the call raises.
PyTorch is used for device memory and streams only (tensor.data_ptr(), torch.cuda.current_stream()).
"""
import ctypes
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'liblavila_hip.so')

LVL_F32, LVL_BF16 = 0, 1
LVL_F16 = 2          # lvl_clip_ingest's output only
ATTN_SPACE, ATTN_TIME = 0, 1
# The epilogues of lvl_linear_tn (LVL_EPI_* of the header; csrc/gemm_tn_kernel.h holds the library's table):
# name -> (code, two_out: writes aux_out, colsum: reads aux_in and leaves column sums, f32: exists in the f32-class mode).
# 6-8 are the exact (erf) GELU twins of 1, 2, 4. Every name is a module constant too (C.EPI_BIAS, ...).
TN_EPILOGUES = {
    'EPI_BIAS': (0, False, False, True),
    'EPI_BIAS_QUICKGELU': (1, True, False, True),
    'EPI_QUICKGELU_BWD': (2, False, True, True),
    'EPI_BIAS_RESIDUAL': (3, False, False, True),
    'EPI_BIAS_QUICKGELU_DERIV': (4, True, False, False),
    'EPI_MUL_AUX_COLSUM': (5, False, True, False),
    'EPI_BIAS_GELU': (6, True, False, True),
    'EPI_GELU_BWD': (7, False, True, True),
    'EPI_BIAS_GELU_DERIV': (8, True, False, False),
}
globals().update({_name: _row[0] for _name, _row in TN_EPILOGUES.items()})
LN_PLAIN, LN_GENERAL = 1, 2          # flags of lvl_layernorm_*_mixed
ACT_GELU_NEW, ACT_SQRELU, ACT_GELU_ERF = 0, 1, 2

_c = ctypes
_P, _I, _L, _F = _c.c_void_p, _c.c_int, _c.c_int64, _c.c_float
_U64, _U32 = _c.c_uint64, _c.c_uint32

# name -> (restype, argtypes); must list every function of include/lavila_hip.h
SIGNATURES = {
    'lvl_version': (_c.c_char_p, []),
    'lvl_set_compute_units': (_I, [_I]),
    'lvl_set_gemm_mfma_shape': (_I, [_I]),
    'lvl_debug_late_workgroups': (_I, [_I]),
    'lvl_last_error': (_c.c_char_p, []),
    'lvl_workspace_floats': (_L, [_c.c_char_p, _L, _L]),
    'lvl_layernorm_fwd': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _F, _I, _P]),
    'lvl_layernorm_bwd': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _P]),
    'lvl_layernorm_fwd_mixed': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _F, _I, _P]),
    'lvl_layernorm_bwd_mixed': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _P]),
    'lvl_droppath_add_layernorm_fwd': (_I, [_P] * 10 + [_L, _L, _I, _F, _I, _P]),
    'lvl_droppath_add_layernorm_bwd': (_I, [_P] * 13 + [_L, _L, _I, _I, _P]),
    'lvl_layernorm_apply': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _P]),
    'lvl_quickgelu_apply': (_I, [_P, _P, _L, _I, _I, _P]),
    'lvl_bias_quickgelu_fwd': (_I, [_P, _P, _P, _L, _I, _I, _P]),
    'lvl_bias_quickgelu_bwd': (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _I, _P]),
    'lvl_patchify': (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    'lvl_embed_tokens_fwd': (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    # (frames u8, params i32 [B,8], flip i32 [B] | NULL, out, B, F, H, W, S, [P, ld,] clip / frame / row stride in bytes,
    #  mean x3, std x3, dtype, stream)
    'lvl_clip_ingest': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _L, _L, _L] + [_F] * 6 + [_I, _P]),
    'lvl_clip_ingest_patches': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _L, _L, _L, _L] + [_F] * 6 + [_I, _P]),
    'lvl_divided_attn_fwd': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    'lvl_divided_attn_bwd': (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    'lvl_attention_fast_path': (_I, [_I, _I, _I, _I]),
    'lvl_attention_fast_path_f32': (_I, [_I, _I, _I, _I]),
    'lvl_debug_f32_generic': (_I, [_I]),
    'lvl_debug_space_stream': (_I, [_I]),
    'lvl_debug_stream_variant': (_I, [_I]),
    'lvl_set_fp8_qk': (_I, [_I]),
    'lvl_debug_generic_attention_calls': (_I, [_I]),
    'lvl_causal_attn_fwd': (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    'lvl_causal_attn_bwd': (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    'lvl_clip_loss_fwd': (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _P]),
    'lvl_clip_loss_bwd': (_I, [_P, _P, _P, _P, _P, _F, _I, _I, _I, _I, _I, _P, _P, _I, _P]),
    'lvl_ssl_clip_loss_fwd': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _P]),
    'lvl_ssl_clip_loss_bwd': (_I, [_P, _P, _P, _P, _P, _P, _F, _I, _I, _I, _I, _P, _P, _I, _P]),
    'lvl_margin_loss_prepare': (_I, [_P, _P, _P, _F, _I, _I, _P, _I, _P]),
    'lvl_margin_loss_fwd': (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _I, _P]),
    'lvl_margin_loss_bwd': (_I, [_P, _P, _P, _P, _F, _I, _I, _I, _I, _P, _P, _I, _P]),
    'lvl_token_xent_fwd': (_I, [_P, _L, _P, _L, _L, _I, _L, _P, _P, _P, _P, _P, _I, _P]),
    'lvl_token_xent_reduce': (_I, [_P, _P, _P, _I, _I, _P, _P]),
    'lvl_token_xent_bwd': (_I, [_P, _L, _P, _L, _P, _P, _F, _L, _I, _L, _P, _I, _P]),
    'lvl_linear_tn': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _P]),
    'lvl_linear_tn_ragged': (_I, [_P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _P]),
    'lvl_linear_wgrad': (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _P]),
    'lvl_linear_wgrad_plan': (_I, [_L, _I, _I, _c.POINTER(_I)]),
    'lvl_linear_wgrad_pair_of_block': (_I, [_I, _I, _I]),
    'lvl_cast_transpose': (_I, [_P, _P, _P, _I, _I, _P]),
    'lvl_cast_transpose_multi': (_I, [_P, _I, _L, _P]),
    'lvl_split_bf16x3': (_I, [_P, _P, _L, _I, _L, _L, _L, _I, _P]),
    'lvl_cls_attn_fwd': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    'lvl_cls_attn_bwd': (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    'lvl_mq_cross_attn_fwd': (_I, [_P, _L, _P, _P, _I, _I, _I, _I, _I, _P]),
    'lvl_mq_cross_attn_bwd_ws': (_L, [_I, _I, _I, _I]),
    'lvl_mq_cross_attn_bwd': (_I, [_P, _L, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    'lvl_qkv_bias_grad': (_I, [_P, _P, _P, _P, _L, _I, _I, _P]),
    'lvl_divided_attn_bwd_bias_ws': (_L, [_I, _I, _I, _I, _I, _I]),
    'lvl_divided_attn_bwd_bias': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    'lvl_vec_mat_f32': (_I, [_P, _P, _P, _I, _I, _P]),
    'lvl_embed_tokens_bwd_ws': (_L, [_I, _I, _I]),
    'lvl_embed_tokens_bwd': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    'lvl_text_embed_fwd': (_I, [_P, _L, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    'lvl_text_embed_bwd_ws': (_L, [_I, _I, _I]),
    # (dx, tokens, tok_stride, dtable | NULL, dpos | NULL, ws (NULL allowed with a NULL dtable), B, L, W, V, ctx, dtype, stream)
    'lvl_text_embed_bwd': (_I, [_P, _P, _L, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    'lvl_debug_time_bwd_rider': (_I, [_I]),
    'lvl_linear_skinny': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    'lvl_linear_skinny_f32c': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    'lvl_linear_skinny_ln': (_I, [_P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    'lvl_sample_max_vocab': (_I, []),
    'lvl_sample_next_token': (_I, [_P, _L, _I, _I, _F, _I, _F, _P, _P, _L, _P, _P, _P, _P, _P]),
    'lvl_gpt2_embed': (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    'lvl_gated_add_layernorm': (_I, [_P, _P, _P, _P, _P, _F, _P, _P, _I, _I, _I, _P]),
    'lvl_act_inplace': (_I, [_P, _L, _I, _I, _P]),
    'lvl_gated_add_layernorm_train': (_I, [_P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _I, _I, _I, _P]),
    'lvl_gated_add_layernorm_bwd': (_I, [_P] * 14 + [_I, _I, _I, _P]),
    'lvl_act_fwd': (_I, [_P, _P, _L, _I, _I, _P]),
    'lvl_act_bwd': (_I, [_P, _P, _P, _L, _I, _I, _P]),
    'lvl_cross_attn_rows_bwd': (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    'lvl_decode_self_attn': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    'lvl_cross_attn_rows_fwd': (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    'lvl_dropout_mask': (_I, [_P, _L, _U64, _U64, _U32, _F, _P]),
    'lvl_dropout_apply': (_I, [_P, _P, _L, _U64, _U32, _F, _I, _P]),
    'lvl_gated_add_layernorm_train_drop': (_I, [_P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _I, _I, _U64, _U32, _F, _I, _P]),
    'lvl_gated_add_layernorm_bwd_drop': (_I, [_P] * 14 + [_I, _I, _U64, _U32, _F, _I, _P]),
    'lvl_attn_rows_drop_fwd': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _L, _L, _L, _I, _U64, _U32, _F, _I, _P]),
    'lvl_attn_rows_drop_bwd': (_I, [_P] * 7 + [_I, _I, _I, _I, _L, _L, _L, _I, _U64, _U32, _F, _I, _P]),
    'lvl_keymask_attn_fwd': (_I, [_P] * 5 + [_I, _I, _I, _I, _L, _L, _L, _L, _I, _P]),
    'lvl_keymask_attn_bwd': (_I, [_P] * 9 + [_I, _I, _I, _I, _L, _L, _L, _L, _I, _P]),
    'lvl_keymask_attn_drop_fwd': (_I, [_P] * 5 + [_I, _I, _I, _I, _L, _L, _L, _L, _I, _U64, _U32, _F, _I, _P]),
    'lvl_keymask_attn_drop_bwd': (_I, [_P] * 9 + [_I, _I, _I, _I, _L, _L, _L, _L, _I, _U64, _U32, _F, _I, _P]),
    'lvl_dropout_add_layernorm_fwd': (_I, [_P, _P, _P, _P, _F, _P, _P, _P, _P, _I, _I, _L, _U64, _U32, _F, _I, _P]),
    'lvl_dropout_add_layernorm_bwd': (_I, [_P] * 11 + [_I, _I, _L, _U64, _U32, _F, _I, _P]),
    'lvl_rows_pack': (_I, [_P, _L, _L, _P, _I, _I, _I, _P, _I, _P]),
    'lvl_rows_unpack': (_I, [_P, _P, _I, _I, _I, _P, _L, _L, _I, _P]),
}

_lib = None
_lock = threading.Lock()


class HipExtensionError(RuntimeError):
    pass


def lib():
    """Loads liblavila_hip.so once. Raises HipExtensionError (never falls back) if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise HipExtensionError(
                    f'{LIB_PATH} is missing: build it with `python -m lavila_amd.build` '
                    '(or __graft_entry__.build()); lavila_amd has no CPU / eager fallback')
            try:
                handle = ctypes.CDLL(LIB_PATH)
            except OSError as e:
                raise HipExtensionError(f'cannot load {LIB_PATH}: {e}') from e
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(handle, name)
                fn.restype = res
                fn.argtypes = args
            cus = os.environ.get('LAVILA_COMPUTE_UNITS')        # CUs for the persistent GEMM kernels (see the header)
            if cus and handle.lvl_set_compute_units(int(cus)) != 0:
                raise HipExtensionError('LAVILA_COMPUTE_UNITS: ' + handle.lvl_last_error().decode(errors='replace'))
            _lib = handle
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().lvl_last_error().decode(errors='replace')
        raise HipExtensionError(f'{what} failed (status {rc}): {msg}')


def dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return LVL_F32
    if t.dtype == torch.bfloat16:
        return LVL_BF16
    raise HipExtensionError(
        f'lavila_amd kernels take float32 or bfloat16 activations, got {t.dtype} '
        '(fp16 autocast is remapped to bf16 by the model wrappers; see INTEGRATION.md)')


def require_device(*tensors):
    """Every kernel is queued on the CURRENT device's current stream (stream_ptr): tensors must live there."""
    cur = None
    for t in tensors:
        if t is None:
            continue
        if t.is_cuda:
            if cur is None:
                cur = torch.cuda.current_device()
            if t.device.index != cur:
                raise HipExtensionError(
                    f'lavila_amd: tensor on {t.device} but the current device is cuda:{cur}; call '
                    'torch.cuda.set_device() (one process per GPU) before running the model')
        if not t.is_cuda:
            raise HipExtensionError(
                'lavila_amd: tensor on %s -- the HIP kernels need a ROCm device tensor; there is no CPU '
                'fallback (the CPU oracle under oracle/ is test infrastructure only)' % t.device)
        if not t.is_contiguous():
            raise HipExtensionError('lavila_amd: non-contiguous tensor passed to a HIP kernel')


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def workspace(op: str, rows: int, cols: int, device) -> torch.Tensor:
    n = lib().lvl_workspace_floats(op.encode(), rows, cols)
    if n < 0:
        raise HipExtensionError(f'unknown workspace op {op}')
    return torch.empty(max(int(n), 1), dtype=torch.float32, device=device)
