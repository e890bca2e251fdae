"""MI355X-native TimeSformer video tower behind the reference's own interface.

Mirrors `lavila/models/timesformer.py` of facebookresearch/LaViLa (class names, constructor
signatures, forward()/forward_features() signatures, parameter/state_dict names, error behaviour),
but the execution plan is ours: no rearrange copies, no materialised attention scores, the
BCTHW->BTCHW permute folded into the patch gather, every residual add fused into the LayerNorm
that consumes it, and every Linear layer (qkv, proj, fc1 + bias + QuickGELU, fc2, patch embedding), the
LayerNorms and the divided space-time attention core run by hand-written HIP kernels through the C ABI
(include/lavila_hip.h: lvl_linear_tn / lvl_linear_wgrad / lvl_layernorm_* / lvl_divided_attn_*). No call of
this file reaches a library GEMM in bf16 unless the shape does not tile (ops.warn_once says so). There is
no CPU path: forward() on a CPU tensor raises. fp16 models / inputs (model.half(), eval_zeroshot.py
--use-half) compute in bf16 and hand fp16 back.
"""
from collections import OrderedDict
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .chain import PendingMlp, ScaledBranch, checkpointed, close, cls_query_attention, compose, triple


# LAVILA_CLS_LAST=0 computes the whole last block as the reference does (A/B and debugging)
CLS_ONLY_LAST_BLOCK = __import__('os').environ.get('LAVILA_CLS_LAST', '1') != '0'


def to_2tuple(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x, x)


def _compute_dtype(weight: torch.Tensor) -> torch.dtype:
    """Activation dtype of the tower: the autocast dtype when autocast is on, else the dtype of the weights;
    fp16 (the reference's AMP dtype, or a model.half()) means bf16 (ops.autocast_dtype / ops.lowp)."""
    lp = ops.autocast_dtype()
    if lp is not None:
        return lp
    return torch.bfloat16 if weight.dtype == torch.float16 else weight.dtype


def _like_caller(out, *given):
    """fp16 in (parameters or input) -> fp16 out, as nn.Module.half() callers expect (eval_zeroshot.py:212-261)."""
    if out.dtype == torch.bfloat16 and not torch.is_autocast_enabled() and \
            any(g is not None and g.dtype == torch.float16 for g in given):
        return out.to(torch.float16)
    return out


class LayerNorm(nn.Module):
    """nn.LayerNorm(dim, eps) with the HIP kernel underneath; same parameter names (weight, bias)."""

    def __init__(self, normalized_shape, eps=1e-5):
        super().__init__()
        dim = normalized_shape if isinstance(normalized_shape, int) else normalized_shape[-1]
        self.normalized_shape = (dim,)
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))
        self.bias = nn.Parameter(torch.zeros(dim))

    def forward(self, x):
        return ops.layer_norm(x, self.weight, self.bias, self.eps)

    def extra_repr(self):
        return f'{self.normalized_shape}, eps={self.eps}'


class DropPath(nn.Module):
    """Per-sample stochastic depth (timm.models.layers.DropPath semantics, timesformer.py:31,161)."""

    def __init__(self, drop_prob=0.0):
        super().__init__()
        self.drop_prob = float(drop_prob)

    def sample_scale(self, batch, device):
        """[batch] float32 of bernoulli(keep) / keep, drawn from the device generator (torch.manual_seed reproduces a run, no
        host read-back): the per-sample factors of one stochastic-depth site, as lvl_droppath_add_layernorm_* take them. The
        only place the fused residual chain draws a mask."""
        keep = 1.0 - self.drop_prob
        return torch.empty(batch, dtype=torch.float32, device=device).bernoulli_(keep).div_(keep)

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep = 1.0 - self.drop_prob
        mask = x.new_empty((x.shape[0],) + (1,) * (x.ndim - 1)).bernoulli_(keep)
        return x * (mask / keep)


class QuickGELUAct(nn.Module):
    """Marker for the fused bias+QuickGELU kernel; calling it standalone applies x*sigmoid(1.702x)."""

    def forward(self, x):
        return ops.bias_quick_gelu(x, None)


def classify_act(act):
    """The activation of an Mlp as the fused MLP kernels know it: ops.ACT_QUICKGELU (QuickGELU: every CLIP_OPENAI_* tower),
    ops.ACT_GELU (nn.GELU with approximate='none', the exact erf GELU: the default of SpaceTimeTransformer, the ImageNet-ViT
    tower of CLIP_HF_TIMESFORMER_DISTILBERT_BASE) or None (anything else -- the tanh approximation included: it runs as the
    module it is, between two Linear kernels)."""
    if type(act).__name__ in ('QuickGELU', 'QuickGELUAct'):
        return ops.ACT_QUICKGELU
    if isinstance(act, nn.GELU) and getattr(act, 'approximate', 'none') == 'none':
        return ops.ACT_GELU
    return None


class Mlp(nn.Module):
    """fc2(act(fc1(x))) -- timesformer.py:42-58. With QuickGELU (all CLIP_OPENAI_* models) the fc1 bias add
    and the activation run as one HIP kernel on the raw GEMM output; on the block chain QuickGELU and the exact GELU both
    live in the GEMM epilogues (`act_kind`, ops.mlp)."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)
        self.act_kind = classify_act(self.act)          # classified once: ops.ACT_QUICKGELU, ops.ACT_GELU or None (unfused)
        self._fused_act = self.act_kind == ops.ACT_QUICKGELU

    def hidden(self, x):
        if self._fused_act:
            return self.drop(ops.bias_quick_gelu(ops.linear(x, self.fc1.weight), self.fc1.bias))
        return self.drop(self.act(ops.linear(x, self.fc1.weight, self.fc1.bias)))

    def forward(self, x):
        return _like_caller(self.drop(ops.linear(self.hidden(x), self.fc2.weight, self.fc2.bias)), x)


class VideoPatchEmbed(nn.Module):
    """Video to patch embedding -- timesformer.py:61-84. `proj` keeps the Conv2d parameter layout
    ([D,3,P,P], bias only when ln_pre=False) so checkpoints interoperate; the computation is the HIP patch
    gather + one GEMM against proj.weight viewed as [D, 3*P*P]."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, num_frames=8, ln_pre=False):
        super().__init__()
        img_size = to_2tuple(img_size)
        patch_size = to_2tuple(patch_size)
        self.img_size = img_size
        self.patch_size = patch_size
        self.num_patches = (img_size[1] // patch_size[1]) * (img_size[0] // patch_size[0]) * num_frames
        self.num_frames = num_frames
        self.embed_dim = embed_dim
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size, bias=not ln_pre)

    def tokens_from_bcthw(self, video):
        """[B,C,F,H,W] -> [B, F*N, D] without the BTCHW copy."""
        assert video.shape[2] <= self.num_frames
        return self._tokens(video, frame_major=False)

    def tokens_from_btchw(self, video):
        """[B,F,C,H,W] (what forward_features / forward receive, timesformer.py:79-84,345-348) -> [B, F*N, D]: the
        gather reads this layout in place as well (no permute().contiguous() round trip of the clip)."""
        ops.refuse_pending(video, 'a frame-major ([B,F,C,H,W]) entry point (forward_features, VideoPatchEmbed.forward)')
        assert video.shape[1] <= self.num_frames
        return self._tokens(video, frame_major=True)

    def _tokens(self, video, frame_major):
        if self.patch_size[0] != self.patch_size[1]:
            raise NotImplementedError('non-square patches')
        return conv_patch_tokens(self.proj, video, self.patch_size[0], frame_major)

    def forward(self, x):
        """Reference signature: x [B,F,C,H,W] -> [B*F, D, H/P, W/P] (timesformer.py:79-84)."""
        ops.refuse_pending(x, 'VideoPatchEmbed.forward (frame-major, [B,F,C,H,W])')
        B, Fr, C, H, W = x.shape
        assert Fr <= self.num_frames
        tok = _like_caller(self.tokens_from_btchw(x), x, self.proj.weight)
        gh, gw = H // self.patch_size[0], W // self.patch_size[1]
        return tok.reshape(B * Fr, gh, gw, -1).permute(0, 3, 1, 2)


_padded_patch_weights = __import__('weakref').WeakKeyDictionary()     # Conv2d module -> (state key, zero-padded [D, 640] weight)


def conv_patch_tokens(conv, video, patch, frame_major):
    """The stride-P Conv2d `conv` (weight [D, 3, P, P], optional bias) on every frame of a clip ([B,C,F,H,W], or
    [B,F,C,H,W] when frame_major) as the HIP patch gather + one GEMM against the weight viewed as [D, 3*P*P]:
    -> [B, F*N, D], rows (b, f, n)-major. Shared by VideoPatchEmbed and openai_model.VisionTransformer."""
    w = conv.weight
    w2 = w.reshape(w.shape[0], -1)
    k = w2.shape[1]
    if isinstance(video, ops.PendingClip):
        # uint8 frames straight to the GEMM operand: the 14 x 14 towers' rows are written 640 wide (zero columns behind
        # 588), so the pad copy below is not paid
        wide = k % 64 and video.is_cuda and w2.shape[0] % 256 == 0
        patches = ops.patchify(video, patch, _compute_dtype(w), frame_major=frame_major, ld=k + (64 - k % 64 if wide else 0))
    else:
        patches = ops.patchify(video, patch, _compute_dtype(w), frame_major=frame_major)
    if k % 64 and patches.is_cuda and w2.shape[0] % 256 == 0:
        # 14 x 14 patches: 3*14*14 = 588 contraction elements. The MFMA GEMMs walk K in blocks of 64: zero columns up
        # to 640 on both operands (exact) keep the patch embedding of the L/14 towers on lvl_linear_tn /
        # lvl_linear_wgrad; the weight gradient comes back through the pad's slice
        pad = 64 - k % 64
        if patches.shape[-1] == k:
            patches = F.pad(patches, (0, pad))
        if torch.is_grad_enabled() and w.requires_grad:
            w2 = F.pad(w2, (0, pad))        # part of the autograd graph: one pad (and one cast) per training step
        else:
            # inference: ONE padded copy per parameter state, so that ops.weight_copies' cache (keyed on the tensor it
            # is handed) hits on every later call instead of re-padding and re-casting per forward
            key = (w._version, w.data_ptr(), ops._generation, w.dtype)
            hit = _padded_patch_weights.get(conv)
            if hit is None or hit[0] != key:
                hit = _padded_patch_weights[conv] = (key, F.pad(w2.detach(), (0, pad)))
            w2 = hit[1]
    return ops.linear(patches, w2, conv.bias)


class VarAttention(nn.Module):
    """Divided attention layer -- timesformer.py:87-144. qkv/proj are plain Linears; everything between them
    (head split, q scaling, CLS-attends-all, per-frame / per-location grouping, softmax, merge) is one C-ABI
    call (lvl_divided_attn_fwd / _bwd)."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0.,
                 initialize='random'):
        super().__init__()
        self.num_heads = num_heads
        head_dim = dim // num_heads
        if head_dim != 64:
            raise NotImplementedError(f'lavila_amd attention kernels are built for head_dim 64, got {head_dim}')
        if qk_scale is not None and abs(qk_scale - head_dim ** -0.5) > 1e-12:
            raise NotImplementedError('qk_scale override')
        self.scale = qk_scale or head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        if initialize == 'zeros':
            self.qkv.weight.data.fill_(0)
            self.qkv.bias.data.fill_(0)
            self.proj.weight.data.fill_(1)
            self.proj.bias.data.fill_(0)
        if attn_drop != 0. or proj_drop != 0.:
            raise NotImplementedError('attention / projection dropout (never used by the reference configs)')
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj_drop = nn.Dropout(proj_drop)

    @staticmethod
    def _mode(einops_to, einops_dims):
        if einops_to.replace(' ', '') == '(bf)nd':
            return 'space', int(einops_dims['f'])
        if einops_to.replace(' ', '') == '(bn)fd':
            return 'time', int(einops_dims['n'])
        raise NotImplementedError(f'einops pattern {einops_to!r}')

    def core(self, x, mode, frames, n_per_frame, want_token=False, ln=None):
        """qkv Linear + attention core; returns the pre-projection tensor [B,T,D] (want_token: and its column-sum token,
        ops.COLSUM_TOKENS -- for callers that hand BOTH to a token-aware consumer and use the tensor nowhere else).
        ln: the ops.LnRecipe of x (selective recompute: the qkv Linear rebuilds x in backward instead of keeping it)."""
        bias = self.qkv.bias
        # the GEMM adds the bias; its gradient comes out of the attention backward call (ops._DividedAttnFn),
        # hence the detached copy for the Linear
        qkv = ops.linear(x, self.qkv.weight, None if bias is None else bias.detach(), ln=ln)
        return ops.divided_attention(qkv, frames, n_per_frame, self.num_heads, mode, bias=bias, want_token=want_token)

    def forward(self, x, einops_from, einops_to, einops_dims):
        mode, k = self._mode(einops_to, einops_dims)
        patches = x.shape[1] - 1
        frames, n = (k, patches // k) if mode == 'space' else (patches // k, k)
        return _like_caller(ops.linear(self.core(x, mode, frames, n), self.proj.weight, self.proj.bias), x)


def _video_checkpoint_mode(use_checkpoint):
    """ops.checkpoint_mode for the video tower: None, 'block' or 'selective'."""
    mode = ops.checkpoint_mode(use_checkpoint)
    if mode == 'selective' and ops.RESIDUAL_F32:
        raise NotImplementedError("use_checkpoint='selective' with the float32 residual stream (LAVILA_RESIDUAL_F32): the "
                                  'LayerNorm outputs there are casts of the kernel output and are not rebuilt')
    return mode


class SpaceTimeBlock(nn.Module):
    """timesformer.py:147-198, 'frozen-in-time' wiring:
         t = x + [tanh(alpha)] * timeattn(norm3(x));  x1 = x + attn(norm1(t));  out = x1 + mlp(norm2(x1))
    """

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0.,
                 drop_path=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm, time_init='zeros',
                 attention_style='frozen-in-time', is_tanh_gating=False):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = VarAttention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale,
                                 attn_drop=attn_drop, proj_drop=drop)
        self.timeattn = VarAttention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale,
                                     attn_drop=attn_drop, proj_drop=drop, initialize=time_init)
        if is_tanh_gating:
            self.alpha_timeattn = nn.Parameter(torch.zeros([]))
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        mlp_hidden_dim = int(dim * mlp_ratio)
        self.mlp = Mlp(in_features=dim, hidden_features=mlp_hidden_dim, act_layer=act_layer, drop=drop)
        self.norm3 = norm_layer(dim)
        self.attention_style = attention_style

    def _stochastic(self):
        """Stochastic depth lives in this training forward: the block stays on the fused chain and its two per-sample
        scaled adds run in the LayerNorm kernels that read them (ops.scaled_add_layer_norm)."""
        return self.training and isinstance(self.drop_path, DropPath) and self.drop_path.drop_prob > 0.

    def _time_half(self, res, pend, pend_bias, frames, n_per_frame, recipe, sel):
        """The first half of a block on the chain: x = res + pend + pend_bias closed into norm3, time attention, its
        projection, norm1 of t = x + time_out. Returns (x, h1, r1): t is never stored; x is handed through so that its second
        use, x + space_out, sends its gradient into norm1's backward kernel instead of a separate add.
        recipe: handed to the close (a pending MLP of the block before then keeps neither its input nor its hidden
        activation); sel: norm3's and norm1's outputs of THIS block are not kept either (r1: the ops.LnRecipe of h1)."""
        if self.attention_style != 'frozen-in-time':
            raise NotImplementedError
        if self.training and self.mlp.drop.p > 0.:
            raise NotImplementedError(f'SpaceTimeBlock on the fused residual chain has no MLP dropout: mlp.drop.p = '
                                      f'{self.mlp.drop.p} must be 0 to train it (no constructor sets it: drop / drop_rate '
                                      '!= 0 raise)')
        x, h3, r3 = close(res, pend, pend_bias, self.norm3, recipe=recipe)
        r3 = r3 if sel else None
        ta, n1 = self.timeattn, self.norm1
        if hasattr(self, 'alpha_timeattn'):
            o_t = ta.core(h3, 'time', frames, n_per_frame, ln=r3)
            y_t = torch.tanh(self.alpha_timeattn).to(o_t.dtype) * ops.linear(o_t, ta.proj.weight, ta.proj.bias)
            b_t = tok_y = None
        else:
            # column-sum tokens (ops.COLSUM_TOKENS): o_t -> projection -> fused add + norm1; the backward hands
            # sum_rows(d o_t) to the attention backward, which needs it for the v third of d(qkv bias)
            o_t, tok_o = ta.core(h3, 'time', frames, n_per_frame, want_token=True, ln=r3)
            (y_t, tok_y), b_t = ops.linear_with_token(o_t, ta.proj.weight, tok_o), ta.proj.bias
        del h3
        return triple(ops.add_layer_norm_pass(x, y_t, b_t, n1.weight, n1.bias, n1.eps, ytoken=tok_y, recipe=sel))

    def _mlp_pending(self, x1, h2, r2=None, defer=False, scale=None):
        """(x1, y, fc2 bias): the block output x1 + y + bias with the MLP branch of h2 = norm2(x1) left pending -- for the
        next consumer to enqueue (PendingMlp: `defer`, ops.RESIDUAL_EPILOGUE, a classified activation, bf16), computed by
        the fused MLP kernels, or composed around an activation they do not know; under stochastic depth (scale: the
        branch's per-sample factors) inside a ScaledBranch. fc2's bias stays pending in every form.
        r2: the ops.LnRecipe of h2 (selective recompute)."""
        m = self.mlp
        if m.act_kind is None:
            y = ops.linear(m.hidden(h2), m.fc2.weight)
        elif (defer and scale is None and ops.RESIDUAL_EPILOGUE and h2.dtype == torch.bfloat16
                and x1.dtype == torch.bfloat16):
            y = PendingMlp(h2, m, r2)
        else:
            y = ops.mlp(h2, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.act_kind, ln=r2)
        return x1, (y if scale is None else ScaledBranch(y, scale)), m.fc2.bias

    def chain(self, res, pend, pend_bias, frames, n_per_frame, defer_mlp=False, selective=False):
        """One block on the fused residual chain (chain.py).

        The block input is x = res + pend + pend_bias (pend/pend_bias may be None); that add is fused into
        norm3. Returns (x1, y, y_bias) with the block output = x1 + y + y_bias left *pending* so that the
        next consumer (next block's norm3 or the final norm) fuses it too.
        selective (use_checkpoint='selective'): the same kernels in the same order, but norm3 / norm1 / norm2's outputs and
        the MLP hidden activation are not kept for backward: every LayerNorm hands out the recipe of its output
        (ops.LnRecipe) and the Linear that consumes the output keeps that instead. A block with stochastic depth keeps every
        activation and runs the scaled adds below."""
        stoch = self._stochastic()
        sel = bool(selective) and not stoch
        # (a pending MLP of the block before is closed in THIS block's mode: its recipe travels with it)
        x, h1, r1 = self._time_half(res, pend, pend_bias, frames, n_per_frame, recipe=sel, sel=sel)
        sa, n2 = self.attn, self.norm2
        if stoch:
            # x1 = x + c_space * (proj(o_s) + bias) inside norm2's kernel, the MLP branch left pending with its own scale: the
            # time branch carries no drop path in the reference (timesformer.py:183-196). Masks in the reference's order.
            c_s = self.drop_path.sample_scale(x.shape[0], x.device)
            c_m = self.drop_path.sample_scale(x.shape[0], x.device)
            o_s = sa.core(h1, 'space', frames, n_per_frame)
            del h1
            x1, h2, _ = close(x, ScaledBranch(ops.linear(o_s, sa.proj.weight), c_s), sa.proj.bias, n2)
            return self._mlp_pending(x1, h2, scale=c_m)
        # ops.RESIDUAL_EPILOGUE: x1 leaves the projection GEMM (residual epilogue), norm2 reads it
        o_s, tok_s = sa.core(h1, 'space', frames, n_per_frame, want_token=True, ln=r1)
        del h1
        x1, h2, r2 = triple(ops.linear_add_layer_norm(o_s, sa.proj.weight, sa.proj.bias, x, n2.weight, n2.bias, n2.eps,
                                                      xtoken=tok_s, recipe=sel))
        return self._mlp_pending(x1, h2, r2, defer=defer_mlp)

    def chain_cls(self, res, pend, pend_bias, frames, n_per_frame, selective=False):
        """The LAST block when only the cls row of its output is read (`norm(x)[:, 0]`, timesformer.py:377): same
        arithmetic as `chain`, restricted to what reaches that row. Time attention, norm1 and the k | v thirds of the space
        qkv run on every token (the cls query of the space attention reads the keys / values of all of them); the q
        third, the attention itself (lvl_cls_attn_*: one query per head), its output projection, norm2 and the whole MLP
        -- 2/3 of a block's flops -- run on the B cls rows only. Exact, like
        the caption trim of the text tower: the skipped rows feed nothing (their gradient is exactly zero in the
        reference, too). Returns (x1, y, y_bias) of the cls rows, [B, D] each.
        selective: reaches the close only, stochastic or not (the pending MLP of the block before keeps neither its input
        nor its hidden activation); this block's own LayerNorm outputs are kept (its MLP runs on B rows)."""
        x, h1, _ = self._time_half(res, pend, pend_bias, frames, n_per_frame, recipe=bool(selective), sel=False)
        sa = self.attn
        y_s = ops.linear(cls_query_attention(h1, sa.qkv.weight, sa.qkv.bias, sa.num_heads), sa.proj.weight)      # [B, D]
        c_s = c_m = None
        if self._stochastic():
            # the two scaled adds of `chain` on the cls rows: one row per sample
            c_s = self.drop_path.sample_scale(x.shape[0], x.device)
            c_m = self.drop_path.sample_scale(x.shape[0], x.device)
        x1, h2, _ = close(x, y_s if c_s is None else ScaledBranch(y_s, c_s), sa.proj.bias, self.norm2, rows=0)
        return self._mlp_pending(x1, h2, scale=c_m)

    def forward(self, x, einops_from_space, einops_to_space, einops_from_time, einops_to_time,
                time_n, space_f, use_checkpoint=False):
        """Reference signature (timesformer.py:173-174); materialises the block output."""
        frames, n = int(space_f), int(time_n)
        mode = _video_checkpoint_mode(use_checkpoint)
        if mode == 'block':
            x1, y, b = checkpointed(self.chain, x, None, None, frames, n)
        else:
            x1, y, b = self.chain(x, None, None, frames, n, selective=mode == 'selective')
        # (a scaled branch: the closing add through the scaled kernel; nothing reads its normalised rows here)
        return _like_caller(compose(x1, y, b, norm_for_scaled=self.norm3, bias_first=True), x)


class SpaceTimeTransformer(nn.Module):
    """Divided space-time ViT -- timesformer.py:201-390 (same constructor, attributes and state_dict)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12,
                 num_heads=12, mlp_ratio=4., qkv_bias=True, qk_scale=None, representation_size=None,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0., hybrid_backbone=None, norm_layer=None,
                 num_frames=8, time_init='rand', attention_style='frozen-in-time', ln_pre=False,
                 act_layer=nn.GELU, is_tanh_gating=False):
        super().__init__()
        self.num_classes = num_classes
        self.num_features = self.embed_dim = embed_dim
        self.num_frames = num_frames
        norm_layer = norm_layer or partial(LayerNorm, eps=1e-6)
        print("######USING ATTENTION STYLE: ", attention_style)
        if hybrid_backbone is not None:
            raise NotImplementedError('hybrid backbone not implemented')
        if drop_rate != 0.:
            raise NotImplementedError('drop_rate != 0 (never used by the reference configs)')
        self.patch_embed = VideoPatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans,
                                           embed_dim=embed_dim, num_frames=num_frames, ln_pre=ln_pre)
        num_patches = self.patch_embed.num_patches
        self.patches_per_frame = num_patches // num_frames

        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.patches_per_frame + 1, embed_dim))
        self.temporal_embed = nn.Parameter(torch.zeros(1, num_frames, embed_dim))
        self.ln_pre = LayerNorm(embed_dim, eps=1e-5) if ln_pre else None
        self.pos_drop = nn.Dropout(p=drop_rate)

        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]
        self.blocks = nn.ModuleList([
            SpaceTimeBlock(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
                           qk_scale=qk_scale, drop=drop_rate, attn_drop=attn_drop_rate, drop_path=dpr[i],
                           norm_layer=norm_layer, time_init=time_init, attention_style=attention_style,
                           act_layer=act_layer, is_tanh_gating=is_tanh_gating)
            for i in range(depth)])
        self.norm = norm_layer(embed_dim)

        if representation_size:
            self.num_features = representation_size
            self.pre_logits = nn.Sequential(OrderedDict([('fc', nn.Linear(embed_dim, representation_size)),
                                                         ('act', nn.Tanh())]))
        else:
            self.pre_logits = nn.Identity()
        self.head = nn.Linear(self.num_features, num_classes) if num_classes > 0 else nn.Identity()

        nn.init.trunc_normal_(self.pos_embed, std=.02)
        nn.init.trunc_normal_(self.cls_token, std=.02)
        if num_frames == 1:
            self.apply(self._init_weights)

        self.einops_from_space = 'b (f n) d'
        self.einops_to_space = '(b f) n d'
        self.einops_from_time = 'b (f n) d'
        self.einops_to_time = '(b n) f d'

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, (nn.LayerNorm, LayerNorm)):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {'pos_embed', 'cls_token'}

    def get_classifier(self):
        return self.head

    def reset_classifier(self, num_classes, global_pool=''):
        self.num_classes = num_classes
        self.head = nn.Linear(self.embed_dim, num_classes) if num_classes > 0 else nn.Identity()

    def _freeze(self, temporal):
        freeze_list = []
        for n, p in self.named_parameters():
            is_temporal = 'temporal_embed' in n or 'timeattn' in n or 'norm3' in n
            if is_temporal == temporal:
                p.requires_grad = False
                freeze_list.append(n)
        print("Freeze the pretrained parts in vision model: {}".format(freeze_list))

    def freeze_spatial_weights(self):
        self._freeze(temporal=False)

    def freeze_temporal_weights(self):
        self._freeze(temporal=True)

    # ------------------------------------------------------------------------------------------------
    def _features_from_tokens(self, tok, frames, use_checkpoint, cls_at_last, after_block=None):
        """tok: [B, F*N, D] patch-embedded tokens (frame-major). after_block: optional (index, callable), called once
        after that block has been enqueued (CLIP.forward starts the text tower from there); an argument of this one
        call, never module state, so concurrent forwards of one or several models cannot see each other's hook."""
        n = self.patches_per_frame
        if tok.shape[1] != frames * n:
            raise ValueError(f'got {tok.shape[1]} patch tokens for {frames} frames; this model was built for '
                             f'{n} patches per frame (img_size / patch_size are fixed at construction)')
        if ops.RESIDUAL_F32 and tok.dtype != torch.float32:
            tok = tok.float()                  # the stream starts in f32, as cat([cls_token f32, half]) does in the reference
        x = ops.embed_tokens(tok, self.cls_token, self.pos_embed, self.temporal_embed, frames, n)
        if self.ln_pre is not None:
            x = ops.layer_norm(x, self.ln_pre.weight, self.ln_pre.bias, self.ln_pre.eps, stream=True)
        x = self.pos_drop(x)
        mode = _video_checkpoint_mode(use_checkpoint)
        res, pend, pend_b = x, None, None
        hook = after_block
        last = len(self.blocks) - 1
        # with stochastic depth in the tower no MLP waits for the next block in the plain step: block checkpointing closes
        # every add in the composed form, and the two modes then run the same kernels (equal to the bit under one seed)
        stochastic = any(blk._stochastic() for blk in self.blocks)
        for i, blk in enumerate(self.blocks):
            # the last block of a cls-pooled forward only has to produce its cls rows (SpaceTimeBlock.chain_cls); any other
            # but the last may leave its MLP to the next block's norm3 (ops.RESIDUAL_EPILOGUE: residual add in fc2's
            # epilogue). 'selective': the plain step's kernels in the plain step's order; what is kept for backward differs
            cls_only = cls_at_last and i == last and CLS_ONLY_LAST_BLOCK and blk.attention_style == 'frozen-in-time'
            fn = blk.chain_cls if cls_only else blk.chain
            how = {} if cls_only else {'defer_mlp': i != last and (mode == 'selective' or not stochastic)}
            if mode == 'block':
                res, pend, pend_b = checkpointed(fn, res, pend, pend_b, frames, n)
            else:
                res, pend, pend_b = fn(res, pend, pend_b, frames, n, selective=mode == 'selective', **how)
            if hook is not None and i == hook[0]:
                hook[1]()
        # the final residual add + LayerNorm; cls_at_last: only row 0 of every sample feeds the output, [B, D]
        out = close(res, pend, pend_b, self.norm, keep_sum=False, rows=0 if cls_at_last else None)[1]
        return self.pre_logits(out) if cls_at_last else out

    def forward_features(self, x, use_checkpoint=False, cls_at_last=True):
        """Reference signature: x is [B, F, C, H, W] (timesformer.py:345-382; the narrator's entry with
        cls_at_last=False, narrator.py:74). The gather reads this layout in place.
        use_checkpoint: False / None, True, 'block' or 'selective' (ops.checkpoint_mode)."""
        with ops.model_forward():
            b, curr_frames, channels, _, _ = x.shape
            tok = self.patch_embed.tokens_from_btchw(x)
            out = self._features_from_tokens(tok, curr_frames, use_checkpoint, cls_at_last)
            return _like_caller(out, x, self.cls_token)

    def forward(self, x, use_checkpoint=False, _after_block=None):
        """x: [B, C, T, H, W] (timesformer.py:384-390); the BCTHW->BTCHW copy is folded into the gather.
        `_after_block` is not part of the reference signature (see _features_from_tokens)."""
        with ops.model_forward():
            tok = self.patch_embed.tokens_from_bcthw(x)
            out = self._features_from_tokens(tok, x.shape[2], use_checkpoint, True, _after_block)
            return self.head(_like_caller(out, x, self.cls_token))
