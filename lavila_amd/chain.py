"""The fused residual chain of the pre-norm towers (timesformer.SpaceTimeBlock / SpaceTimeTransformer,
openai_model.ResidualAttentionBlock / Transformer).

A block does not add its last branch to the residual stream. It returns (res, pend, pend_bias) and the block output
`res + pend + pend_bias` stays pending until the next consumer's LayerNorm, whose kernel does the add. The `pend` slot holds
None (nothing to add), a tensor, a PendingMlp (an MLP that has not run yet: its second GEMM adds the residual in its
epilogue) or a ScaledBranch (stochastic depth: the add takes one factor per sample). Two functions read the slot: `close`
(the sum and its normalised rows, for whatever consumes the block output through a LayerNorm) and `compose` (the sum as a
tensor, for the reference-signature forwards). `checkpointed` carries the triple through torch.utils.checkpoint."""
import torch
import torch.utils.checkpoint as checkpoint

from . import ops


class PendingMlp:
    """A block's `x1 + mlp(norm2(x1))` that has not been computed yet: with ops.RESIDUAL_EPILOGUE the MLP's second GEMM adds
    the residual in its epilogue and the NEXT consumer's LayerNorm reads the sum, so the MLP is enqueued by that consumer
    (close -> ops.mlp_residual_layer_norm). Travels in the `pend` slot; the fc2 bias in `pend_bias`."""

    __slots__ = ('h', 'mlp', 'ln')

    def __init__(self, h, mlp, ln=None):
        self.h, self.mlp, self.ln = h, mlp, ln      # ln: the ops.LnRecipe of h (selective recompute), or None

    def materialize(self):
        """The MLP branch as a tensor (fc2's bias still pending), for consumers that want the composed form."""
        m = self.mlp
        return ops.mlp(self.h, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.act_kind, ln=self.ln)


class ScaledBranch:
    """A branch output that is still to be added as `res + scale[sample] * (y + bias)`: a branch of a block with stochastic
    depth (timesformer.py:192,196). Travels in the `pend` slot like a tensor; close and compose add it with
    ops.scaled_add_layer_norm."""

    __slots__ = ('y', 'scale')

    def __init__(self, y, scale):
        self.y, self.scale = y, scale       # scale: [B] float32 (DropPath.sample_scale)


def _rows_per_sample(x):
    return 1 if x.dim() == 2 else x.numel() // (x.shape[0] * x.shape[-1])


def take_rows(t, rows):
    """The selected row of every sample of [B, L, W]: `rows` is a [B] int64 tensor (the EOT rows of the text tower) or the
    int 0 (the cls rows of the image and video towers)."""
    if isinstance(rows, int):
        return t[:, rows].contiguous()
    return t[torch.arange(t.shape[0], device=t.device), rows].contiguous()


def triple(out):
    """(s, h) or (s, h, recipe) of one of ops' add + LayerNorm forms as (s, h, recipe or None)."""
    return out if len(out) == 3 else (*out, None)


def close(res, pend, pend_bias, norm, *, keep_sum=True, recipe=False, rows=None):
    """(s, h, recipe or None) with s = res + pend + pend_bias and h = norm(s), in one LayerNorm kernel (a PendingMlp: its two
    GEMMs, then the plain LayerNorm). With pend None s is res.
    keep_sum=False: nothing reads s (a final norm); it may come back as None.
    recipe: also the ops.LnRecipe of h, for the Linear that consumes h (selective recompute); a PendingMlp's own recipe
    travels with it; a scaled sum has none (the Linear keeps h).
    rows (None, the int 0 or a [B] int64 tensor): only those rows of a [B, L, W] res / pend are summed and normalised."""
    w, b, eps = norm.weight, norm.bias, norm.eps
    if isinstance(pend, PendingMlp) and (rows is not None or not keep_sum):
        raise NotImplementedError('a PendingMlp is closed on every row, by a consumer that reads the sum')
    if rows is not None and res.dim() == 3:
        res = take_rows(res, rows)
    if pend is None:
        out = ops.layer_norm(res, w, b, eps, recipe=recipe)
        return (res, *out) if recipe else (res, out, None)
    if isinstance(pend, ScaledBranch):
        y = take_rows(pend.y, rows) if (rows is not None and pend.y.dim() == 3) else pend.y
        return triple(ops.scaled_add_layer_norm(res, y, pend_bias, pend.scale, _rows_per_sample(res), w, b, eps))
    if isinstance(pend, PendingMlp):
        m = pend.mlp
        fused = ops.mlp_residual_layer_norm(pend.h, m.fc1.weight, m.fc1.bias, m.fc2.weight, pend_bias, res, w, b, eps,
                                            ln=pend.ln, recipe=recipe, act=m.act_kind)
        if fused is not None:
            return triple(fused)
        pend = pend.materialize()
    elif rows is not None and pend.dim() == 3:
        pend = take_rows(pend, rows)
    return triple(ops.add_layer_norm(res, pend, pend_bias, w, b, eps, keep_sum=keep_sum, recipe=recipe))


def compose(res, pend, pend_bias, norm_for_scaled=None, bias_first=False):
    """The block output res + pend + pend_bias as a tensor: the reference-signature forwards and a tower without a final norm.
    A ScaledBranch is added by the scaled kernel under `norm_for_scaled`'s detached parameters (nothing reads the
    normalised rows). bias_first: res + (pend + pend_bias), the order SpaceTimeBlock.forward has always summed in."""
    if pend is None:
        return res
    if isinstance(pend, ScaledBranch):
        n = norm_for_scaled
        return ops.scaled_add_layer_norm(res, pend.y, pend_bias, pend.scale, _rows_per_sample(res), n.weight.detach(),
                                         n.bias.detach(), n.eps)[0]
    if isinstance(pend, PendingMlp):
        raise NotImplementedError('a PendingMlp is closed by the LayerNorm of the next consumer (close)')
    bias = pend_bias.to(pend.dtype)
    return res + (pend + bias) if bias_first else res + pend + bias


def cls_query_attention(h, qkv_weight, qkv_bias, heads):
    """Full self-attention of [B, T, D] rows h for the cls query alone -> [B, D]: the k | v thirds of the qkv Linear on every
    token, the q third on the B cls rows, lvl_cls_attn_* (one query per head). The GEMMs add the (detached) bias; its
    gradient comes out of the attention backward."""
    D = h.shape[-1]
    bq, bkv = (None, None) if qkv_bias is None else (qkv_bias.detach()[:D], qkv_bias.detach()[D:])
    kv = ops.linear(h, qkv_weight[D:], bkv)                                  # [B, T, 2D]
    q = ops.linear(h[:, 0].contiguous(), qkv_weight[:D], bq)                 # [B, D]
    return ops.cls_attention(q, kv, heads, bias=qkv_bias)


def _chain_flat(fn, res, pend, pend_b, pend_c, *args):
    """`fn` (a block's chain method) with a ScaledBranch taken apart into tensors on the way in and out: what
    torch.utils.checkpoint carries across a block boundary. Returns (res, pend, pend_bias, pend_scale or None)."""
    if pend_c is not None:
        pend = ScaledBranch(pend, pend_c)
    res, pend, pend_b = fn(res, pend, pend_b, *args)
    if isinstance(pend, ScaledBranch):
        return res, pend.y, pend_b, pend.scale
    return res, pend, pend_b, None


def checkpointed(fn, res, pend, pend_bias, *args):
    """fn(res, pend, pend_bias, *args) -> (res, pend, pend_bias) under torch.utils.checkpoint (block checkpointing)."""
    y, c = (pend.y, pend.scale) if isinstance(pend, ScaledBranch) else (pend, None)
    res, y, pend_bias, c = checkpoint.checkpoint(_chain_flat, fn, res, y, pend_bias, c, *args, use_reentrant=False)
    return res, (y if c is None else ScaledBranch(y, c)), pend_bias
