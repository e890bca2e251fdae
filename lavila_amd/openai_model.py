"""MI355X-native OpenAI CLIP modules behind the reference interface (`lavila/models/openai_model.py`: QuickGELU :177-179,
ResidualAttentionBlock :182-216, Transformer :219-232, VisionTransformer :235-272, CLIP :275-417, convert_weights :420-441,
build_model :444-485).

Same class names, constructor signatures and state_dict keys (attn.in_proj_weight, attn.in_proj_bias,
attn.out_proj.*, ln_1.*, ln_2.*, mlp.c_fc.*, mlp.c_proj.*; conv1.weight, class_embedding, positional_embedding, ln_pre.*,
ln_post.*, proj). The execution is batch-major ([B, L, W]; the reference's NLD<->LND permutes disappear), residual adds are
fused into the LayerNorms, bias+QuickGELU and its backward are epilogues of the c_fc / c_proj GEMMs (lvl_linear_tn), and
the attention core is a C-ABI call: lvl_causal_attn_fwd/_bwd under the causal text mask, and without a mask (the image
tower: full self-attention over [cls + N patches]) lvl_divided_attn_fwd/_bwd in space mode with ONE frame -- the cls query
sees all 1 + N keys and so does every patch query. The `ModifiedResNet` towers (RN50 ... RN50x64) are not built.
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .chain import checkpointed, close, cls_query_attention, compose, take_rows
from .timesformer import LayerNorm, _like_caller, conv_patch_tokens


class QuickGELU(nn.Module):
    """x * sigmoid(1.702 x) -- openai_model.py:177-179 (HIP kernel)."""

    def forward(self, x: torch.Tensor):
        return ops.bias_quick_gelu(x, None)


class _SelfAttentionParams(nn.Module):
    """Parameter container with nn.MultiheadAttention's names (in_proj_weight/in_proj_bias/out_proj)."""

    def __init__(self, d_model: int, n_head: int):
        super().__init__()
        self.embed_dim = d_model
        self.num_heads = n_head
        self.in_proj_weight = nn.Parameter(torch.empty(3 * d_model, d_model))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * d_model))
        self.out_proj = nn.Linear(d_model, d_model)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.constant_(self.out_proj.bias, 0.)


class ResidualAttentionBlock(nn.Module):
    def __init__(self, d_model: int, n_head: int, attn_mask: torch.Tensor = None):
        super().__init__()
        if d_model // n_head != 64:
            raise NotImplementedError('lavila_amd attention kernels are built for head_dim 64')
        self.attn = _SelfAttentionParams(d_model, n_head)
        self.ln_1 = LayerNorm(d_model)
        self.mlp = nn.Sequential(OrderedDict([
            ("c_fc", nn.Linear(d_model, d_model * 4)),
            ("gelu", QuickGELU()),
            ("c_proj", nn.Linear(d_model * 4, d_model))
        ]))
        self.ln_2 = LayerNorm(d_model)
        # The reference passes CLIP.build_attention_mask() (causal, models.py:131-137) for the text tower -- the kernel
        # applies the causal mask analytically -- and no mask for the image tower (openai_model.py:247). Any other mask is
        # rejected loudly.
        if attn_mask is not None:
            L = attn_mask.shape[0]
            causal = torch.full((L, L), float('-inf')).triu_(1)
            # (a mask built on the meta device -- shape inspection without storage -- has no values to compare)
            if attn_mask.shape != causal.shape or not (attn_mask.is_meta or torch.equal(attn_mask.float().cpu(), causal)):
                raise NotImplementedError('only the causal CLIP text mask (or no mask) is supported')
        self.attn_mask = attn_mask

    def _mlp_pending(self, x1, h2):
        return x1, ops.mlp_quickgelu(h2, self.mlp.c_fc.weight, self.mlp.c_fc.bias, self.mlp.c_proj.weight), \
            self.mlp.c_proj.bias

    def chain(self, res, pend, pend_bias):
        """Batch-major block on the fused residual chain (chain.py; see SpaceTimeBlock.chain): the add of the block before
        rides in ln_1's kernel."""
        l2, at = self.ln_2, self.attn
        x, h, _ = close(res, pend, pend_bias, self.ln_1)
        # the GEMM adds the in-proj bias; its gradient comes out of the attention backward (hence the detached copy)
        qkv = ops.linear(h, at.in_proj_weight, at.in_proj_bias.detach())
        tok = None
        if self.attn_mask is not None:
            o = ops.causal_attention(qkv, at.num_heads, bias=at.in_proj_bias)
        else:
            # full self-attention over [cls + N patches] = the space family with one frame; the column-sum token gives
            # the v third of the in-proj bias gradient without a pass over dout (ops.COLSUM_TOKENS), as in SpaceTimeBlock
            o, tok = ops.divided_attention(qkv, 1, h.shape[1] - 1, at.num_heads, 'space', bias=at.in_proj_bias,
                                           want_token=True)
        # x + attn(ln_1(x)) (openai_model.py:199): the residual add rides in out_proj's GEMM epilogue when the shapes
        # are the MFMA GEMM's (ops.RESIDUAL_EPILOGUE), ln_2 reads the sum
        x1, h2 = ops.linear_add_layer_norm(o, at.out_proj.weight, at.out_proj.bias, x, l2.weight, l2.bias, l2.eps, xtoken=tok)
        return self._mlp_pending(x1, h2)

    def chain_rows(self, res, pend, pend_bias, rows):
        """The LAST block when only one position per sample is read afterwards -- exact, see SpaceTimeBlock.chain_cls: the
        skipped rows feed nothing. Returns [B, W] tensors.
        Causal (text tower; `rows` [B] int64: the EOT row, models.py:158-160): the attention runs on every position (row
        `rows[b]` attends to all positions before it), the output projection, ln_2 and the MLP on the B selected rows only.
        No mask (image tower; `rows` must be 0, the cls row, openai_model.py:265): the k | v thirds of the in-proj run on
        every token, the q third, the attention (lvl_cls_attn_*: one query per head), the output projection, ln_2 and the
        MLP on the B cls rows."""
        at = self.attn
        if self.attn_mask is None and not (isinstance(rows, int) and rows == 0):
            raise NotImplementedError('unmasked ResidualAttentionBlock.chain_rows: only the cls row (rows=0)')
        x, h, _ = close(res, pend, pend_bias, self.ln_1)
        if self.attn_mask is not None:
            o = ops.causal_attention(ops.linear(h, at.in_proj_weight, at.in_proj_bias.detach()), at.num_heads,
                                     bias=at.in_proj_bias)
            o_rows = take_rows(o, rows)
        else:
            o_rows = cls_query_attention(h, at.in_proj_weight, at.in_proj_bias, at.num_heads)      # [B, D]
        x1, h2, _ = close(x, ops.linear(o_rows, at.out_proj.weight), at.out_proj.bias, self.ln_2, rows=rows)
        return self._mlp_pending(x1, h2)

    def forward(self, x: torch.Tensor, use_checkpoint=False):
        """Reference signature: x is [L, N, D] (openai_model.py:206-216)."""
        return compose(*self.chain(x.permute(1, 0, 2).contiguous(), None, None)).permute(1, 0, 2)


class Transformer(nn.Module):
    def __init__(self, width: int, layers: int, heads: int, attn_mask: torch.Tensor = None):
        super().__init__()
        self.width = width
        self.layers = layers
        self.resblocks = nn.Sequential(*[ResidualAttentionBlock(width, heads, attn_mask) for _ in range(layers)])

    def forward_batch_major(self, x, final_ln, use_checkpoint=False, rows=None):
        """x: [B, L, W]. Runs all blocks on the fused chain and applies `final_ln` (CLIP.ln_final / VisionTransformer.ln_post);
        final_ln None (the image tower's all-token output, openai_model.py:272) returns the bare block output.
        `rows`: only those token rows are normalised and returned ([B, W]) -- a [B] int64 tensor for the causal tower (the
        EOT rows), the int 0 for the unmasked tower (the cls rows); the last block then runs on those rows only
        (timesformer.CLS_ONLY_LAST_BLOCK).
        use_checkpoint: see ops.checkpoint_mode. 'selective' runs the plain path here: at 32-77 positions of width 512 the
        text tower's activations are about 1 % of the video tower's."""
        from .timesformer import CLS_ONLY_LAST_BLOCK
        step = checkpointed if ops.checkpoint_mode(use_checkpoint) == 'block' else (lambda fn, *a: fn(*a))
        res, pend, pb = x.contiguous(), None, None
        last = len(self.resblocks) - 1
        for i, blk in enumerate(self.resblocks):
            if rows is not None and i == last and CLS_ONLY_LAST_BLOCK:      # only the selected rows leave the tower
                res, pend, pb = step(blk.chain_rows, res, pend, pb, rows)
            else:
                res, pend, pb = step(blk.chain, res, pend, pb)
        if rows is None and final_ln is None:
            return compose(res, pend, pb)
        return close(res, pend, pb, final_ln, keep_sum=False, rows=rows)[1]

    def forward(self, x: torch.Tensor, use_checkpoint=False):
        """Reference signature: [L, N, D] -> [L, N, D] (openai_model.py:226-232)."""
        res, pend, pb = x.permute(1, 0, 2).contiguous(), None, None
        for blk in self.resblocks:
            res, pend, pb = blk.chain(res, pend, pb)
        return compose(res, pend, pb).permute(1, 0, 2)


class VisionTransformer(nn.Module):
    """openai_model.py:235-272: the per-frame image tower of the OpenAI CLIP models (`CLIP_OPENAI_VIT*`) and of the per-frame
    narrators (`VCLM_OPENAI_VIT*`). Same parameters and initialisation; the patch embedding is the HIP patch gather + one
    GEMM against conv1.weight viewed as [W, 3*P*P], the tokens are assembled by lvl_embed_tokens_* with one frame and no
    temporal embedding, the blocks run on the fused residual chain. Input float32 / fp16 / bf16; bf16 inside under
    autocast or with fp16 / bf16 parameters, the f32 class otherwise."""

    def __init__(self, input_resolution: int, patch_size: int, width: int, layers: int, heads: int, output_dim: int):
        super().__init__()
        self.input_resolution = input_resolution
        self.output_dim = output_dim
        self.conv1 = nn.Conv2d(in_channels=3, out_channels=width, kernel_size=patch_size, stride=patch_size, bias=False)

        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn((input_resolution // patch_size) ** 2 + 1, width))
        self.ln_pre = LayerNorm(width)

        self.transformer = Transformer(width, layers, heads)

        self.ln_post = LayerNorm(width)
        self.proj = nn.Parameter(scale * torch.randn(width, output_dim))

    def _from_tokens(self, tok, apply_project, use_checkpoint, cls_at_last):
        """tok [n, N, W]: the patch-embedded tokens of n images -> [n, output_dim] (cls_at_last) or [n, N, W]."""
        n_patches = self.positional_embedding.shape[0] - 1
        if tok.shape[1] != n_patches:
            raise ValueError(f'got {tok.shape[1]} patch tokens per image; this tower was built for {n_patches} '
                             '(input_resolution / patch_size are fixed at construction)')
        if ops.RESIDUAL_F32 and tok.dtype != torch.float32:
            tok = tok.float()                  # the stream starts in f32, as cat([class_embedding f32, half]) would
        W = tok.shape[-1]
        x = ops.embed_tokens(tok, self.class_embedding.view(1, 1, W), self.positional_embedding.unsqueeze(0), None, 1,
                             n_patches)
        x = ops.layer_norm(x, self.ln_pre.weight, self.ln_pre.bias, self.ln_pre.eps, stream=True)
        if not cls_at_last:
            # no ln_post on this path, as in the reference (openai_model.py:271-272)
            return self.transformer.forward_batch_major(x, None, use_checkpoint=use_checkpoint)[:, 1:, :]
        x = self.transformer.forward_batch_major(x, self.ln_post, use_checkpoint=use_checkpoint, rows=0)
        if self.proj is not None and apply_project:
            if x.dtype != self.proj.dtype and not torch.is_autocast_enabled():
                x = x.to(self.proj.dtype)        # fp16 images into an f32 model, or the reverse
            x = ops.project(x, self.proj)
        return x

    def _patch(self):
        return self.conv1.kernel_size[0]

    def forward(self, x: torch.Tensor, apply_project=True, use_checkpoint=False, cls_at_last=True):
        """x [n, 3, H, W] -> ln_post(x[:, 0]) (@ proj) [n, output_dim], or with cls_at_last=False the patch rows of the last
        block's output [n, N, W] (openai_model.py:252-272). use_checkpoint: ops.checkpoint_mode."""
        if x.dim() != 4:
            raise ValueError(f'VisionTransformer.forward takes [n, 3, H, W] images, got {tuple(x.shape)}')
        with ops.model_forward():
            tok = conv_patch_tokens(self.conv1, x.unsqueeze(2), self._patch(), False)          # one frame per image
            out = self._from_tokens(tok, apply_project, use_checkpoint, cls_at_last)
            return _like_caller(out, x, self.conv1.weight)

    def forward_clip(self, video, apply_project=True, use_checkpoint=False, cls_at_last=True):
        """Not in the reference: video [B, C, T, H, W] -> what `forward` gives for
        `video.permute(0, 2, 1, 3, 4).reshape(-1, C, H, W)` (CLIP.encode_image, openai_model.py:376-378; narrator.py:66-68),
        rows (b, t)-major, without that copy of the clip: the patch gather reads BCTHW in place."""
        if video.dim() != 5:
            raise ValueError(f'VisionTransformer.forward_clip takes [B, 3, T, H, W] clips, got {tuple(video.shape)}')
        with ops.model_forward():
            tok = conv_patch_tokens(self.conv1, video, self._patch(), False)                   # [B, T*N, W]
            tok = tok.reshape(video.shape[0] * video.shape[2], -1, tok.shape[-1])
            out = self._from_tokens(tok, apply_project, use_checkpoint, cls_at_last)
            return _like_caller(out, video, self.conv1.weight)


class CLIP(nn.Module):
    """openai_model.py:275-417: the OpenAI CLIP dual encoder (per-frame image tower, frame embeddings averaged), the
    paper's zero-shot baseline. `forward` returns the dict of lavila_amd.models.CLIP, so the same drivers and CLIPLoss
    run it. The text side is models.CLIP's (the `text_embed` kernel, caption trim, row-only last block)."""

    def __init__(self,
                 embed_dim: int,
                 # vision
                 image_resolution: int,
                 vision_layers,
                 vision_width: int,
                 vision_patch_size: int,
                 # text
                 context_length: int,
                 vocab_size: int,
                 transformer_width: int,
                 transformer_heads: int,
                 transformer_layers: int
                 ):
        super().__init__()

        self.context_length = context_length

        if isinstance(vision_layers, (tuple, list)):
            raise NotImplementedError(f'openai_model.CLIP: vision_layers={tuple(vision_layers)} asks for the ModifiedResNet '
                                      'image tower (RN50 ... RN50x64), which is not built; only the VisionTransformer '
                                      'towers (an int number of layers)')
        vision_heads = vision_width // 64
        self.visual = VisionTransformer(
            input_resolution=image_resolution,
            patch_size=vision_patch_size,
            width=vision_width,
            layers=vision_layers,
            heads=vision_heads,
            output_dim=embed_dim
        )

        self.transformer = Transformer(
            width=transformer_width,
            layers=transformer_layers,
            heads=transformer_heads,
            attn_mask=self.build_attention_mask()
        )

        self.vocab_size = vocab_size
        self.token_embedding = nn.Embedding(vocab_size, transformer_width)
        self.positional_embedding = nn.Parameter(torch.empty(self.context_length, transformer_width))
        self.ln_final = LayerNorm(transformer_width)

        self.text_projection = nn.Parameter(torch.empty(transformer_width, embed_dim))
        self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))

        self.initialize_parameters()

    def initialize_parameters(self):
        """openai_model.py:331-358 (only the text tower is re-initialised, as there)."""
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)

        proj_std = (self.transformer.width ** -0.5) * ((2 * self.transformer.layers) ** -0.5)
        attn_std = self.transformer.width ** -0.5
        fc_std = (2 * self.transformer.width) ** -0.5
        for block in self.transformer.resblocks:
            nn.init.normal_(block.attn.in_proj_weight, std=attn_std)
            nn.init.normal_(block.attn.out_proj.weight, std=proj_std)
            nn.init.normal_(block.mlp.c_fc.weight, std=fc_std)
            nn.init.normal_(block.mlp.c_proj.weight, std=proj_std)

        if self.text_projection is not None:
            nn.init.normal_(self.text_projection, std=self.transformer.width ** -0.5)

    def build_attention_mask(self):
        """Additive causal mask (openai_model.py:360-366); the HIP kernel applies it analytically."""
        mask = torch.empty(self.context_length, self.context_length)
        mask.fill_(float("-inf"))
        mask.triu_(1)
        return mask

    @property
    def dtype(self):
        return self.visual.conv1.weight.dtype

    def encode_image(self, image, apply_project=True, use_checkpoint=False):
        """openai_model.py:372-382. [n, 3, H, W]: per-image features (always projected, the arguments are not passed on, as
        in the reference); [B, 3, T, H, W]: the tower per frame, frame features averaged over T."""
        from .models import _amp_region, _half_out
        with ops.model_forward(), _amp_region():
            if image.ndim == 4:
                return _half_out(self.visual(image), image, self.visual.conv1.weight)
            bb, tt = image.shape[0], image.shape[2]
            x = self.visual.forward_clip(image, apply_project=apply_project, use_checkpoint=use_checkpoint)    # [B*T, D]
            return _half_out(x.view(bb, tt, -1).mean(1), image, self.visual.conv1.weight)

    def _eot_rows(self, text):
        from .models import CLIP as _VideoCLIP
        return _VideoCLIP._eot_rows(self, text)

    def encode_text(self, text, use_checkpoint=False):
        """openai_model.py:384-397 through models.CLIP.encode_text: the same attributes (token_embedding,
        positional_embedding, transformer, ln_final, text_projection) drive the same kernels."""
        from .models import CLIP as _VideoCLIP
        return _VideoCLIP.encode_text(self, text, use_checkpoint=use_checkpoint)

    def forward(self, image, text, use_checkpoint=False, norm_embed=True):
        """openai_model.py:399-417: the embeddings are always L2-normalised (`norm_embed` is accepted and unused, as in the
        reference), logit_scale is exp'd."""
        ops.checkpoint_mode(use_checkpoint)           # anything else raises here, before a kernel is enqueued
        with ops.model_forward():
            image_features = self.encode_image(image, use_checkpoint=use_checkpoint)
            text_features = self.encode_text(text, use_checkpoint=use_checkpoint)
            return {'image_embed': F.normalize(image_features.float(), dim=-1),
                    'text_embed': F.normalize(text_features.float(), dim=-1),
                    'logit_scale': self.logit_scale.exp()}


def convert_weights(model: nn.Module):
    """Convert applicable model parameters to fp16 (openai_model.py:420-441; host-side)."""

    def _convert_weights_to_fp16(l):
        if isinstance(l, (nn.Conv1d, nn.Conv2d, nn.Linear)):
            l.weight.data = l.weight.data.half()
            if l.bias is not None:
                l.bias.data = l.bias.data.half()

        if isinstance(l, (nn.MultiheadAttention, _SelfAttentionParams)):
            for attr in [*[f"{s}_proj_weight" for s in ["in", "q", "k", "v"]], "in_proj_bias", "bias_k", "bias_v"]:
                tensor = getattr(l, attr, None)
                if tensor is not None:
                    tensor.data = tensor.data.half()

        for name in ["text_projection", "proj"]:
            if hasattr(l, name):
                attr = getattr(l, name)
                if attr is not None:
                    attr.data = attr.data.half()

    model.apply(_convert_weights_to_fp16)


def build_model(state_dict: dict):
    """openai_model.py:444-485: the ten constructor arguments from the tensor shapes of an OpenAI CLIP state dict, the
    weights loaded (strict). The result is float32 in eval mode: the reference converts to fp16 here and every caller
    (openai_clip.load on the CPU) converts back with .float(), which leaves the published fp16 values unchanged."""
    if "visual.proj" not in state_dict:
        counts = [len(set(k.split(".")[2] for k in state_dict if k.startswith(f"visual.layer{b}"))) for b in [1, 2, 3, 4]]
        raise NotImplementedError(f'openai_model.build_model: a ModifiedResNet state dict (visual.layer1..4 with {counts} '
                                  'blocks); only the VisionTransformer CLIPs are built')
    vision_width = state_dict["visual.conv1.weight"].shape[0]
    vision_layers = len(
        [k for k in state_dict.keys() if k.startswith("visual.") and k.endswith(".attn.in_proj_weight")]
    )
    vision_patch_size = state_dict["visual.conv1.weight"].shape[-1]
    grid_size = round((state_dict["visual.positional_embedding"].shape[0] - 1) ** 0.5)
    image_resolution = vision_patch_size * grid_size

    embed_dim = state_dict["text_projection"].shape[1]
    context_length = state_dict["positional_embedding"].shape[0]
    vocab_size = state_dict["token_embedding.weight"].shape[0]
    transformer_width = state_dict["ln_final.weight"].shape[0]
    transformer_heads = transformer_width // 64
    transformer_layers = len(set(k.split(".")[2] for k in state_dict if k.startswith("transformer.resblocks")))

    model = CLIP(
        embed_dim,
        image_resolution, vision_layers, vision_width, vision_patch_size,
        context_length, vocab_size, transformer_width, transformer_heads, transformer_layers
    )

    state_dict = {k: v for k, v in state_dict.items() if k not in ("input_resolution", "context_length", "vocab_size")}
    model.load_state_dict(state_dict)
    return model.float().eval()
