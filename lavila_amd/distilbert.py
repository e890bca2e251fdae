"""DistilBERT as the text tower of `CLIP_HF` (reference lavila/models/models.py:176-290, 494-657: transformers'
`DistilBertModel` behind `self.textual`), on the HIP kernels.

`DistilBertModel(config)` keeps transformers' parameter names, shapes, order and initialisation
(`embeddings.{word_embeddings,position_embeddings,LayerNorm}`, `transformer.layer.N.attention.{q_lin,k_lin,v_lin,out_lin}`,
`sa_layer_norm`, `ffn.{lin1,lin2}`, `output_layer_norm`), so `load_state_dict(hf_model.state_dict(), strict=True)` works both
ways and the `textual.*` keys of a LaViLa checkpoint load strictly. `embeddings.position_ids` is a non-persistent buffer as
in current transformers; the key is accepted and dropped when an older checkpoint carries it.

Plan per layer (post-LN, eps 1e-12; modeling_distilbert.py): ops.text_embed + ops.layer_norm; q_lin / k_lin / v_lin as three
ops.linear calls; ops.keymask_attention (lvl_keymask_attn_fwd / _bwd: keys hidden per sample by the padding mask);
LN(out_lin(o) + x) through ops.linear_residual_layer_norm / ops.add_layer_norm; lin1, the exact erf GELU (lvl_act_fwd / _bwd,
LVL_ACT_GELU_ERF), lin2 + residual + output_layer_norm. Under bf16 autocast or `.half()` it computes in bf16 like the CLIP
text tower (attention on the key-masked MFMA kernels up to 256 positions); in float32 it runs the f32-class GEMMs and the
shape-generic attention kernels.

Stated differences from transformers: head dim 64 only; `sinusoidal_pos_embds`, head masks, `inputs_embeds`, `position_ids`,
`output_attentions` / `output_hidden_states` raise NotImplementedError; there is no dropout -- `distilbert_config()` holds
dropout = attention_dropout = 0.0 (transformers' DistilBertConfig and `from_pretrained` carry 0.1) and a training-mode
forward with a non-zero probability raises NotImplementedError naming the fields. `gradient_checkpointing_enable / _disable`
are no-ops (models.py:250-257 skips checkpointing for DistilBERT anyway).
"""
import os
import types

import torch
import torch.nn as nn

from . import _cabi as C
from . import ops
from .gpt2_gated import _ActFn

_SIZES = {'distilbert-base-uncased': dict(vocab_size=30522, max_position_embeddings=512, dim=768, n_heads=12, n_layers=6,
                                          hidden_dim=3072)}
_TEXT_TRIM = os.environ.get('LAVILA_TEXT_TRIM', '1') != '0'


def distilbert_config(name='distilbert-base-uncased', **overrides):
    """The fields of transformers' DistilBertConfig that the tower reads, for the published size -- so that the
    `*_DISTILBERT_BASE` constructors work without the hub. A real DistilBertConfig is accepted everywhere instead.
    dropout / attention_dropout are 0.0 here (transformers: 0.1): the tower has no dropout."""
    cfg = types.SimpleNamespace(activation='gelu', initializer_range=0.02, pad_token_id=0, sinusoidal_pos_embds=False,
                                dropout=0.0, attention_dropout=0.0, **_SIZES[name])
    for k, v in overrides.items():
        setattr(cfg, k, v)
    return cfg


class BaseModelOutput(types.SimpleNamespace):
    """`.last_hidden_state` [B, L, D], the one field CLIP_HF reads (models.py:264-271)."""


class _PadRowFn(torch.autograd.Function):
    """The embedding table as nn.Embedding(padding_idx=...) differentiates it: the padding row receives no gradient."""

    @staticmethod
    def forward(ctx, table, pad):
        ctx.pad = pad
        return table.view_as(table)

    @staticmethod
    def backward(ctx, dtable):
        dtable = dtable.clone()
        dtable[ctx.pad].zero_()
        return dtable, None


class Embeddings(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.word_embeddings = nn.Embedding(config.vocab_size, config.dim, padding_idx=config.pad_token_id)
        self.position_embeddings = nn.Embedding(config.max_position_embeddings, config.dim)
        self.LayerNorm = nn.LayerNorm(config.dim, eps=1e-12)
        self.register_buffer('position_ids', torch.arange(config.max_position_embeddings).expand((1, -1)),
                             persistent=False)

    def forward(self, input_ids):
        we, pe, ln = self.word_embeddings, self.position_embeddings, self.LayerNorm
        L = input_ids.shape[1]
        if L > pe.weight.shape[0]:
            raise ValueError(f'{L} positions exceed max_position_embeddings = {pe.weight.shape[0]}')
        half = we.weight.dtype in (torch.float16, torch.bfloat16)
        act = torch.bfloat16 if half else (ops.autocast_dtype() or torch.float32)
        table = we.weight
        if we.padding_idx is not None and table.requires_grad and torch.is_grad_enabled():
            table = _PadRowFn.apply(table, int(we.padding_idx))
        x = ops.text_embed(input_ids, table, pe.weight, act)         # gather + add, one kernel
        if x is None:                                                 # .half() tables: the gather itself is plumbing
            x = ops.lowp(nn.functional.embedding(input_ids, table) + pe.weight[:L]).to(act)
        return ops.layer_norm(x, ln.weight, ln.bias, ln.eps, stream=True)


class MultiHeadSelfAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.n_heads, self.dim = config.n_heads, config.dim
        self.q_lin = nn.Linear(config.dim, config.dim)
        self.k_lin = nn.Linear(config.dim, config.dim)
        self.v_lin = nn.Linear(config.dim, config.dim)
        self.out_lin = nn.Linear(config.dim, config.dim)


class FFN(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.lin1 = nn.Linear(config.dim, config.hidden_dim)
        self.lin2 = nn.Linear(config.hidden_dim, config.dim)


class TransformerBlock(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.attention = MultiHeadSelfAttention(config)
        self.sa_layer_norm = nn.LayerNorm(config.dim, eps=1e-12)
        self.ffn = FFN(config)
        self.output_layer_norm = nn.LayerNorm(config.dim, eps=1e-12)

    def forward(self, x, keymask, row0=False):
        """x [B, L, D] -> [B, L, D]; row0: only position 0 of every sample is asked for (the LAST layer under CLIP_HF):
        q_lin, the attention's queries, out_lin, both LayerNorms and the FFN run on B rows, k_lin / v_lin on all -- exact,
        as ResidualAttentionBlock.chain_rows. Returns [B, D] then."""
        at, l1, l2, ff = self.attention, self.sa_layer_norm, self.output_layer_norm, self.ffn
        xq = x[:, 0].contiguous().unsqueeze(1) if row0 else x
        q = ops.linear(xq, at.q_lin.weight, at.q_lin.bias)
        k = ops.linear(x, at.k_lin.weight, at.k_lin.bias)
        v = ops.linear(x, at.v_lin.weight, at.v_lin.bias)
        o = ops.keymask_attention(q, k, v, keymask, at.n_heads)
        if row0:
            o, xq = o.squeeze(1), xq.squeeze(1)
        fused = ops.linear_residual_layer_norm(o, at.out_lin.weight, at.out_lin.bias, xq, l1.weight, l1.bias, l1.eps)
        if fused is not None:
            h = fused[1]
        else:
            h = ops.add_layer_norm(xq, ops.linear(o, at.out_lin.weight), at.out_lin.bias, l1.weight, l1.bias, l1.eps,
                                   keep_sum=False)[1]
        a = _ActFn.apply(ops.linear(h, ff.lin1.weight, ff.lin1.bias), C.ACT_GELU_ERF)
        fused = ops.linear_residual_layer_norm(a, ff.lin2.weight, ff.lin2.bias, h, l2.weight, l2.bias, l2.eps)
        if fused is not None:
            return fused[1]
        return ops.add_layer_norm(h, ops.linear(a, ff.lin2.weight), ff.lin2.bias, l2.weight, l2.bias, l2.eps,
                                  keep_sum=False)[1]


class Transformer(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.n_layers = config.n_layers
        self.layer = nn.ModuleList([TransformerBlock(config) for _ in range(config.n_layers)])


def _cfg(config, name, default=None):
    return getattr(config, name, default)


class DistilBertModel(nn.Module):
    def __init__(self, config):
        super().__init__()
        if _cfg(config, 'dim') != _cfg(config, 'n_heads') * 64:
            raise NotImplementedError(f'lavila_amd attention kernels are built for head_dim 64, got '
                                      f'{_cfg(config, "dim")}/{_cfg(config, "n_heads")}')
        if _cfg(config, 'sinusoidal_pos_embds', False):
            raise NotImplementedError('sinusoidal_pos_embds is not built (distilbert-base-uncased learns its positions)')
        if _cfg(config, 'activation', 'gelu') != 'gelu':
            raise NotImplementedError(f'only DistilBERT\'s exact "gelu" activation is built, got {config.activation!r}')
        if _cfg(config, 'dim') % 8 or _cfg(config, 'hidden_dim') % 8:
            raise NotImplementedError('dim and hidden_dim must be multiples of 8')
        self.config = config
        self.embeddings = Embeddings(config)
        self.transformer = Transformer(config)
        self.apply(self._init_weights)

    def _init_weights(self, m):
        """PreTrainedModel._init_weights as DistilBertModel(config) runs it."""
        std = _cfg(self.config, 'initializer_range', 0.02)
        if isinstance(m, nn.Linear):
            nn.init.normal_(m.weight, mean=0.0, std=std)
            nn.init.zeros_(m.bias)
        elif isinstance(m, nn.Embedding):
            nn.init.normal_(m.weight, mean=0.0, std=std)
            if m.padding_idx is not None:
                with torch.no_grad():
                    m.weight[m.padding_idx].zero_()
        elif isinstance(m, nn.LayerNorm):
            nn.init.ones_(m.weight)
            nn.init.zeros_(m.bias)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        state_dict.pop(prefix + 'embeddings.position_ids', None)      # a persistent buffer of older transformers
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def gradient_checkpointing_enable(self, *args, **kwargs):
        """No-op: the reference skips checkpointing for DistilBERT (models.py:250-257)."""

    def gradient_checkpointing_disable(self):
        """No-op."""

    def get_input_embeddings(self):
        return self.embeddings.word_embeddings

    def _refuse(self, kwargs):
        bad = [k for k, v in kwargs.items() if v is not None and v is not False]
        if bad:
            raise NotImplementedError(f'DistilBertModel.forward: {", ".join(sorted(bad))} is not on the CLIP_HF path '
                                      '(built: input_ids and attention_mask)')
        drop = [k for k in ('dropout', 'attention_dropout') if float(_cfg(self.config, k, 0.0) or 0.0) != 0.0]
        if self.training and drop:
            raise NotImplementedError(f'the DistilBERT tower has no dropout: config.{" / ".join(drop)} must be 0.0 to train '
                                      'it (transformers\' DistilBertConfig defaults them to 0.1; distilbert_config() holds '
                                      '0.0), or call .eval()')

    @staticmethod
    def _keymask(input_ids, attention_mask):
        """uint8 [B, L], non-zero = visible, or None; any real or bool dtype comes in (the reference's tokenizer hands
        float32, tokenizer.py:189-208)."""
        if attention_mask is None:
            return None
        if attention_mask.dim() != 2 or attention_mask.shape != input_ids.shape:
            raise ValueError(f'attention_mask {tuple(attention_mask.shape)} must be [batch, positions] = '
                             f'{tuple(input_ids.shape)}')
        if attention_mask.is_complex():
            raise ValueError('attention_mask must be of a real or bool dtype')
        return (attention_mask != 0).to(torch.uint8)

    def _run(self, input_ids, attention_mask, row0, trim):
        if input_ids is None:
            raise ValueError('You have to specify input_ids')
        if input_ids.dim() != 2:
            raise ValueError(f'input_ids must be [batch, positions], got {tuple(input_ids.shape)}')
        keymask = self._keymask(input_ids, attention_mask)
        if not input_ids.is_cuda:
            C.require_device(input_ids)              # raises HipExtensionError: there is no CPU path
        if (trim and keymask is not None and _TEXT_TRIM and input_ids.shape[1] > 1
                and not torch.cuda.is_current_stream_capturing()):
            # columns behind the last visible position of the batch feed no visible row and are never asked for: one host
            # read of a scalar, as CLIP.encode_text's
            pos = torch.arange(1, keymask.shape[1] + 1, device=keymask.device)
            longest = max(1, int((keymask.to(torch.int64) * pos).max().item()))
            input_ids, keymask = input_ids[:, :longest], keymask[:, :longest]
        if keymask is not None:
            keymask = keymask.contiguous()
        from .timesformer import CLS_ONLY_LAST_BLOCK
        x = self.embeddings(input_ids)
        last = len(self.transformer.layer) - 1
        for i, blk in enumerate(self.transformer.layer):
            x = blk(x, keymask, row0=row0 and i == last and CLS_ONLY_LAST_BLOCK)
        return x[:, 0] if (row0 and x.dim() == 3) else x

    def forward(self, input_ids=None, attention_mask=None, head_mask=None, inputs_embeds=None, position_ids=None,
                output_attentions=None, output_hidden_states=None, return_dict=None, **kwargs):
        self._refuse(dict(head_mask=head_mask, inputs_embeds=inputs_embeds, position_ids=position_ids,
                          output_attentions=output_attentions, output_hidden_states=output_hidden_states, **kwargs))
        if return_dict is not None and not return_dict:
            raise NotImplementedError('DistilBertModel.forward: return_dict=False is not on the CLIP_HF path')
        with ops.model_forward():
            return BaseModelOutput(last_hidden_state=self._run(input_ids, attention_mask, False, False))

    def first_rows(self, input_ids, attention_mask=None):
        """[B, D]: `forward(...).last_hidden_state[:, 0]`, what CLIP_HF.encode_text reads (text_use_cls_token), with two
        exact savings: the batch is trimmed to its longest caption and the last layer runs on row 0 only."""
        self._refuse({})
        with ops.model_forward():
            return self._run(input_ids, attention_mask, True, True)
