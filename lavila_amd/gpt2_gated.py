"""The narrator's text decoder -- GPT-2 with gated cross-attention (lavila/models/gpt2_gated.py), MI355X-native, for
inference and bf16 training (BASELINE configs[4]: captioning).

Module and parameter names are the reference's (`transformer.{wte,wpe,ln_f}`, `transformer.h.{i}.{ln_1, attn.{c_attn,
c_proj}, ln_2, mlp.{c_fc,c_proj}, crossattention.{c_attn,q_attn,c_proj}, ln_cross_attn, mlp_crossattention.{c_fc,c_proj},
ln_2_crossattention, alpha_cattn, alpha_dense}`, `lm_head`; Conv1D weights stay [in, out]; the `attn.bias` /
`attn.masked_bias` mask buffers are kept as state) so that `text_decoder.*` of a reference VCLM checkpoint loads with
strict=True. The modules only HOLD parameters. The computation is ONE plan (`_run_blocks`: the order of Conv1Ds, gates and
add + LayerNorm hand-overs) over one of two primitive sets, which share `_lay_out`'s role names; every C entry point has
one call site:

`_Pack`, inference (everything under torch.no_grad(), teacher-forced or decoding):
  * the Conv1D GEMMs run on lvl_linear_tn / lvl_linear_skinny against a packed image of the weights (bf16, [out, in], built
    once per parameter state; the vocabulary is padded to the GEMM's 256-column tiles), f32 models (the parity
    configuration) on the same kernels' f32-class mode against bf16 term images;
  * every residual add (with its tanh(alpha) gate) is fused with the LayerNorm that reads the sum next
    (lvl_gated_add_layernorm) and, while decoding, both are folded into the prologue of the Conv1D that consumes the
    normalised rows (lvl_linear_skinny_ln); the embedding is one gather (lvl_gpt2_embed);
  * teacher-forced forward (`GPT2LMHeadModel.forward`, what VCLM_HF.forward and target scoring call): the causal
    self-attention is lvl_causal_attn_fwd, the cross-attention lvl_cross_attn_rows_fwd over keys / values projected from
    the image tokens ONCE per clip;
  * decoding (`GPT2LMHeadModel.decode_session`, what VCLM_HF.generate drives): ONE new row per caption and step against
    a key/value cache (lvl_decode_self_attn); the position is a device scalar, so a single captured hipGraph is replayed
    for every step. The reference re-runs the whole prefix per token (narrator.py:118-143, `use_cache=False`): same
    numbers, quadratically more work.

`_TrainOps`, training (`GPT2LMHeadModel.forward` with gradients enabled and a trainable decoder parameter, or image tokens
that require a gradient: the frozen-LM recipe with a trainable pooler): the same primitives as small
torch.autograd.Functions on the modules' own parameters, chained by autograd -- Conv1D on lvl_linear_tn / lvl_linear_wgrad
(no weight gradient for a frozen weight), gated add + LayerNorm (lvl_gated_add_layernorm_train / _bwd), the activations
(lvl_act_fwd / lvl_act_bwd), cross-attention (lvl_cross_attn_rows_fwd / _bwd, at most 256 image tokens), ops.causal_attention,
the embedding (lvl_text_embed_fwd / _bwd) and the tied lm_head, whose weight gradient adds into wte's. bf16 only (bf16
parameters, or float32 masters under bf16 autocast): float32 with gradients raises NotImplementedError.
`gradient_checkpointing_enable()` is a no-op.

Dropout (transformers' GPT2Config defaults resid_pdrop, embd_pdrop and attn_pdrop to 0.1, so the reference's narrators were
trained with all three: gpt2_gated.py:186-187, 230, 354, 389-395, 737, 899) is OPT-IN: LAVILA_DECODER_DROPOUT=1 in the
environment or `gpt2_gated.DECODER_DROPOUT = True`, read when a forward or gpt2_config() runs. Off (the default) a non-zero
probability in training mode raises NotImplementedError as before and gpt2_config() defaults the three to 0.0. On,
gpt2_config() defaults them to transformers' values and the training plan applies them inside the kernels that already
touch the data: the embedding (lvl_dropout_apply), every residual add (lvl_gated_add_layernorm_train_drop / _bwd_drop) and
the probabilities of both attentions (lvl_attn_rows_drop_fwd / _bwd, which then also takes the causal self-attention, at most
256 positions). No mask is stored: forward and backward regenerate it from (seed, site, element) -- csrc/dropout.h,
Philox4x32-10; sites in the reference's execution order: 0 the embedding, block i 1 + 6 i + {0 cross-attention
probabilities, 1 cross c_proj, 2 mlp_crossattention, 3 self-attention probabilities, 4 self c_proj, 5 mlp}. One 64-bit seed
per training forward comes from torch's CPU generator (torch.manual_seed reproduces a run; no device read-back);
`fixed_dropout_seed(seed)` pins it. The distribution is the reference's, the random stream is not. A
probability of 0 takes exactly the path without dropout; inference, decoding, .eval() and no_grad never drop.

Packed rows: `forward(..., row_lengths=[B] lengths)` runs the plan on the first len_b positions of every sequence only, as
R = sum len_b packed rows (PackedRows over lvl_rows_pack / lvl_rows_unpack, csrc/pack_rows.hip): the embedding is packed, every
row primitive and the lm_head see R rows, each attention runs its kernels on the zero-filled rectangle [B, longest] between an
unpack and a pack, and `.logits` keeps its shape with exact zeros at and behind len_b. Both primitive sets take it through the
one plan; without the keyword nothing of it is reached. What makes it exact for a causal decoder whose dropped positions carry
ignored labels: DESIGN.md section 4; lavila_amd.narrator.PACK_CAPTIONS switches it on for VCLM_HF.forward.

What the reference's vendored HF class offers beyond this (attention / head masks, token types, past_key_values as
arguments, pruning, model parallelism, the other heads) raises NotImplementedError.
"""
import contextlib
import copy
import os
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _cabi as C
from . import ops

# rows up to which a Conv1D goes to lvl_linear_skinny (one workgroup per 16/32 weight columns) instead of the
# 256x256-tile kernel: a decode step of 64 captions measured 32 us per GEMM on the latter (one CU per 256-column panel);
# the upper end is measured on the teacher-forced pass (rows = captions x positions): the reference's recompute schedule for
# 64 captions x 77 tokens takes 479 / 432 / 345 / 410 ms with the limit at 1024 / 2048 / 8192 / 65536 rows
SKINNY_MAX_ROWS = int(os.environ.get('LAVILA_SKINNY_MAX_ROWS', '8192'))
# rows up to which the residual add + LayerNorm in front of a Conv1D is folded into that GEMM (lvl_linear_skinny_ln)
FUSED_LN_MAX_ROWS = 128

_SIZES = {  # hidden, layers, heads of the published GPT-2 checkpoints (models.py:729,770,914: "gpt2", "gpt2-large", "gpt2-xl")
    'gpt2': (768, 12, 12), 'gpt2-medium': (1024, 24, 16), 'gpt2-large': (1280, 36, 20), 'gpt2-xl': (1600, 48, 25),
}


# Decoder dropout switch: None = follow LAVILA_DECODER_DROPOUT in the environment, True / False = set here. Read per call
# (decoder_dropout_enabled), never cached.
DECODER_DROPOUT = None
# what transformers.GPT2Config() holds for resid_pdrop / embd_pdrop / attn_pdrop (tests/test_decoder_dropout_cpu.py compares
# them with the installed transformers)
_HF_PDROP = {'resid_pdrop': 0.1, 'embd_pdrop': 0.1, 'attn_pdrop': 0.1}
ATTN_DROP_MAX_KEYS = 256
_fixed_seed = None


def decoder_dropout_enabled():
    if DECODER_DROPOUT is not None:
        return bool(DECODER_DROPOUT)
    return os.environ.get('LAVILA_DECODER_DROPOUT', '0') == '1'


@contextlib.contextmanager
def fixed_dropout_seed(seed):
    """Every training forward inside draws `seed` (64 bits) instead of a fresh seed from torch's generator."""
    global _fixed_seed
    prev, _fixed_seed = _fixed_seed, int(seed) & 0xffffffffffffffff
    try:
        yield
    finally:
        _fixed_seed = prev


def _draw_seed():
    """One 64-bit seed per training forward from torch's CPU generator: torch.manual_seed reproduces it, ranks seeded
    differently differ, and nothing is read back from the device."""
    if _fixed_seed is not None:
        return _fixed_seed
    lo, hi = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()
    return (hi << 32) | lo


def gpt2_config(name='gpt2', **overrides):
    """The fields of transformers' GPT2Config that the decoder reads, for the published sizes -- so that the VCLM_*
    constructors work without the hub (there is no network here). A real GPT2Config is accepted everywhere instead."""
    width, layers, heads = _SIZES[name]
    pdrop = _HF_PDROP if decoder_dropout_enabled() else dict.fromkeys(_HF_PDROP, 0.0)
    cfg = types.SimpleNamespace(
        vocab_size=50257, n_positions=1024, n_embd=width, n_layer=layers, n_head=heads, n_inner=None,
        activation_function='gelu_new', layer_norm_epsilon=1e-5, initializer_range=0.02, scale_attn_weights=True,
        scale_attn_by_inverse_layer_idx=False, reorder_and_upcast_attn=False, tie_word_embeddings=True,
        add_cross_attention=False, bos_token_id=50256, eos_token_id=50256, use_cache=False,
        # transformers' GPT2Config defaults these three to 0.1, so the reference's decoder trains WITH dropout; here that is
        # opt-in (decoder_dropout_enabled): off, they default to 0.0 and a non-zero value refuses to train
        # (GPT2LMHeadModel._train_ops)
        **pdrop)
    for k, v in overrides.items():
        setattr(cfg, k, v)
    return cfg


def augment_gpt2_config(config, cross_attn_freq=1, gated_xattn=True):
    """gpt2_gated.py:84-90."""
    new_config = copy.deepcopy(config)
    new_config.add_cross_attention = True
    new_config.add_cross_attention_freq = cross_attn_freq
    new_config.is_tanh_gating = gated_xattn
    return new_config


def _cfg(config, name, default=None):
    aliases = {'n_embd': 'hidden_size', 'n_layer': 'num_hidden_layers', 'n_head': 'num_attention_heads',
               'n_positions': 'max_position_embeddings'}
    if hasattr(config, name):
        return getattr(config, name)
    if name in aliases and hasattr(config, aliases[name]):
        return getattr(config, aliases[name])
    return default


class Conv1D(nn.Module):
    """transformers.pytorch_utils.Conv1D as gpt2_gated.py:184-188,383-384 uses it: y = x @ weight + bias with
    weight [in, out] (normal std 0.02), bias [out] zeros."""

    def __init__(self, nf, nx):
        super().__init__()
        self.nf = nf
        self.weight = nn.Parameter(torch.empty(nx, nf))
        self.bias = nn.Parameter(torch.zeros(nf))
        nn.init.normal_(self.weight, std=0.02)


class GPT2Attention(nn.Module):
    """Parameter holder of gpt2_gated.py:149-189 (self-attention: c_attn -> 3*D; cross-attention: q_attn on the text,
    c_attn -> 2*D on the image tokens; c_proj)."""

    def __init__(self, config, is_cross_attention=False, layer_idx=None):
        super().__init__()
        D, P = _cfg(config, 'n_embd'), _cfg(config, 'n_positions')
        self.register_buffer('bias', torch.tril(torch.ones((P, P), dtype=torch.uint8)).view(1, 1, P, P))
        self.register_buffer('masked_bias', torch.tensor(-1e4))
        self.embed_dim = D
        self.num_heads = _cfg(config, 'n_head')
        self.head_dim = D // self.num_heads
        self.is_cross_attention = is_cross_attention
        self.layer_idx = layer_idx
        if is_cross_attention:
            self.c_attn = Conv1D(2 * D, D)
            self.q_attn = Conv1D(D, D)
        else:
            self.c_attn = Conv1D(3 * D, D)
        self.c_proj = Conv1D(D, D)


class GPT2MLP(nn.Module):
    """gpt2_gated.py:379-396: c_fc -> gelu_new (or relu^2 in the cross-attention MLP) -> c_proj."""

    def __init__(self, intermediate_size, config, squared_relu=False):
        super().__init__()
        D = _cfg(config, 'n_embd')
        self.c_fc = Conv1D(intermediate_size, D)
        self.c_proj = Conv1D(D, intermediate_size)
        self.squared_relu = squared_relu


class GPT2Block(nn.Module):
    """gpt2_gated.py:399-419."""

    def __init__(self, config, layer_idx=None):
        super().__init__()
        D = _cfg(config, 'n_embd')
        inner = _cfg(config, 'n_inner') or 4 * D
        eps = _cfg(config, 'layer_norm_epsilon', 1e-5)
        self.ln_1 = nn.LayerNorm(D, eps=eps)
        self.attn = GPT2Attention(config, layer_idx=layer_idx)
        self.ln_2 = nn.LayerNorm(D, eps=eps)
        self.add_cross_attention_freq = _cfg(config, 'add_cross_attention_freq', 1)
        if _cfg(config, 'add_cross_attention', False) and layer_idx % self.add_cross_attention_freq == 0:
            self.crossattention = GPT2Attention(config, is_cross_attention=True, layer_idx=layer_idx)
            self.ln_cross_attn = nn.LayerNorm(D, eps=eps)
            self.mlp_crossattention = GPT2MLP(inner, config, squared_relu=True)
            self.ln_2_crossattention = nn.LayerNorm(D, eps=eps)
            if _cfg(config, 'is_tanh_gating', False):
                self.alpha_cattn = nn.Parameter(torch.zeros([]))
                self.alpha_dense = nn.Parameter(torch.zeros([]))
        self.mlp = GPT2MLP(inner, config)

    @property
    def has_cross(self):
        return hasattr(self, 'crossattention')


class GPT2Model(nn.Module):
    """gpt2_gated.py:726-747 (parameters)."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        D = _cfg(config, 'n_embd')
        self.embed_dim = D
        self.wte = nn.Embedding(_cfg(config, 'vocab_size'), D)
        self.wpe = nn.Embedding(_cfg(config, 'n_positions'), D)
        self.h = nn.ModuleList([GPT2Block(config, layer_idx=i) for i in range(_cfg(config, 'n_layer'))])
        self.ln_f = nn.LayerNorm(D, eps=_cfg(config, 'layer_norm_epsilon', 1e-5))
        std = _cfg(config, 'initializer_range', 0.02)
        nn.init.normal_(self.wte.weight, std=std)
        nn.init.normal_(self.wpe.weight, std=std)


class CausalLMOutput:
    """What VCLM_HF reads of transformers' CausalLMOutputWithCrossAttentions: `.logits`, `.loss`, `[0]`."""

    def __init__(self, logits, loss=None):
        self.logits, self.loss, self.past_key_values = logits, loss, None

    def __getitem__(self, i):
        return (((self.loss,) if self.loss is not None else ()) + (self.logits,))[i]


# --------------------------------------------------------------------------------------------------
# device-side image of the parameters + the plan that runs on it
# --------------------------------------------------------------------------------------------------
def _pad_rows(t, multiple):
    n = -t.shape[0] % multiple
    return t if n == 0 else torch.cat([t, t.new_zeros(n, *t.shape[1:])])


def _tanh_gate(alpha):
    return None if alpha is None else torch.tanh(alpha.detach().to(torch.float32)).reshape(1)


def _lay_out(p, model, conv, ln, gate):
    """What both primitive sets know of the model: its geometry and, per block, the plan's operands under ONE set of role
    names. conv(Conv1D), ln(LayerNorm) and gate(alpha parameter or None) give a set's own representation of each."""
    tr = model.transformer
    p.D, p.heads, p.eps = tr.embed_dim, tr.h[0].attn.num_heads, float(tr.ln_f.eps)
    p.vocab, p.positions = tr.wte.weight.shape[0], tr.wpe.weight.shape[0]
    p.blocks = []
    for blk in tr.h:
        e = {'ln_1': ln(blk.ln_1), 'c_attn': conv(blk.attn.c_attn), 'c_proj': conv(blk.attn.c_proj),
             'ln_2': ln(blk.ln_2), 'fc': conv(blk.mlp.c_fc), 'proj': conv(blk.mlp.c_proj), 'cross': blk.has_cross}
        if blk.has_cross:
            e.update({'ln_x': ln(blk.ln_cross_attn), 'xq': conv(blk.crossattention.q_attn),
                      'xkv': conv(blk.crossattention.c_attn), 'xproj': conv(blk.crossattention.c_proj),
                      'ln_2x': ln(blk.ln_2_crossattention), 'xfc': conv(blk.mlp_crossattention.c_fc),
                      'xfproj': conv(blk.mlp_crossattention.c_proj),
                      'gate_c': gate(getattr(blk, 'alpha_cattn', None)), 'gate_d': gate(getattr(blk, 'alpha_dense', None))})
        p.blocks.append(e)
    p.ln_f = ln(tr.ln_f)


class PackedRows:
    """The row layout of a forward with `row_lengths`: caption b keeps its first len_b of L positions, the plan's rows are the
    R = sum len_b kept ones in caption order (ops.pack_rows / ops.unpack_rows over `cu`, the [B + 1] int32 offsets on the
    device). The attentions run on the rectangle [B, longest] with zeros behind a caption's rows (`around`); the plan hands
    this object to `cross_attn` where an unpacked forward hands the positions per caption."""

    def __init__(self, lengths, L, device):
        self.lengths, self.B, self.L = lengths, len(lengths), L
        self.longest, self.rows = max(lengths), sum(lengths)
        cu = [0]
        for n in lengths:
            cu.append(cu[-1] + n)
        self.cu = torch.tensor(cu, dtype=torch.int32).to(device)

    def pack(self, x):
        """[B, positions, W] -> [R, W]."""
        return ops.pack_rows(x, self.cu, self.rows)

    def unpack(self, y, positions):
        """[R, W] -> [B, positions, W] with zeros behind every caption's rows (positions >= the longest caption)."""
        return ops.unpack_rows(y, self.cu, self.B, positions)

    def around(self, attention, y):
        """attention([B * longest, W] rows of the zero-filled rectangle) -> [B * longest, D], on the packed rows y."""
        out = attention(self.unpack(y, self.longest).reshape(self.B * self.longest, -1))
        return self.pack(out.reshape(self.B, self.longest, -1))


def _row_lengths_on_host(row_lengths, B, L):
    """What can be said about `row_lengths` without a read-back: -> (the lengths as a list, or None for a device tensor whose
    values travel with the forward's one read-back; that tensor as int64 [B], or None)."""
    if torch.is_tensor(row_lengths):
        if row_lengths.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
            raise ValueError(f'row_lengths must hold integers, got {row_lengths.dtype}')
        if row_lengths.dim() != 1 or row_lengths.shape[0] != B:
            raise ValueError(f'row_lengths must have shape [{B}] (one length per sequence), got {tuple(row_lengths.shape)}')
        if row_lengths.is_cuda:
            return None, row_lengths.to(torch.int64)
        row_lengths = row_lengths.tolist()
    elif not isinstance(row_lengths, (list, tuple)):
        raise ValueError(f'row_lengths must be a [B] integer tensor or a list, got {type(row_lengths).__name__}')
    if len(row_lengths) != B:
        raise ValueError(f'row_lengths must hold one length per sequence ({B}), got {len(row_lengths)}')
    if not all(isinstance(n, int) and not isinstance(n, bool) for n in row_lengths):
        raise ValueError('row_lengths must hold integers')
    return _checked_row_lengths(row_lengths, L), None


def _checked_row_lengths(lengths, L):
    bad = [n for n in lengths if not 1 <= n <= L]
    if bad:
        raise ValueError(f'row_lengths must lie in [1, {L}] (the sequence length), got {bad[0]}')
    return [int(n) for n in lengths]


def cross_attn_rows_raw(q, kv, qrep, heads):
    """lvl_cross_attn_rows_fwd: rows q [rows, D] over the image keys | values kv [rows / qrep, Tk, 2 D] -> [rows, D]."""
    out = torch.empty_like(q)
    C.check(C.lib().lvl_cross_attn_rows_fwd(C.ptr(q), C.ptr(kv), C.ptr(out), q.shape[0], qrep, kv.shape[1], heads,
                                            C.dtype_code(q), C.stream_ptr()), 'lvl_cross_attn_rows_fwd')
    return out


class _Pack:
    """Inference image of the decoder's parameters for one compute dtype: bf16 -> every Conv1D as a contiguous [out, in]
    bf16 matrix (what lvl_linear_tn streams), the token table padded to a multiple of 256 rows (it doubles as the
    lm_head operand when tied), position table in bf16, biases / LayerNorm parameters / tanh(alpha) gates in f32.
    f32 (the parity configuration; round 5) -> every Conv1D as the bf16 TERM IMAGES [out, 3 in] of its float32 [out, in]
    matrix (ops.split3 role 1): the products run on the own MFMA kernels in f32-class mode (lvl_linear_skinny_f32c, or
    lvl_linear_tn where it tiles), ~2^-17 relative per product -- no library GEMM on the decoder's float32 path either."""

    def __init__(self, model, dtype):
        tr = model.transformer
        self.dtype = dtype
        self.key = model._param_key()
        lowp = dtype == torch.bfloat16
        f32 = lambda p: p.detach().to(torch.float32).contiguous()
        # float32: every Conv1D width is a multiple of the model width (a multiple of 64): the f32-class kernels take them all
        self.own = (not lowp) and ops.F32_MFMA and tr.embed_dim % 32 == 0

        def conv(m):      # -> (matrix, bias f32, out, in)
            w = m.weight.detach()
            if lowp:
                return (w.t().to(torch.bfloat16).contiguous(), f32(m.bias), w.shape[1], w.shape[0])
            if self.own:
                return (ops.split3(f32(w.t()), 1), f32(m.bias), w.shape[1], w.shape[0])
            return (f32(w), f32(m.bias), w.shape[1], w.shape[0])

        _lay_out(self, model, conv, ln=lambda m: (f32(m.weight), f32(m.bias)), gate=_tanh_gate)
        wte, head = tr.wte.weight.detach(), model.lm_head.weight.detach()
        tied = head.data_ptr() == wte.data_ptr()
        if lowp:
            self.wte = _pad_rows(wte.to(torch.bfloat16), 256)
            self.wpe = tr.wpe.weight.detach().to(torch.bfloat16).contiguous()
            self.head = self.wte if tied else _pad_rows(head.to(torch.bfloat16), 256)
            self.head3 = None
        else:
            self.wte, self.wpe = f32(wte), f32(tr.wpe.weight)
            self.head = self.wte if tied else f32(head)
            self.head3 = ops.split3(_pad_rows(self.head, 256), 1) if self.own else None

    # ---- primitives --------------------------------------------------------------------------------
    def _skinny(self, x2, w, b, act):
        return ops.linear_skinny_raw(x2, w, b, act)

    def gemm(self, x2, entry, act=None):
        """Conv1D (+ activation). bf16: few rows (decoding) -> lvl_linear_skinny with the activation in its epilogue;
        many rows (teacher-forced captions, the image keys / values) -> lvl_linear_tn, activation in place afterwards;
        widths neither kernel tiles -> library GEMM (logged). f32: the term images on the own kernels in f32-class mode
        (ops.linear_f32_rows); the library GEMM against the [in, out] master only with LAVILA_F32_MFMA=0."""
        w, b, n_out, n_in = entry
        rows = x2.shape[0]
        if self.dtype == torch.bfloat16:
            if rows <= SKINNY_MAX_ROWS and n_out % 16 == 0 and n_in % 32 == 0:
                return self._skinny(x2, w, b, act)
            y = ops.linear_tn_rows(x2, w, b)        # lvl_linear_tn, or lvl_linear_tn_ragged for widths in 64s (GPT-2 XL)
            if y is None:
                ops.warn_once(('conv1d', n_out, n_in), f'decoder Conv1D [{n_in}->{n_out}] on {rows} rows runs on the '
                              'library GEMM (in % 64 == 0 and out % 256 == 0, or out % 64 == 0 with both >= 256, needed)')
                y = F.linear(x2, w, b.to(torch.bfloat16))
        elif self.own:                                  # float32 decoder, term images: own kernels in f32-class mode
            return ops.linear_f32_rows(x2, w, b, act)
        else:                                           # LAVILA_F32_MFMA=0 (A/B): library GEMM against the [in, out] master
            y = torch.addmm(b, x2, w)
        return y if act is None else self.act(y, act)

    def logits(self, h2, rows=None):
        """lm_head (no bias, gpt2_gated.py:1010,1139): [rows, D] -> [rows, vocab] (a view of the padded product); of packed
        rows (`rows`: their PackedRows) -> [B, L, vocab], the padded product unpacked with zero rows behind every caption."""
        full = self._padded_logits(h2)
        if rows is None:
            return full[:, :self.vocab]
        if full.shape[1] % 8:                           # the library GEMM against an unpadded head (LAVILA_F32_MFMA=0)
            full = F.pad(full, (0, -full.shape[1] % 8))
        return rows.unpack(full, rows.L)[:, :, :self.vocab]

    def _padded_logits(self, h2):
        if self.dtype == torch.bfloat16:
            # 50432 x 768 (profiles/r03_skinny_variants.json, in-graph): up to 128 rows lvl_linear_skinny's LDS-staged tiles
            # (17 us; the 256-column-panel kernel 32), beyond that the panel kernel (72 us at 640 rows; tiles 87-120)
            if h2.shape[0] > 128 and ops._tn_ok(h2.shape[0], self.head.shape[0], self.D) and self.head.shape[0] >= 8192:
                return ops.linear_tn_raw(h2, self.head, None, C.EPI_BIAS)
            if h2.shape[0] <= SKINNY_MAX_ROWS and self.D % 32 == 0:
                return self._skinny(h2, self.head, None, None)
            if ops._tn_ok(h2.shape[0], self.head.shape[0], self.D):
                return ops.linear_tn_raw(h2, self.head, None, C.EPI_BIAS)
        elif self.head3 is not None:                    # float32: f32-class mode of the own kernels
            return ops.linear_f32_rows(h2, self.head3)
        return F.linear(h2, self.head)

    def embed(self, ids, L, pos_dev=None, rows=None):
        ids = ids.reshape(-1).contiguous()
        C.require_device(ids)
        out = torch.empty(ids.shape[0], self.D, dtype=self.dtype, device=ids.device)
        C.check(C.lib().lvl_gpt2_embed(C.ptr(ids), C.ptr(self.wte), C.ptr(self.wpe), C.ptr(pos_dev), C.ptr(out),
                                       ids.shape[0], L, self.D, self.vocab, self.positions, C.dtype_code(out),
                                       C.stream_ptr()), 'lvl_gpt2_embed')
        return out if rows is None else rows.pack(out.reshape(-1, L, self.D))

    def add_ln(self, res, y, gate, ln):
        """res <- res + gate * y (in place) -> (res, LayerNorm(res))."""
        h = torch.empty_like(res)
        C.check(C.lib().lvl_gated_add_layernorm(C.ptr(res), C.ptr(y), C.ptr(gate), C.ptr(ln[0]), C.ptr(ln[1]), self.eps,
                                                C.ptr(res) if y is not None else None, C.ptr(h), res.shape[0], self.D,
                                                C.dtype_code(res), C.stream_ptr()), 'lvl_gated_add_layernorm')
        return res, h

    def act(self, u, which):
        C.check(C.lib().lvl_act_inplace(C.ptr(u), u.numel(), which, C.dtype_code(u), C.stream_ptr()), 'lvl_act_inplace')
        return u

    def cross_attn(self, q, kv, qrep):
        if isinstance(qrep, PackedRows):
            return qrep.around(lambda rect: cross_attn_rows_raw(rect, kv, qrep.longest, self.heads), q)
        return cross_attn_rows_raw(q, kv, qrep, self.heads)

    def gemm_ln(self, x, pend, entry, act=None, fuse=True):
        """Conv1D of LayerNorm(x + gate * y) for the pending (y, gate, ln): -> (product, new residual). Few rows in bf16
        and `fuse`: ONE kernel (lvl_linear_skinny_ln: add, statistics and normalisation in the GEMM's prologue; the new
        residual goes to a fresh buffer because the other column strips still read the old one). Otherwise the fused
        add + LayerNorm kernel (residual updated in place) followed by the GEMM. Measured at 64 captions
        (profiles/r03_narrator_decode_n1.json): launched one by one the folded form is 15 % faster per token step (48
        launches fewer); inside a replayed hipGraph it is 2.5 % SLOWER (the prologue's two barriers sit on the critical
        path of every column strip, where the stand-alone kernel costs 2.5 us once) -- so graph replay keeps them apart."""
        y, gate, ln = pend
        w, b, n_out, n_in = entry
        rows = x.shape[0]
        if (fuse and self.dtype == torch.bfloat16 and rows <= FUSED_LN_MAX_ROWS and n_out % 16 == 0 and n_in % 32 == 0
                and n_in <= 1792):
            out = torch.empty(rows, n_out, dtype=torch.bfloat16, device=x.device)
            new_x = torch.empty_like(x) if y is not None else x
            C.require_device(x, y, w, b)
            C.check(C.lib().lvl_linear_skinny_ln(C.ptr(x), C.ptr(y), C.ptr(gate), C.ptr(ln[0]), C.ptr(ln[1]), self.eps,
                                                 C.ptr(new_x) if y is not None else None, C.ptr(w), C.ptr(b), C.ptr(out),
                                                 rows, n_out, n_in, -1 if act is None else act, C.stream_ptr()),
                    'lvl_linear_skinny_ln')
            return out, new_x
        x, h = self.add_ln(x, y, gate, ln)
        return self.gemm(h, entry, act), x


# ---- the plan: ONE walk over the blocks, for either primitive set (p: a _Pack, or the _TrainOps defined below) ----------
def _image_kv(p, enc):
    """crossattention.c_attn on the image tokens (gpt2_gated.py:330), once per clip and cross-attention block:
    [Bc, NQ, D] -> list of [Bc, NQ, 2D] (None for blocks without cross-attention)."""
    enc2 = enc.reshape(-1, enc.shape[-1]).to(p.dtype).contiguous()
    return [p.gemm(enc2, e['xkv']).reshape(enc.shape[0], enc.shape[1], 2 * p.D) if e['cross'] else None
            for e in p.blocks]


def _run_blocks(p, x, xkv, qrep, self_attention, fuse_ln=True):
    """The block stack on rows x [rows, D] -> LayerNorm_f of the final residual. xkv: per block image keys / values
    or None (no encoder states: plain GPT-2, gpt2_gated.py:432); qrep: the rows per clip, or the PackedRows of a forward on
    packed caption rows (handed to p.cross_attn as it is); `self_attention(i, qkv)` -> [rows, D]. Every residual
    add + LayerNorm is PENDING as (y, gate, ln) until the Conv1D that reads it (p.gemm_ln -> (product, new residual)).
    Before every primitive that has a dropout site the plan sets `p.site`: of the pending add's y, or of the attention
    probabilities -- 1 + 6 i + k in the reference's execution order (k: 0 cross-attention probabilities, 1 cross c_proj,
    2 mlp_crossattention, 3 self-attention probabilities, 4 self c_proj, 5 mlp). Only the training primitives read it."""
    with_image = xkv is not None

    def first_ln(i):
        if i == len(p.blocks):
            return p.ln_f
        e = p.blocks[i]
        return e['ln_x'] if (e['cross'] and with_image) else e['ln_1']

    def conv_of_pending(entry, act):                     # -> (Conv1D of LayerNorm(x + gate * y), new residual)
        p.site = pend_site
        return p.gemm_ln(x, pend, entry, act, fuse_ln)

    pend, pend_site = (None, None, first_ln(0)), None
    for i, e in enumerate(p.blocks):
        site = 1 + 6 * i
        if e['cross'] and with_image:
            q, x = conv_of_pending(e['xq'], None)
            p.site = site
            a = p.cross_attn(q, xkv[i], qrep)
            pend, pend_site = (p.gemm(a, e['xproj']), e['gate_c'], e['ln_2x']), site + 1
            u, x = conv_of_pending(e['xfc'], C.ACT_SQRELU)
            pend, pend_site = (p.gemm(u, e['xfproj']), e['gate_d'], e['ln_1']), site + 2
        qkv, x = conv_of_pending(e['c_attn'], None)
        a = self_attention(i, qkv)                       # its dropout site: site + 3
        pend, pend_site = (p.gemm(a, e['c_proj']), None, e['ln_2']), site + 4
        u, x = conv_of_pending(e['fc'], C.ACT_GELU_NEW)
        pend, pend_site = (p.gemm(u, e['proj']), None, first_ln(i + 1)), site + 5
    p.site = pend_site
    return p.add_ln(x, *pend)[1]                         # ln_f feeds lm_head (the 256-column-panel kernel): materialised


# --------------------------------------------------------------------------------------------------
# training (bf16): autograd Functions over the own kernels, and the primitive set (_TrainOps) that hands them to the plan
# --------------------------------------------------------------------------------------------------
class _Conv1DFn(torch.autograd.Function):
    """y = x W + b for a Conv1D weight W [in, out]: forward and input gradient on lvl_linear_tn, weight gradient on
    lvl_linear_wgrad (ops._wgrad), like ops._LinearFn. ops.weight_copies(W) yields both bf16 operands at once: the plain
    cast [in, out] is what the input-gradient GEMM reads, its transpose [out, in] what the forward reads; the pair follows
    the weight-copy discipline of ops.py (re-cast after every optimizer step and at the top of every training forward).
    A frozen weight gets no weight-gradient GEMM. Widths the kernels do not tile go to the library GEMM, logged."""

    @staticmethod
    def forward(ctx, x2, weight, bias):
        n_in, n_out = weight.shape
        rows = x2.shape[0]
        w_in_out, w_out_in = ops.weight_copies(weight)
        # forward and input gradient each pick lvl_linear_tn or lvl_linear_tn_ragged by their own shape (c_fc [1600 -> 6400]
        # tiles lvl_linear_tn forward and needs the ragged entry backward); the layer is on the own kernels when both are served
        ctx.mode = ops._route(x2, rows, n_out, n_in, ctx.needs_input_grad[0], ragged=(True, True))
        ctx.meta = (weight.dtype, bias.dtype)
        x2 = x2 if x2.is_contiguous() else x2.contiguous()
        ctx.save_for_backward(x2, w_in_out)
        if ctx.mode:
            return ops._gemm(ctx.mode, x2, w_out_in, ops._f32(bias), ragged=True)
        ops.warn_once(('conv1d', n_out, n_in), f'decoder Conv1D [{n_in}->{n_out}] on {rows} rows runs on the '
                      'library GEMM (in % 64 == 0 and out % 256 == 0, or out % 64 == 0 with both >= 256, needed)')
        with torch.autocast('cuda', enabled=False):
            return F.linear(x2, w_out_in, bias.detach().to(torch.bfloat16))

    @staticmethod
    def backward(ctx, dy):
        x2, w_in_out = ctx.saved_tensors
        wdt, bdt = ctx.meta
        dy = dy if dy.is_contiguous() else dy.contiguous()
        with torch.autocast('cuda', enabled=False):      # swap: dw = x^T dy, [in, out], the Conv1D layout
            return ops._linear_backward(ctx.needs_input_grad, dy, x2, w_in_out, ctx.mode, wdt, bdt, ragged=True, swap=True)


class _GatedAddLnFn(torch.autograd.Function):
    """s = res + tanh(alpha) * y, h = LayerNorm(s): (s, h) -- or h alone when there is no y (the first norm of the stack).
    Forward lvl_gated_add_layernorm_train (the inference kernel, which also returns mean / rstd), backward
    lvl_gated_add_layernorm_bwd: lvl_layernorm_bwd on the kept sum with the residual stream's gradient as `dadd`, then one
    pass for dy = gate * ds and the deterministic gate gradient.
    drop = (seed, site, p): dropout on y, s = res + (keep ? tanh(alpha) / (1 - p) : 0) * y, through
    lvl_gated_add_layernorm_train_drop / _bwd_drop; the backward regenerates the mask from ctx.drop."""

    @staticmethod
    def forward(ctx, res, y, alpha, gamma, beta, eps, drop=None):
        res = res if res.is_contiguous() else res.contiguous()
        g, b = ops._f32(gamma), ops._f32(beta)
        gate = _tanh_gate(alpha)
        if y is not None:
            y = y if y.is_contiguous() else y.contiguous()
        s, h, mean, rstd = ops.add_ln_fwd_raw(res, y, gate, g, b, eps, drop)
        ctx.save_for_backward(res if s is None else s, y if gate is not None else None, gate, g, mean, rstd)
        ctx.meta = (y is not None, None if alpha is None else alpha.dtype, gamma.dtype, beta.dtype)
        ctx.drop = drop
        return h if s is None else (s, h)

    @staticmethod
    def backward(ctx, *grads):
        s, y, gate, g, mean, rstd = ctx.saved_tensors
        has_y, adt, gdt, bdt = ctx.meta
        dadd, dh = (grads if has_y else (None, grads[0]))
        if dh is None:
            dh = torch.zeros_like(s)
        dh = dh if dh.is_contiguous() else dh.contiguous()
        if dadd is not None and not dadd.is_contiguous():
            dadd = dadd.contiguous()
        ds, dy, dgamma, dbeta, dgate = ops.add_ln_bwd_raw(dh, s, y, gate, g, mean, rstd, dadd, ctx.drop)
        dalpha = None
        if gate is not None:
            dalpha = (dgate * (1.0 - gate * gate)).reshape(()).to(adt)
        # an ungated add without dropout has no dy of its own: it is ds
        return ds, ((ds if dy is None else dy) if has_y else None), dalpha, dgamma.to(gdt), dbeta.to(bdt), None, None


class _ActFn(torch.autograd.Function):
    """a = gelu_new(u) / relu(u)^2 out of place (lvl_act_fwd; u is kept), du = da * act'(u) (lvl_act_bwd)."""

    @staticmethod
    def forward(ctx, u, which):
        u = u if u.is_contiguous() else u.contiguous()
        a = torch.empty_like(u)
        C.check(C.lib().lvl_act_fwd(C.ptr(u), C.ptr(a), u.numel(), which, C.dtype_code(u), C.stream_ptr()), 'lvl_act_fwd')
        ctx.save_for_backward(u)
        ctx.which = which
        return a

    @staticmethod
    def backward(ctx, da):
        u, = ctx.saved_tensors
        da = da if da.is_contiguous() else da.contiguous()
        du = torch.empty_like(u)
        C.check(C.lib().lvl_act_bwd(C.ptr(u), C.ptr(da), C.ptr(du), u.numel(), ctx.which, C.dtype_code(u), C.stream_ptr()),
                'lvl_act_bwd')
        return du, None


CROSS_ATTN_BWD_MAX_KEYS = 256


class _DropoutFn(torch.autograd.Function):
    """out = keep ? x / (1 - p) : 0 (lvl_dropout_apply; the embedding site); the backward is the same call on the gradient."""

    @staticmethod
    def _apply(x, drop):
        seed, site, p = drop
        x = x if x.is_contiguous() else x.contiguous()
        out = torch.empty_like(x)
        C.require_device(x)
        C.check(C.lib().lvl_dropout_apply(C.ptr(x), C.ptr(out), x.numel(), seed, site, p, C.dtype_code(x), C.stream_ptr()),
                'lvl_dropout_apply')
        return out

    @staticmethod
    def forward(ctx, x, seed, site, p):
        ctx.drop = (seed, site, p)
        return _DropoutFn._apply(x, ctx.drop)

    @staticmethod
    def backward(ctx, dout):
        return _DropoutFn._apply(dout, ctx.drop), None, None, None


def _off_ptr(t, elements):
    return C._c.c_void_p(t.data_ptr() + elements * t.element_size())


class _RowsAttnFn(torch.autograd.Function):
    """The decoder's rows attention. kv given: the cross-attention, q [rows, D] over kv [rows / qrep, Tk, 2 D]. kv None: the
    causal self-attention on q = qkv [B L, 3 D] with qrep = L positions per caption (keys and values are its own thirds;
    the gradient comes back as dqkv); built only with dropout.
    drop None: lvl_cross_attn_rows_fwd / _bwd. drop = (seed, site, p): dropout on the attention probabilities,
    lvl_attn_rows_drop_fwd / _bwd on the same operands as strides."""

    @staticmethod
    def _layout(q, kv, qrep, heads):
        D = heads * 64
        if kv is None:         # (k, v, contexts, Tk, q stride, kv row stride, kv context stride, causal)
            return _off_ptr(q, D), _off_ptr(q, 2 * D), q.shape[0] // qrep, qrep, 3 * D, 3 * D, qrep * 3 * D, 1
        return C.ptr(kv), _off_ptr(kv, D), kv.shape[0], kv.shape[1], D, 2 * D, kv.shape[1] * 2 * D, 0

    @staticmethod
    def forward(ctx, q, kv, qrep, heads, drop=None):
        keys = qrep if kv is None else kv.shape[1]
        if drop is None:
            if kv is None:
                raise C.HipExtensionError('decoder rows attention: the causal form (kv None) is built with dropout only')
            if q.dtype != torch.bfloat16 or keys > CROSS_ATTN_BWD_MAX_KEYS:
                raise C.HipExtensionError(f'decoder cross-attention backward is built for bf16 and at most '
                                          f'{CROSS_ATTN_BWD_MAX_KEYS} image tokens per clip (got {q.dtype}, {keys})')
        elif q.dtype != torch.bfloat16 or keys > ATTN_DROP_MAX_KEYS:
            raise C.HipExtensionError(f'decoder attention with attn_pdrop > 0 is built for bf16 and at most '
                                      f'{ATTN_DROP_MAX_KEYS} keys (caption positions / image tokens per clip); got '
                                      f'{q.dtype}, {keys}')
        q = q if q.is_contiguous() else q.contiguous()
        if kv is not None:
            kv = kv if kv.is_contiguous() else kv.contiguous()
        C.require_device(q, kv)
        if drop is None:
            out = cross_attn_rows_raw(q, kv, qrep, heads)
        else:
            k, v, contexts, Tk, qs, kvs, kvc, causal = _RowsAttnFn._layout(q, kv, qrep, heads)
            out = torch.empty(q.shape[0], heads * 64, dtype=q.dtype, device=q.device)
            C.check(C.lib().lvl_attn_rows_drop_fwd(C.ptr(q), k, v, C.ptr(out), contexts, qrep, Tk, heads, qs, kvs, kvc, causal,
                                                   *drop, C.dtype_code(q), C.stream_ptr()), 'lvl_attn_rows_drop_fwd')
        ctx.save_for_backward(q, kv)
        ctx.cfg = (qrep, heads, drop)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, kv = ctx.saved_tensors
        qrep, heads, drop = ctx.cfg
        D = heads * 64
        dout = dout if dout.is_contiguous() else dout.contiguous()
        dq = torch.empty_like(q)
        dkv = torch.empty_like(kv) if kv is not None else None
        if drop is None:
            C.check(C.lib().lvl_cross_attn_rows_bwd(C.ptr(q), C.ptr(kv), C.ptr(dout), C.ptr(dq), C.ptr(dkv), q.shape[0], qrep,
                                                    kv.shape[1], heads, C.dtype_code(q), C.stream_ptr()),
                    'lvl_cross_attn_rows_bwd')
        else:
            k, v, contexts, Tk, qs, kvs, kvc, causal = _RowsAttnFn._layout(q, kv, qrep, heads)
            dk, dv = (_off_ptr(dq, D), _off_ptr(dq, 2 * D)) if kv is None else (C.ptr(dkv), _off_ptr(dkv, D))
            C.check(C.lib().lvl_attn_rows_drop_bwd(C.ptr(q), k, v, C.ptr(dout), C.ptr(dq), dk, dv, contexts, qrep, Tk, heads,
                                                   qs, kvs, kvc, causal, *drop, C.dtype_code(q), C.stream_ptr()),
                    'lvl_attn_rows_drop_bwd')
        return dq, dkv, None, None, None


class _LmHeadFn(torch.autograd.Function):
    """logits = h W^T for the (tied) lm_head weight W [vocab, D]: the vocabulary is padded with zero rows to the GEMM's
    256-column tiles (as the inference image is), the padded bf16 image and its transpose are cast per forward from the
    current parameter (nothing cached, nothing stale) and the padded columns are dropped again. dW [vocab, D] comes back as
    a gradient of the weight: tied, autograd adds it to the embedding's. `padded`: the whole padded product is the result
    (what a forward on packed rows unpacks; its gradient arrives in that shape too)."""

    @staticmethod
    def forward(ctx, h2, weight, padded=False):
        V, D = weight.shape
        rows = h2.shape[0]
        w = _pad_rows(weight.detach().to(torch.bfloat16), 256)
        Vp = w.shape[0]
        ctx.mode = ops._route(h2, rows, Vp, D, ragged=(False, True))            # the input gradient has N = D: ragged at 1600
        h2 = h2 if h2.is_contiguous() else h2.contiguous()
        ctx.save_for_backward(h2, w)
        ctx.meta = (V, weight.dtype, padded)
        if ctx.mode:
            full = ops._gemm(ctx.mode, h2, w)
        else:
            ops.warn_once(('lm_head', V, D), f'decoder lm_head [{D}->{V}] on {rows} rows runs on the library GEMM')
            with torch.autocast('cuda', enabled=False):
                full = F.linear(h2, w)
        return full if padded else full[:, :V]

    @staticmethod
    def backward(ctx, dlogits):
        h2, w = ctx.saved_tensors
        V, wdt, padded = ctx.meta
        if padded:
            dl = dlogits.to(torch.bfloat16).contiguous()
        else:
            dl = torch.zeros(h2.shape[0], w.shape[0], dtype=torch.bfloat16, device=h2.device)
            dl[:, :V] = dlogits
        need = ctx.needs_input_grad
        with torch.autocast('cuda', enabled=False):
            wt = w.t().contiguous() if (ctx.mode and need[0]) else w.t()
            dh, dw, _ = ops._linear_backward(need[:2], dl, h2, wt, ctx.mode, wdt, ragged=True)
        return dh, None if dw is None else dw[:V], None


class _TrainOps:
    """The plan's primitives as the autograd Functions above (rows in bf16). A Conv1D / LayerNorm role is the module itself,
    a gate the alpha parameter (_GatedAddLnFn takes and differentiates its tanh). Nothing is cached: built per forward.
    `pdrop` = (resid, embd, attn) probabilities this forward applies (all 0: exactly the plan without dropout); with any
    of them set, ONE seed is drawn here and travels in each Function's ctx."""
    dtype = torch.bfloat16

    def __init__(self, model, pdrop=(0.0, 0.0, 0.0)):
        _lay_out(self, model, conv=lambda m: m, ln=lambda m: m, gate=lambda alpha: alpha)
        self.wte, self.wpe, self.head = model.transformer.wte.weight, model.transformer.wpe.weight, model.lm_head.weight
        self.p_resid, self.p_embd, self.p_attn = (float(v) for v in pdrop)
        self.seed = _draw_seed() if any(pdrop) else 0
        self.site = None                              # set by the plan before every primitive that has a dropout site

    def embed(self, ids, L, rows=None):
        x = ops.text_embed(ids, self.wte, self.wpe, self.dtype)
        if x is None:                                 # tables the gather kernel does not take (bf16 parameters, width > 2048)
            x = (F.embedding(ids, self.wte) + self.wpe[:L]).to(self.dtype)
        # packed rows: the embedding dropout site then indexes the PACKED rows (element = packed row * D + column)
        x = x.reshape(-1, self.D) if rows is None else rows.pack(x.reshape(-1, L, self.D))
        return _DropoutFn.apply(x, self.seed, 0, self.p_embd) if self.p_embd else x

    def self_attn(self, i, qkv, L):
        """The causal self-attention of block i on qkv [B L, 3D]: ops.causal_attention, or with attn_pdrop the rows kernel."""
        if self.p_attn:
            return _RowsAttnFn.apply(qkv, None, L, self.heads, (self.seed, 1 + 6 * i + 3, self.p_attn))
        return ops.causal_attention(qkv.reshape(-1, L, 3 * self.D), self.heads).reshape(-1, self.D)

    def gemm(self, x2, m, act=None):
        y = _Conv1DFn.apply(x2, m.weight, m.bias)
        return y if act is None else _ActFn.apply(y, act)

    def add_ln(self, res, y, alpha, ln):
        if y is not None and self.p_resid:
            return _GatedAddLnFn.apply(res, y, alpha, ln.weight, ln.bias, self.eps, (self.seed, self.site, self.p_resid))
        out = _GatedAddLnFn.apply(res, y, alpha, ln.weight, ln.bias, self.eps)
        return out if y is not None else (res, out)

    def gemm_ln(self, x, pend, m, act=None, fuse=True):
        x, h = self.add_ln(x, *pend)
        return self.gemm(h, m, act), x

    def cross_attn(self, q, kv, qrep):
        if isinstance(qrep, PackedRows):              # the rectangle's (ctx, h, i, j) index serves the dropout site
            return qrep.around(lambda rect: self.cross_attn(rect, kv, qrep.longest), q)
        if self.p_attn:
            return _RowsAttnFn.apply(q, kv, qrep, self.heads, (self.seed, self.site, self.p_attn))
        return _RowsAttnFn.apply(q, kv, qrep, self.heads)

    def logits(self, h2, rows=None):
        if rows is None:
            return _LmHeadFn.apply(h2, self.head)
        return rows.unpack(_LmHeadFn.apply(h2, self.head, True), rows.L)[:, :, :self.vocab]


class DecodeSession:
    """Key/value-cached decoding of `rows = contexts * seqs_per_context` captions, one token per step.
    step(ids [rows]) -> logits [rows, vocab] of the NEXT token (a view of a buffer that the next step overwrites).
    With graph=True the step is captured once into a hipGraph (position, ids and logits live in fixed device buffers)
    and replayed; the session is bound to the parameter values it was built from (`stale()` tells)."""

    def __init__(self, model, pack, image_tokens, max_length, seqs_per_context=1, graph=True):
        self.model, self.pack = model, pack
        dev = image_tokens.device
        Bc = image_tokens.shape[0]
        self.rows, self.qrep, self.capacity = Bc * seqs_per_context, seqs_per_context, int(max_length)
        if self.capacity > pack.positions:
            raise ValueError(f'decode length {self.capacity} exceeds the decoder\'s {pack.positions} positions')
        self.contexts, self.context_len = Bc, image_tokens.shape[1]
        self.xkv = _image_kv(pack, image_tokens)
        self.cache = [torch.zeros(self.rows, self.capacity, 2 * pack.D, dtype=pack.dtype, device=dev) for _ in pack.blocks]
        self.pos = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ids = torch.zeros(self.rows, dtype=torch.int64, device=dev)
        self.steps = 0
        self._logits = None
        self._graph = None
        self.graphed = bool(graph)
        if graph:
            self._capture()

    def stale(self):
        return self.pack.key != self.model._param_key()

    def _self_attention(self, i, qkv):
        out = torch.empty(self.rows, self.pack.D, dtype=qkv.dtype, device=qkv.device)
        C.check(C.lib().lvl_decode_self_attn(C.ptr(qkv), C.ptr(self.cache[i]), C.ptr(self.pos), C.ptr(out), self.rows,
                                             self.capacity, self.pack.heads, C.dtype_code(qkv), C.stream_ptr()),
                'lvl_decode_self_attn')
        return out

    def _run(self):
        p = self.pack
        x = p.embed(self.ids, 1, self.pos)
        h = _run_blocks(p, x, self.xkv, self.qrep, self._self_attention, fuse_ln=not self.graphed)
        logits = p.logits(h)
        self.pos.add_(1)
        return logits

    def _capture(self):
        """One eager step on a side stream (lazy kernel attributes, allocator warm-up), then the capture. A capture that
        fails (e.g. another thread launching on the device meanwhile) leaves the session on eager launches, loudly."""
        try:
            self._capture_step()
        except RuntimeError as e:                        # hipGraph errors surface as RuntimeError from torch
            import warnings
            warnings.warn(f'DecodeSession: hipGraph capture failed ({e}); decoding with eager launches')
            self._graph, self._logits, self.graphed = None, None, False
            torch.cuda.synchronize()
            self.pos.zero_()

    def _capture_step(self):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):           # first launch outside the capture: lazy kernel attributes, allocator warm-up
            self._run()
            self.pos.zero_()
        torch.cuda.current_stream().wait_stream(side)
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph):
            self._logits = self._run()
        self.pos.zero_()

    def reset(self):
        self.pos.zero_()
        self.steps = 0

    def rebind(self, image_tokens):
        """Start over on other clips of the same shape: their keys / values are projected INTO the buffers the captured
        graph reads, the position returns to 0 (cache rows are rewritten before they are read)."""
        if tuple(image_tokens.shape[:2]) != (self.contexts, self.context_len):
            raise ValueError('DecodeSession.rebind: image tokens of another shape need another session')
        for dst, src in zip(self.xkv, _image_kv(self.pack, image_tokens)):
            if dst is not None:
                dst.copy_(src)
        self.reset()
        return self

    def reorder(self, index):
        """Beam search: row r continues the caption that row index[r] held (narrator.py:223,337: `input_ids[beam_idx]`;
        the reference re-runs the prefixes, here the cached keys / values move with their captions). Only the filled
        positions are gathered; rows of one clip stay inside that clip, so the image keys / values are untouched."""
        n = self.steps
        if n == 0:
            return
        for c in self.cache:
            c[:, :n] = c[:, :n].index_select(0, index)

    def step(self, ids):
        if self.steps >= self.capacity:
            raise RuntimeError(f'DecodeSession: cache of {self.capacity} positions is full')
        self.ids.copy_(ids.reshape(-1))
        self.steps += 1
        if self._graph is not None:
            self._graph.replay()
            return self._logits
        return self._run()


class GPT2LMHeadModel(nn.Module):
    """gpt2_gated.py:1004-1162 (the language-model head on GPT2Model). `forward` takes the reference's
    keyword names; everything but input_ids / encoder_hidden_states / labels must be left at None."""

    def __init__(self, config):
        super().__init__()
        if _cfg(config, 'activation_function', 'gelu_new') != 'gelu_new':
            raise NotImplementedError('only GPT-2\'s gelu_new activation is built')
        if _cfg(config, 'scale_attn_by_inverse_layer_idx', False) or _cfg(config, 'reorder_and_upcast_attn', False) or \
                not _cfg(config, 'scale_attn_weights', True):
            raise NotImplementedError('attention variants other than GPT-2\'s 1/sqrt(d) scaling are not built')
        D, H = _cfg(config, 'n_embd'), _cfg(config, 'n_head')
        if D != H * 64:
            raise NotImplementedError(f'lavila_amd attention kernels are built for head_dim 64, got {D}/{H}')
        self.config = config
        self.transformer = GPT2Model(config)
        self.lm_head = nn.Linear(D, _cfg(config, 'vocab_size'), bias=False)
        if _cfg(config, 'tie_word_embeddings', True):
            self.lm_head.weight = self.transformer.wte.weight
        self._packs = {}
        self._sessions = {}

    def __getstate__(self):
        """The packed weights and decode sessions (device buffers, captured graphs) are caches of the parameters: they
        are rebuilt on demand and never copied or pickled with the module (copy.deepcopy, torch.save(model))."""
        state = self.__dict__.copy()
        state['_packs'], state['_sessions'] = {}, {}
        return state

    # ---- reference API ---------------------------------------------------------------------------------
    def freeze_lm_weights(self):
        """gpt2_gated.py:1019-1030."""
        for n, p in self.named_parameters():
            p.requires_grad = ('crossattention' in n or 'cross_attn' in n or 'alpha_cattn' in n or 'alpha_dense' in n)

    def gradient_checkpointing_enable(self):
        pass                                    # a no-op: the training plan keeps its activations

    def gradient_checkpointing_disable(self):
        pass

    def get_output_embeddings(self):
        return self.lm_head

    def _param_key(self):
        """What the packed inference image was built from: the decoder's OWN parameters (version counter + storage) and a
        decoder-local generation. (Round 3 keyed on the process-wide weight-copy generation of ops.py, which every
        optimizer step and every grad-enabled model forward anywhere in the process bumps: a 1.5-B-parameter repack and a
        hipGraph recapture per batch for nothing -- ADVICE r3.) Writes that bypass the version counter (`param.data`
        edits, a fused optimizer stepping the decoder) need `invalidate_packed_weights()`."""
        return (getattr(self, '_pack_gen', 0),) + tuple((p._version, p.data_ptr()) for p in self.parameters())

    def invalidate_packed_weights(self):
        """Forget the packed bf16 image and the decode sessions built on it (they are rebuilt on the next call)."""
        self._pack_gen = getattr(self, '_pack_gen', 0) + 1
        self._packs, self._sessions = {}, {}

    clear_sessions = invalidate_packed_weights

    def _compute_dtype(self):
        lp = ops.autocast_dtype()
        if lp is not None:
            return lp
        dt = self.transformer.wte.weight.dtype
        return torch.bfloat16 if dt == torch.float16 else dt

    def _pack(self, dtype=None):
        dtype = dtype or self._compute_dtype()
        if dtype not in (torch.float32, torch.bfloat16):
            raise C.HipExtensionError(f'the decoder computes in float32 or bfloat16, not {dtype}')
        pack = self._packs.get(dtype)
        if pack is None or pack.key != self._param_key():
            if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
                raise NotImplementedError('the packed inference image of lavila_amd.gpt2_gated (decoding, float32) has no '
                                          'backward: call it under torch.no_grad()')
            C.require_device(self.transformer.wte.weight)
            with torch.no_grad(), torch.autocast('cuda', enabled=False):
                pack = self._packs[dtype] = _Pack(self, dtype)
        return pack

    def forward(self, input_ids=None, past_key_values=None, attention_mask=None, token_type_ids=None, position_ids=None,
                head_mask=None, inputs_embeds=None, encoder_hidden_states=None, encoder_attention_mask=None, labels=None,
                use_cache=None, output_attentions=None, output_hidden_states=None, return_dict=None, row_lengths=None):
        """`row_lengths` ([B] integers on the device or the host, or a list; 1 <= len_b <= L): only the first len_b positions
        of sequence b run through the decoder, as packed rows (PackedRows); `.logits` keeps its shape, with exact zeros at
        and behind position len_b. Exact for what a causal decoder computes at the kept positions; it is not
        `attention_mask`, which stays refused."""
        unsupported = dict(past_key_values=past_key_values, attention_mask=attention_mask, token_type_ids=token_type_ids,
                           position_ids=position_ids, head_mask=head_mask, inputs_embeds=inputs_embeds,
                           encoder_attention_mask=encoder_attention_mask)
        bad = [k for k, v in unsupported.items() if v is not None]
        if bad or use_cache or output_attentions or output_hidden_states or return_dict is False:
            raise NotImplementedError(f'GPT2LMHeadModel.forward: {bad or "use_cache / output_* / return_dict=False"} is '
                                      'not on the narrator path (cached decoding: decode_session())')
        if input_ids is None:
            raise ValueError('You have to specify input_ids')
        shape = tuple(input_ids.shape)
        L = shape[-1]
        lengths = lengths_dev = None
        if row_lengths is not None:
            lengths, lengths_dev = _row_lengths_on_host(row_lengths, input_ids.numel() // max(L, 1), L)
        train = self._trains(encoder_hidden_states)
        p = self._train_ops() if train else self._pack()
        if L > p.positions:
            raise ValueError(f'sequence of {L} tokens exceeds the decoder\'s {p.positions} positions')
        ids = input_ids.reshape(-1, L).contiguous()
        B = ids.shape[0]
        if lengths_dev is None:
            lo, hi = (int(v) for v in torch.stack(torch.aminmax(ids)).tolist())  # ONE read-back; the gather kernels clamp
        else:                                                                    # ... in which device lengths travel along
            C.require_device(ids, lengths_dev)
            lo, hi, *lengths = torch.cat([torch.stack(torch.aminmax(ids)), lengths_dev]).tolist()
            lengths = _checked_row_lengths(lengths, L)
        if lo < 0 or hi >= p.vocab:
            raise IndexError(f'input_ids out of range [0, {p.vocab}): min {lo}, max {hi}')
        rows = None if lengths is None else PackedRows(lengths, L, ids.device)
        enc = encoder_hidden_states
        if enc is not None:
            enc = ops.lowp(enc)
            if enc.shape[0] != B or enc.shape[-1] != p.D:
                raise ValueError(f'encoder_hidden_states {tuple(enc.shape)} does not match {B} sequences of width {p.D}')
        with (ops.model_forward() if train else torch.no_grad()), torch.autocast('cuda', enabled=False):
            xkv = qrep = None
            if enc is not None and any(e['cross'] for e in p.blocks):
                xkv, qrep = _image_kv(p, enc), L

            def self_attention(i, qkv, L=L):
                if train:
                    return p.self_attn(i, qkv, L)
                return ops.causal_attention(qkv.reshape(B, L, 3 * p.D), p.heads).reshape(B * L, p.D)
            if rows is None:
                h = _run_blocks(p, p.embed(ids, L), xkv, qrep, self_attention)
                logits = p.logits(h).reshape(*shape, p.vocab)
            else:       # the plan on the kept rows; each attention on the zero-filled rectangle [B, longest caption]
                def packed_self_attention(i, qkv):
                    return rows.around(lambda rect: self_attention(i, rect, rows.longest), qkv)
                h = _run_blocks(p, p.embed(ids, L, rows=rows), xkv, rows if xkv is not None else None, packed_self_attention)
                logits = p.logits(h, rows).reshape(*shape, p.vocab)
            loss = None
            if labels is not None:                              # gpt2_gated.py:1142-1148
                loss = F.cross_entropy(logits[..., :-1, :].reshape(-1, p.vocab).float(), labels[..., 1:].reshape(-1))
        if not train and self.transformer.wte.weight.dtype == torch.float16 and not torch.is_autocast_enabled():
            logits = logits.to(torch.float16)
        return CausalLMOutput(logits, loss)

    def _trains(self, encoder_hidden_states):
        """The training primitives run when gradients are enabled and a decoder parameter or the image tokens require one
        (the latter: freeze_lm_weights() on everything with a trainable pooler in front)."""
        return torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters()) or
                                            (encoder_hidden_states is not None and encoder_hidden_states.requires_grad))

    def _train_ops(self):
        """The training primitive set, after the refusals of what it does not do (raised before any device work)."""
        if self._compute_dtype() != torch.bfloat16:
            raise NotImplementedError('lavila_amd.gpt2_gated trains in bf16 (bf16 parameters, or float32 masters under '
                                      'torch.autocast(\'cuda\', dtype=torch.bfloat16)); there is no float32 backward for the '
                                      'decoder: call it under torch.no_grad()')
        names = ('resid_pdrop', 'embd_pdrop', 'attn_pdrop')
        drop = [k for k in names if _cfg(self.config, k, 0.0)]
        pdrop = (0.0, 0.0, 0.0)
        if drop and self.training:
            if not decoder_dropout_enabled():
                raise NotImplementedError(f'the decoder has no dropout: config.{" / ".join(drop)} must be 0.0 to train it '
                                          '(transformers\' GPT2Config defaults them to 0.1), or call .eval(). The dropout '
                                          'kernels are opt-in: LAVILA_DECODER_DROPOUT=1 or gpt2_gated.DECODER_DROPOUT = True')
            pdrop = tuple(float(_cfg(self.config, k, 0.0)) for k in names)
            if not all(0.0 <= v < 1.0 for v in pdrop):
                raise ValueError(f'config.{" / ".join(names)} = {pdrop} must lie in [0, 1)')
        C.require_device(self.transformer.wte.weight)
        return _TrainOps(self, pdrop)

    def applies_dropout(self):
        """Whether a training forward of this decoder would drop now (switch on, training mode, a non-zero probability)."""
        return bool(self.training and decoder_dropout_enabled() and
                    any(_cfg(self.config, k, 0.0) for k in ('resid_pdrop', 'embd_pdrop', 'attn_pdrop')))

    def decode_session(self, encoder_hidden_states, max_length, seqs_per_context=1, graph=True):
        """Cached decoding against `encoder_hidden_states` [contexts, NQ, D]; see DecodeSession. The last sessions are
        kept (buffers + captured graph) and re-bound when the next batch has the same shape -- the captioning drivers
        call generate() once per batch (main_infer_narrator.py:178-188) -- as long as the parameters have not changed."""
        pack = self._pack()
        enc = ops.lowp(encoder_hidden_states)
        key = (tuple(enc.shape), str(enc.device), int(max_length), int(seqs_per_context), bool(graph), pack.dtype)
        with torch.no_grad(), torch.autocast('cuda', enabled=False):
            sess = self._sessions.get(key)
            if sess is not None and sess.pack is pack:
                return sess.rebind(enc)
            # keep two: drop the older ones BEFORE the new session's buffers are allocated
            self._sessions = {k: v for k, v in list(self._sessions.items())[-1:] if v.pack is pack}
            sess = DecodeSession(self, pack, enc, max_length, seqs_per_context, graph)
            self._sessions[key] = sess
            return sess
