"""Restatement of the DistilBERT text tower's dropout (the mask contract of include/lavila_hip.h), written from the
specification and not from the kernel source: the masks in numpy on top of tests/dropout_reference.py (Philox4x32-10,
threshold and float32 scale are the decoder's), and the tower of tests/distilbert_reference.py in float64 with those masks.

transformers' modeling_distilbert.py calls dropout 1 + 2 n_layers times per forward, in this order:
    site 0          the embedding behind embeddings.LayerNorm                                  [B, L, D]   (dropout)
    site 1 + 2 n    layer n, the attention probabilities behind the masked softmax           [B, H, L, L]   (attention_dropout)
    site 2 + 2 n    layer n, the output of ffn.lin2 with its bias, before + sa_output        [B, L, D]   (dropout)

Row sites:        e = (b L + i) D + c, L = the positions the tower runs on (after the trim).
Attention sites:  e = ((((b H + h) L + i) << s) | j for query i and key j; s = 8 up to 256 keys, else the smallest s with
                  2^s >= Tk.
A call on a subset of rows addresses the elements of the full call: row r of a row call has e = r * row_index_stride + c
(D for all rows, L D for row 0 of every sample); query i of context b of an attention call is row b * idx_qrep + i of the
index (idx_qrep = L when the call holds one query per sample).

P is the softmax over the visible keys (all keys: the uniform distribution of a sample without a visible key), then
Pd = keep ? scale P : 0 and O = Pd V; autograd gives dP = keep ? scale (dO V^T) : 0, dS = P (dP - sum_j P dP)."""
import numpy as np
import torch

import distilbert_reference as R
import dropout_reference as DR

MASK32 = np.uint64(0xFFFFFFFF)


def site_embedding():
    return 0


def site_attention(layer):
    return 1 + 2 * layer


def site_ffn(layer):
    return 2 + 2 * layer


def attn_shift(Tk):
    s = 8
    while (1 << s) < Tk:
        s += 1
    return s


def keep_at(seed, site, e, p):
    """bool array of the shape of e: keep of the elements with the (arbitrary, uint64) indices e."""
    e = np.asarray(e, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    g = e >> np.uint64(2)
    zero = np.zeros_like(g)
    w = DR.philox4x32_10((g & MASK32, g >> np.uint64(32), zero + np.uint64(site), zero), (seed & 0xFFFFFFFF, seed >> 32))
    r = (e & np.uint64(3)).astype(np.int64)
    word = np.choose(r, w)
    return word >= np.uint64(DR.threshold(p))


def row_keep(seed, site, rows, D, p, row_index_stride=None):
    """bool [rows, D]: the rows of a row call, row_index_stride elements apart in the index (default D: all rows)."""
    stride = D if row_index_stride is None else row_index_stride
    e = np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(stride) + np.arange(D, dtype=np.uint64)[None, :]
    return keep_at(seed, site, e, p)


def attn_keep(seed, site, contexts, H, qrep, Tk, p, idx_qrep=None):
    """bool [contexts, H, qrep, Tk]: the queries 0 .. qrep - 1 of every context, idx_qrep query rows per context in the
    index (default qrep: the full call)."""
    L = qrep if idx_qrep is None else idx_qrep
    assert L >= qrep
    s = np.uint64(attn_shift(Tk))
    b = np.arange(contexts, dtype=np.uint64)[:, None, None, None]
    h = np.arange(H, dtype=np.uint64)[None, :, None, None]
    i = np.arange(qrep, dtype=np.uint64)[None, None, :, None]
    j = np.arange(Tk, dtype=np.uint64)[None, None, None, :]
    e = ((((b * np.uint64(H) + h) * np.uint64(L)) + i) << s) | j
    return keep_at(seed, site, e, p)


def _t(keep, like):
    return torch.from_numpy(np.ascontiguousarray(keep)).to(like.dtype)


def keymask_attention_drop(q, k, v, mask, heads, keep, scale):
    """R.keymask_attention with Pd = keep * scale * P; keep bool [B, H, Lq, Lk] (numpy or torch)."""
    B, Lq, D = q.shape
    qh, kh, vh = (t.reshape(B, -1, heads, 64).permute(0, 2, 1, 3) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / 8.0
    if mask is not None:
        s = s.masked_fill((mask == 0)[:, None, None, :], torch.finfo(s.dtype).min)
    keep = keep if torch.is_tensor(keep) else _t(keep, s)
    pd = torch.softmax(s, -1) * (keep.to(s.dtype) * scale)
    return (pd @ vh).permute(0, 2, 1, 3).reshape(B, Lq, D)


def block(x, mask, w, p, heads, layer, seed, p_drop, p_attn):
    B, L, D = x.shape
    a = p + 'attention.'
    keep = attn_keep(seed, site_attention(layer), B, heads, L, L, p_attn)
    o = keymask_attention_drop(R._lin(x, w, a + 'q_lin'), R._lin(x, w, a + 'k_lin'), R._lin(x, w, a + 'v_lin'), mask, heads,
                               keep, float(DR.scale(p_attn)))
    h = R.layer_norm(R._lin(o, w, a + 'out_lin') + x, w[p + 'sa_layer_norm.weight'], w[p + 'sa_layer_norm.bias'])
    f = R._lin(R.gelu_erf(R._lin(h, w, p + 'ffn.lin1')), w, p + 'ffn.lin2')
    f = f * (_t(row_keep(seed, site_ffn(layer), B * L, D, p_drop).reshape(B, L, D), f) * float(DR.scale(p_drop)))
    return R.layer_norm(f + h, w[p + 'output_layer_norm.weight'], w[p + 'output_layer_norm.bias'])


def tower(ids, mask, w, heads, seed, p_drop, p_attn, prefix=''):
    """R.tower in train mode under the masks of `seed`: last_hidden_state [B, L, D]. p_drop = p_attn = 0 is R.tower, bit for
    bit (every factor is exactly 1)."""
    p = prefix
    B, L = ids.shape
    x = w[p + 'embeddings.word_embeddings.weight'][ids] + w[p + 'embeddings.position_embeddings.weight'][:L]
    x = R.layer_norm(x, w[p + 'embeddings.LayerNorm.weight'], w[p + 'embeddings.LayerNorm.bias'])
    D = x.shape[-1]
    x = x * (_t(row_keep(seed, site_embedding(), B * L, D, p_drop).reshape(B, L, D), x) * float(DR.scale(p_drop)))
    layers = 1 + max(int(k[len(p) + 18:].split('.')[0]) for k in w if k.startswith(p + 'transformer.layer.'))
    for i in range(layers):
        x = block(x, mask, w, f'{p}transformer.layer.{i}.', heads, i, seed, p_drop, p_attn)
    return x


def clip_hf_forward(video, ids, mask, w, vision_heads, text_heads, seed, p_drop, p_attn, norm_embed=False):
    """R.clip_hf_forward with the text tower under dropout (the video tower has none)."""
    from oracle import oracle as O
    img = O.vision_tower(video, w, vision_heads) @ w['image_projection']
    txt = tower(ids, mask, w, text_heads, seed, p_drop, p_attn, 'textual.')[:, 0] @ w['text_projection']
    if norm_embed:
        img, txt = O.l2_normalize(img), O.l2_normalize(txt)
    return {'image_embed': img, 'text_embed': txt, 'logit_scale': w['logit_scale'].exp()}
