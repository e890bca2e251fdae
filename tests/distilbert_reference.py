"""Float64 restatement of DistilBERT as CLIP_HF uses it (reference lavila/models/models.py:176-290 around transformers'
modeling_distilbert.py) and of key-masked attention, with autograd. Plain torch on the CPU, independent of lavila_amd;
pinned to tests/golden/clip_hf_distilbert.pt (generated from the unmodified reference) by tests/test_clip_hf_cpu.py.

The mask rule is transformers': the scores of hidden keys are replaced by the most negative finite value before the
softmax. In float64 a hidden key then has probability exactly 0 and receives no gradient, and a sample with no visible key
gets the uniform distribution over all its keys (every score equals the fill)."""
import math

import torch

EPS = 1e-12


def keymask_attention(q, k, v, mask, heads):
    """q [B, Lq, D], k / v [B, Lk, D] float64; mask [B, Lk] (non-zero = visible) or None. softmax(q k^T / 8) v per head of
    64 channels over the visible keys."""
    B, Lq, D = q.shape
    qh, kh, vh = (t.reshape(B, -1, heads, 64).permute(0, 2, 1, 3) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / 8.0
    if mask is not None:
        s = s.masked_fill((mask == 0)[:, None, None, :], torch.finfo(s.dtype).min)
    return (torch.softmax(s, -1) @ vh).permute(0, 2, 1, 3).reshape(B, Lq, D)


def layer_norm(x, w, b, eps=EPS):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _lin(x, w, name):
    return x @ w[name + '.weight'].t() + w[name + '.bias']


def block(x, mask, w, p, heads):
    a = p + 'attention.'
    o = keymask_attention(_lin(x, w, a + 'q_lin'), _lin(x, w, a + 'k_lin'), _lin(x, w, a + 'v_lin'), mask, heads)
    h = layer_norm(_lin(o, w, a + 'out_lin') + x, w[p + 'sa_layer_norm.weight'], w[p + 'sa_layer_norm.bias'])
    f = _lin(gelu_erf(_lin(h, w, p + 'ffn.lin1')), w, p + 'ffn.lin2')
    return layer_norm(f + h, w[p + 'output_layer_norm.weight'], w[p + 'output_layer_norm.bias'])


def tower(ids, mask, w, heads, prefix=''):
    """last_hidden_state [B, L, D]. w: name -> float64 tensor (the state dict, `prefix` in front of every name)."""
    p = prefix
    L = ids.shape[1]
    x = w[p + 'embeddings.word_embeddings.weight'][ids] + w[p + 'embeddings.position_embeddings.weight'][:L]
    x = layer_norm(x, w[p + 'embeddings.LayerNorm.weight'], w[p + 'embeddings.LayerNorm.bias'])
    layers = 1 + max(int(k[len(p) + 18:].split('.')[0]) for k in w if k.startswith(p + 'transformer.layer.'))
    for i in range(layers):
        x = block(x, mask, w, f'{p}transformer.layer.{i}.', heads)
    return x


def clip_hf_forward(video, ids, mask, w, vision_heads, text_heads, norm_embed=False):
    """CLIP_HF.forward with projection='default' and text_use_cls_token=True; the video tower is the oracle's."""
    from oracle import oracle as O
    img = O.vision_tower(video, w, vision_heads) @ w['image_projection']
    txt = tower(ids, mask, w, text_heads, 'textual.')[:, 0] @ w['text_projection']
    if norm_embed:
        img, txt = O.l2_normalize(img), O.l2_normalize(txt)
    return {'image_embed': img, 'text_embed': txt, 'logit_scale': w['logit_scale'].exp()}


def doubles(w, grad=True):
    """float64 leaves of a float32 state dict."""
    return {k: v.double().clone().requires_grad_(grad and v.is_floating_point()) for k, v in w.items()}
