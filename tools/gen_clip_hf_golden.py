"""Writes tests/golden/clip_hf_distilbert.pt from the UNMODIFIED reference: lavila/models/models.py:176-290 (CLIP_HF,
imported through oracle.ref_import.load_reference()) around transformers' own DistilBertModel(DistilBertConfig(...)),
randomly initialised (nothing is downloaded), and the reference's SpaceTimeTransformer. CPU, float32. Data only.

  (A) mask set A (prefix lengths 1, 5, 16, 17, 21, 21), the dual encoder in train mode: last_hidden_state of the text
      tower, image_embed / text_embed (norm_embed=True), logit_scale, the CLIPLoss loss and the gradients of one backward.
  (B) mask set B (holes; a sample whose key 0 is hidden; a sample with only its last key visible), the text tower alone:
      last_hidden_state and the gradients of sum(last_hidden_state * upstream) over the visible rows.
  (C) the state-dict key order and shapes, and the signatures of CLIP_HF and of the three
      CLIP_OPENAI_TIMESFORMER_*_DISTILBERT_BASE constructors.

Gradients are stored as oracle/gen_golden.py's select_gradients does: 1-D tensors in full, four rows (0, 1, the middle,
the last) of every 2-D one. Weights are procedural (oracle.procedural_weights by name and shape): seeds and shapes are
stored, not tensors; the token ids, masks and the upstream of (B) are drawn behind torch.manual_seed(input_seed) by
`inputs()` below and stored too (a few KB).

    python tools/gen_clip_hf_golden.py        (needs the reference tree and transformers; see oracle/ref_import.py)
"""
import contextlib
import inspect
import io
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from oracle import oracle as O  # noqa: E402
from oracle.ref_import import load_reference  # noqa: E402

CONFIG = dict(vocab=128, positions=40, t_dim=256, t_heads=4, t_layers=2, t_hidden=512,
              img=32, patch=16, dim=128, depth=1, heads=2, frames=2, embed=64, batch=6, length=21)
WEIGHT_SEED, INPUT_SEED = 23, 5
PREFIX_LENGTHS = (1, 5, 16, 17, 21, 21)
CONSTRUCTORS = ('CLIP_OPENAI_TIMESFORMER_BASE_DISTILBERT_BASE', 'CLIP_OPENAI_TIMESFORMER_LARGE_DISTILBERT_BASE',
                'CLIP_OPENAI_TIMESFORMER_LARGE_336PX_DISTILBERT_BASE')


def inputs(c, seed):
    """video, ids [B, L] int64, mask A and mask B [B, L] float32 (what the reference's tokenizer hands), upstream of (B)."""
    B, L = c['batch'], c['length']
    video, _ = O.synthetic_batch(B, c['frames'], c['img'], seed=seed)
    torch.manual_seed(seed)
    ids = torch.randint(1, c['vocab'], (B, L))
    mask_a = torch.zeros(B, L)
    for b, n in enumerate(PREFIX_LENGTHS):
        mask_a[b, :n] = 1
    ids = ids * mask_a.long()                  # the tokenizer pads with id 0 = padding_idx
    ids[4, 3] = 0                              # ... and one VISIBLE token with the padding id (its table row gets no gradient)
    mask_b = (torch.rand(B, L) < 0.6).float()  # holes
    mask_b[0, 0], mask_b[0, 1] = 0, 1          # key 0 hidden
    mask_b[1] = 0
    mask_b[1, L - 1] = 1                       # only the last key visible
    mask_b[2] = 1                              # all visible
    mask_b[3, 0], mask_b[3, 15:] = 1, 0        # holes inside a prefix of 15
    mask_b[3, 7] = 0
    upstream = torch.randn(B, L, c['t_dim']) / L        # gradients of O(1), as those of the contrastive loss in (A)
    return video, ids, mask_a, mask_b, upstream


def build(ref, c):
    from transformers import DistilBertConfig, DistilBertModel
    with contextlib.redirect_stdout(io.StringIO()):
        vis = ref.timesformer.SpaceTimeTransformer(
            img_size=c['img'], patch_size=c['patch'], embed_dim=c['dim'], depth=c['depth'], num_heads=c['heads'],
            num_frames=c['frames'], time_init='zeros', attention_style='frozen-in-time', ln_pre=True,
            act_layer=ref.openai_model.QuickGELU)
        vis.head = vis.pre_logits = vis.fc = nn.Identity()
        text = DistilBertModel(DistilBertConfig(
            vocab_size=c['vocab'], max_position_embeddings=c['positions'], dim=c['t_dim'], n_heads=c['t_heads'],
            n_layers=c['t_layers'], hidden_dim=c['t_hidden'], dropout=0.0, attention_dropout=0.0))
        model = ref.models.CLIP_HF(embed_dim=c['embed'], vision_width=c['dim'], vision_model=vis, text_width=c['t_dim'],
                                   text_model=text, text_use_cls_token=True, text_is_regressive=False)
    return model


def select(grads):
    full, slices = {}, {}
    for k, g in grads.items():
        if g.ndim <= 1:
            full[k] = g.clone()
        else:
            g2 = g.reshape(-1, g.shape[-1]) if g.ndim == 3 else g.reshape(g.shape[0], -1)
            rows = sorted({0, min(1, g2.shape[0] - 1), g2.shape[0] // 2, g2.shape[0] - 1})
            slices[k] = (rows, g2[rows].clone())
    return full, slices


def main():
    ref = load_reference()
    c = CONFIG
    model = build(ref, c)
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    print(model.load_state_dict(O.procedural_weights(dict(shapes), seed=WEIGHT_SEED), strict=True))
    model.train()
    video, ids, mask_a, mask_b, upstream = inputs(c, INPUT_SEED)

    # (A) the dual encoder
    kept = {}
    h = model.textual.register_forward_hook(lambda m, i, o: kept.__setitem__('lhs', o.last_hidden_state.detach().clone()))
    out = model(video, ids, mask=mask_a, norm_embed=True)
    h.remove()
    ld = ref.loss.CLIPLoss(use_vissl=False, cache_labels=True, rank=0, world_size=1)(out)
    ld['loss'].backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    assert set(grads) == {k for k, _ in model.named_parameters()}
    assert float(grads['textual.embeddings.word_embeddings.weight'][0].abs().max()) == 0          # padding_idx
    assert float(grads['textual.embeddings.position_embeddings.weight'][max(PREFIX_LENGTHS):].abs().max()) == 0
    full, slices = select(grads)
    a = {'last_hidden_state': kept['lhs'], 'image_embed': out['image_embed'].detach(), 'text_embed': out['text_embed'].detach(),
         'logit_scale': out['logit_scale'].detach(), 'loss': ld['loss'].detach(), 'grads': full, 'grad_slices': slices,
         'grad_norms': {k: g.norm().item() for k, g in grads.items()}}
    e_t = a['text_embed']
    off = ~torch.eye(c['batch'], dtype=torch.bool)
    print(f'[golden] (A) loss {ld["loss"].item():.6f}, text cosines mean {(e_t @ e_t.T)[off].mean().item():.3f} '
          f'max {(e_t @ e_t.T)[off].max().item():.3f}, {len(full)} full gradients, {len(slices)} sliced')

    # (B) the text tower alone
    model.zero_grad(set_to_none=True)
    lhs = model.textual(ids, attention_mask=mask_b).last_hidden_state
    (lhs * upstream * mask_b[..., None]).sum().backward()
    tg = {k: p.grad.detach().clone() for k, p in model.textual.named_parameters()}
    full_b, slices_b = select(tg)
    b = {'last_hidden_state': lhs.detach().clone(), 'grads': full_b, 'grad_slices': slices_b,
         'grad_norms': {k: g.norm().item() for k, g in tg.items()}}

    sig = {'CLIP_HF': {k: str(inspect.signature(getattr(ref.models.CLIP_HF, k)))
                       for k in ('__init__', 'encode_image', 'encode_text', 'forward')}}
    for name in CONSTRUCTORS:
        sig[name] = str(inspect.signature(getattr(ref.models, name)))
    fx = {'config': c, 'weight_seed': WEIGHT_SEED, 'input_seed': INPUT_SEED, 'state_dict': shapes,
          'param_names': [k for k, _ in model.named_parameters()],
          'textual_buffers': [k for k, _ in model.textual.named_buffers()],
          'ids': ids, 'mask_a': mask_a, 'mask_b': mask_b, 'upstream_b': upstream, 'A': a, 'B': b, 'signatures': sig}
    path = os.path.join(ROOT, 'tests', 'golden', 'clip_hf_distilbert.pt')
    torch.save(fx, path)
    assert os.path.getsize(path) < 1_000_000, os.path.getsize(path)
    print(f'[golden] -> {path} ({os.path.getsize(path)} bytes)')


if __name__ == '__main__':
    main()
