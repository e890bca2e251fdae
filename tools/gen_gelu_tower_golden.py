"""Writes tests/golden/gelu_tower_clip_hf.pt from the UNMODIFIED reference: lavila/models/models.py:176-290 (CLIP_HF, default
projection, imported through oracle.ref_import.load_reference()) around the reference's DEFAULT-CONSTRUCTED
SpaceTimeTransformer -- act_layer=nn.GELU, ln_pre=False (so the patch embedding has a bias), LayerNorm eps 1e-6: the tower of
CLIP_HF_TIMESFORMER_DISTILBERT_BASE (models.py:691-720) -- and transformers' own DistilBertModel(DistilBertConfig(...)),
randomly initialised (nothing is downloaded). CPU, float32. Data only.

  plain   drop_path_rate = 0, train mode: image_embed / text_embed (norm_embed=True), logit_scale, the CLIPLoss loss and the
          gradients of one backward.
  drop    the same step with drop_path_rate = 0.5 (depth 2: block 1 drops at 0.5, block 0 at 0): the per-sample keep masks of
          its two dropping sites are recovered by forward hooks on the reference's DropPath modules and stored, so that a test
          can inject them (DropPath.sample_scale) instead of reproducing torch's CPU generator.
  the state-dict key order and shapes, the parameter names, and the signature of CLIP_HF_TIMESFORMER_DISTILBERT_BASE.

Tower: img 32, patch 16, dim 256 (hidden 1024: the smallest width lvl_linear_tn tiles), heads 4, depth 2 (one MLP deferred
into the next block's norm3, one cls-only last block), frames 2. Text tower: the configuration of
tools/gen_clip_hf_golden.py. Gradients are stored as there: 1-D tensors in full, four rows (0, 1, the middle, the last) of
every 2-D one. Weights are procedural (oracle.procedural_weights by name and shape): seeds and shapes are stored, not tensors.

    python tools/gen_gelu_tower_golden.py        (needs the reference tree and transformers; see oracle/ref_import.py)
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
              img=32, patch=16, dim=256, depth=2, heads=4, frames=2, embed=64, batch=6, length=21, drop_path_rate=0.5)
WEIGHT_SEED, INPUT_SEED = 29, 7
PREFIX_LENGTHS = (1, 5, 16, 17, 21, 21)
CONSTRUCTOR = 'CLIP_HF_TIMESFORMER_DISTILBERT_BASE'


def inputs(c, seed):
    """video, ids [B, L] int64, mask [B, L] float32 (what the reference's tokenizer hands)."""
    B, L = c['batch'], c['length']
    video, _ = O.synthetic_batch(B, c['frames'], c['img'], seed=seed)
    torch.manual_seed(seed)
    ids = torch.randint(1, c['vocab'], (B, L))
    mask = torch.zeros(B, L)
    for b, n in enumerate(PREFIX_LENGTHS):
        mask[b, :n] = 1
    return video, ids * mask.long(), mask


def build(ref, c, drop_path_rate):
    from transformers import DistilBertConfig, DistilBertModel
    with contextlib.redirect_stdout(io.StringIO()):
        # every argument the constructor under test leaves at its default is left at its default here
        vis = ref.timesformer.SpaceTimeTransformer(
            img_size=c['img'], patch_size=c['patch'], embed_dim=c['dim'], depth=c['depth'], num_heads=c['heads'],
            num_frames=c['frames'], time_init='zeros', attention_style='frozen-in-time', drop_path_rate=drop_path_rate)
        vis.head = vis.pre_logits = vis.fc = nn.Identity()
        text = DistilBertModel(DistilBertConfig(
            vocab_size=c['vocab'], max_position_embeddings=c['positions'], dim=c['t_dim'], n_heads=c['t_heads'],
            n_layers=c['t_layers'], hidden_dim=c['t_hidden'], dropout=0.0, attention_dropout=0.0))
        model = ref.models.CLIP_HF(embed_dim=c['embed'], vision_width=c['dim'], vision_model=vis, text_width=c['t_dim'],
                                   text_model=text, text_use_cls_token=True, text_is_regressive=False)
    assert isinstance(vis.blocks[0].mlp.act, nn.GELU) and vis.ln_pre is None and vis.norm.eps == 1e-6
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


def step(ref, c, drop_path_rate, seed=None):
    """One training step -> (model, record, keep masks {block name: {'space': [B] int64, 'mlp': [B] int64}})."""
    model = build(ref, c, drop_path_rate)
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict(O.procedural_weights(dict(shapes), seed=WEIGHT_SEED), strict=True)
    model.train()
    sites = []

    def hook(name):
        def fn(mod, args, out):
            sites.append((name, (out.detach().reshape(out.shape[0], -1).abs().amax(1) > 0).to(torch.int64)))
        return fn
    handles = [blk.drop_path.register_forward_hook(hook(f'blocks.{i}'))
               for i, blk in enumerate(model.visual.blocks) if not isinstance(blk.drop_path, nn.Identity)]
    video, ids, mask = inputs(c, INPUT_SEED)
    if seed is not None:
        torch.manual_seed(seed)               # the forward that follows draws the drop-path masks from this stream
    out = model(video, ids, mask=mask, norm_embed=True)
    for h in handles:
        h.remove()
    ld = ref.loss.CLIPLoss(use_vissl=False, cache_labels=True, rank=0, world_size=1)(out)
    ld['loss'].backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    assert set(grads) == {k for k, _ in model.named_parameters()}
    full, slices = select(grads)
    rec = {'image_embed': out['image_embed'].detach(), 'text_embed': out['text_embed'].detach(),
           'logit_scale': out['logit_scale'].detach(), 'loss': ld['loss'].detach(), 'grads': full, 'grad_slices': slices,
           'grad_norms': {k: g.norm().item() for k, g in grads.items()}}
    masks = {}
    for name, keep in sites:                  # two calls per block, in the block's order: space branch, then MLP branch
        masks.setdefault(name, []).append(keep)
    masks = {k: {'space': v[0], 'mlp': v[1]} for k, v in masks.items()}
    return model, shapes, rec, masks


def main():
    ref = load_reference()
    c = CONFIG
    model, shapes, plain, none = step(ref, c, 0.0)
    assert not none
    e = plain['image_embed']
    off = ~torch.eye(c['batch'], dtype=torch.bool)
    print(f'[golden] plain: loss {plain["loss"].item():.6f}, image cosines mean {(e @ e.T)[off].mean().item():.3f} max '
          f'{(e @ e.T)[off].max().item():.3f}, {len(plain["grads"])} full gradients, {len(plain["grad_slices"])} sliced')
    seed = None
    for s in range(100):                      # a seed under which both sites keep some samples and drop some
        _, shapes_d, drop, masks = step(ref, c, c['drop_path_rate'], seed=s)
        if all(0 < int(m.sum()) < c['batch'] for site in masks.values() for m in site.values()):
            seed = s
            break
    assert seed is not None and list(masks) == ['blocks.1'] and shapes_d == shapes, masks
    assert abs(drop['loss'].item() - plain['loss'].item()) > 1e-3          # the masks did drop something
    drop['masks'], drop['seed'] = masks, seed
    print(f'[golden] drop: seed {seed}, loss {drop["loss"].item():.6f}, masks '
          + str({k: {n: m.tolist() for n, m in v.items()} for k, v in masks.items()}))
    keys = [k for k, _ in shapes]
    assert 'visual.patch_embed.proj.bias' in keys and not any(k.startswith('visual.ln_pre.') for k in keys)
    fx = {'config': c, 'weight_seed': WEIGHT_SEED, 'input_seed': INPUT_SEED, 'state_dict': shapes,
          'param_names': [k for k, _ in model.named_parameters()], 'prefix_lengths': PREFIX_LENGTHS,
          'plain': plain, 'drop': drop,
          'signatures': {CONSTRUCTOR: str(inspect.signature(getattr(ref.models, CONSTRUCTOR)))}}
    path = os.path.join(ROOT, 'tests', 'golden', 'gelu_tower_clip_hf.pt')
    torch.save(fx, path)
    assert os.path.getsize(path) < 1_000_000, os.path.getsize(path)
    print(f'[golden] -> {path} ({os.path.getsize(path)} bytes)')


if __name__ == '__main__':
    main()
