"""Writes tests/golden/video_classifier.pt from the UNMODIFIED reference (lavila/models/models.py:24-72 around
lavila/models/timesformer.py's SpaceTimeTransformer, imported through oracle.ref_import.load_reference()): the two
classification fine-tune models of main_finetune_classification.py on a small tower WITH stochastic depth. Data only.

  (a) VideoClassifier, 9 classes, eval mode: logits.
  (b) VideoClassifierMultiHead, classes (7, 11, 13), train mode, dropout 0.0, drop_path_rate 0.5 (block rates 0 / 0.25 /
      0.5): the per-sample keep masks of the four dropping sites (recovered by forward hooks on the reference's DropPath
      modules: a sample is kept iff its output rows are non-zero), the three logit tensors, the driver's loss (the sum of
      three CrossEntropyLoss(label_smoothing=0.1) terms, main_finetune_classification.py:333-343), every gradient norm, and
      in full the gradients of the heads, the 1-D parameters, cls_token, pos_embed and temporal_embed.
  (c) the reference's state_dict key order and shapes, and the constructor / forward signatures, of both classes.

Weights and inputs are procedural (oracle.procedural_weights by name and shape; torch.manual_seed(seed) in front of inputs
and forward): seeds and shapes are stored, not tensors. The seed is the first for which every dropping site has at least one
kept and one dropped sample.

    python tools/gen_classifier_golden.py        (needs the reference tree; see oracle/ref_import.py)
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

CONFIG = dict(img=32, patch=16, dim=128, depth=3, heads=2, frames=4, batch=5, drop_path_rate=0.5, label_smoothing=0.1,
              classes_single=9, classes_multi=(7, 11, 13))
WEIGHT_SEED = 11


def build_tower(ref, c):
    with contextlib.redirect_stdout(io.StringIO()):
        return ref.timesformer.SpaceTimeTransformer(
            img_size=c['img'], patch_size=c['patch'], embed_dim=c['dim'], depth=c['depth'], num_heads=c['heads'],
            num_frames=c['frames'], time_init='rand', attention_style='frozen-in-time', ln_pre=True,
            act_layer=ref.openai_model.QuickGELU, num_classes=0, drop_path_rate=c['drop_path_rate'])


def shapes_of(model):
    return [(k, tuple(v.shape)) for k, v in model.state_dict().items()]


def load_procedural(model, seed):
    shapes = dict(shapes_of(model))
    print(model.load_state_dict(O.procedural_weights(shapes, seed=seed)))
    return shapes


def inputs(c, seed):
    """The clip and the three target vectors, drawn right behind torch.manual_seed(seed); the forward that follows draws
    the drop-path masks from the same stream."""
    torch.manual_seed(seed)
    video = torch.randn(c['batch'], 3, c['frames'], c['img'], c['img'])
    targets = [torch.randint(0, n, (c['batch'],)) for n in c['classes_multi']]
    return video, targets


def run_multi(ref, c, seed):
    model = ref.models.VideoClassifierMultiHead(build_tower(ref, c), dropout=0.0, num_classes_list=list(c['classes_multi']))
    shapes = load_procedural(model, WEIGHT_SEED)
    model.train()
    sites = []

    def hook(name):
        def fn(mod, args, out):
            sites.append((name, (out.detach().reshape(out.shape[0], -1).abs().amax(1) > 0).to(torch.int64)))
        return fn
    handles = [blk.drop_path.register_forward_hook(hook(f'blocks.{i}'))
               for i, blk in enumerate(model.visual.blocks) if not isinstance(blk.drop_path, nn.Identity)]
    video, targets = inputs(c, seed)
    logits = model(video)
    for h in handles:
        h.remove()
    crit = nn.CrossEntropyLoss(label_smoothing=c['label_smoothing'])
    loss = sum(crit(lg, t) for lg, t in zip(logits, targets))
    loss.backward()
    masks = {}
    for name, keep in sites:            # two calls per block, in the block's order: space branch, then MLP branch
        masks.setdefault(name, []).append(keep)
    masks = {k: {'space': v[0], 'mlp': v[1]} for k, v in masks.items()}
    return model, shapes, targets, logits, loss, masks


def mixed(masks, batch):
    return all(0 < int(m.sum()) < batch for site in masks.values() for m in site.values())


def main():
    ref = load_reference()
    c = CONFIG
    seed = None
    for s in range(100):
        model, shapes_multi, targets, logits, loss, masks = run_multi(ref, c, s)
        if mixed(masks, c['batch']):
            seed = s
            break
    assert seed is not None and len(masks) == 2, masks
    for lg in logits:
        assert 0.5 <= lg.std().item() <= 3.0, lg.std().item()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    full = {k: g for k, g in grads.items()
            if k.startswith('fc_cls.') or g.dim() == 1 or k.split('.')[-1] in ('cls_token', 'pos_embed', 'temporal_embed')}
    assert len(full) >= 40 and all(g.abs().max().item() > 0 for g in full.values())
    multi = {'format': 2, 'shapes': shapes_multi, 'targets': targets, 'logits': [lg.detach() for lg in logits],
             'loss': loss.item(), 'masks': masks, 'grads': full, 'grad_slices': {},
             'grad_norms': {k: g.norm().item() for k, g in grads.items()}}
    print(f'[golden] multi-head: seed {seed}, loss {loss.item():.6f}, masks '
          + str({k: {n: m.tolist() for n, m in v.items()} for k, v in masks.items()}))

    single = ref.models.VideoClassifier(build_tower(ref, c), dropout=0.0, num_classes=c['classes_single'])
    shapes_single = load_procedural(single, WEIGHT_SEED)
    single.eval()
    video, _ = inputs(c, seed)
    with torch.no_grad():
        logit = single(video)
    assert 0.5 <= logit.std().item() <= 3.0, logit.std().item()
    print(f'[golden] single head: logits std {logit.std().item():.3f}')

    sig = {}
    for name in ('VideoClassifier', 'VideoClassifierMultiHead'):
        cls = getattr(ref.models, name)
        sig[name] = {'init': str(inspect.signature(cls.__init__)), 'forward': str(inspect.signature(cls.forward))}
    fx = {'config': c, 'weight_seed': WEIGHT_SEED, 'input_seed': seed,
          'single': {'shapes': shapes_single, 'logits': logit},
          'multi': multi,
          'state_dict': {'VideoClassifier': shapes_of(single), 'VideoClassifierMultiHead': shapes_of(model)},
          'signatures': sig}
    path = os.path.join(ROOT, 'tests', 'golden', 'video_classifier.pt')
    torch.save(fx, path)
    assert os.path.getsize(path) < 2_000_000
    print(f'[golden] -> {path} ({os.path.getsize(path)} bytes)')


if __name__ == '__main__':
    main()
