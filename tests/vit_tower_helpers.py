"""Shared by tools/gen_vit_tower_golden.py (which records the reference) and the tests of the OpenAI CLIP image tower
(test_vit_tower_cpu.py, test_gpu_vit_tower.py): the tiny configurations, their procedural weights and inputs. Nothing here
touches the reference tree: both sides rebuild identical tensors from seeds."""
import torch

from oracle import oracle as O

# openai_model.VisionTransformer(input_resolution, patch_size, width, layers, heads, output_dim): 2 x 2 patches of 16
# pixels, and 2 x 2 patches of 14 (3 * 14 * 14 = 588 contraction elements: no multiple of the GEMMs' 64-element K block)
TOWERS = {
    'p16': dict(resolution=32, patch=16, width=128, layers=3, heads=2, output_dim=64, batch=3, weight_seed=41, input_seed=51),
    'p14': dict(resolution=28, patch=14, width=128, layers=3, heads=2, output_dim=64, batch=3, weight_seed=42, input_seed=52),
}

# openai_model.CLIP through build_model: the ten constructor arguments follow from the state dict's shapes
CLIP = dict(embed=64, resolution=32, patch=16, vision_width=128, vision_layers=3, context=16, vocab=64, text_width=128,
            text_layers=2, batch=3, frames=2, weight_seed=43, input_seed=53)

NARRATOR_SEED = 44          # weights of the tiny VCLM_HF around CLIP's tower (decoder: gen_golden.DECODER / NARRATOR widths)
NARRATOR_INPUT_SEED = 54

FULL_MAX = 4096             # gradients up to this many elements are stored in full, four rows of the larger ones


def slice_rows(n):
    return sorted({0, 1, n // 2, n - 1} & set(range(n)))


def tune_tower_weights(weights):
    """oracle.procedural_weights knows the TimeSformer's names; for the ViT's it would give a patch embedding of scale
    P^-0.5 (100 x the positions) -- here: conv1 at (3 P P)^-0.5 like `patch_embed`, positions and class embedding of a
    size that moves the output (0.2), so a wrong position row cannot hide. In place; returns the dict."""
    for k, t in weights.items():
        if k.endswith('conv1.weight'):
            t.mul_((3 * t.shape[2]) ** -0.5)
        elif k.endswith('visual.positional_embedding'):
            t.mul_(10.0)
        elif k.endswith('class_embedding'):
            t.mul_(0.2 * t.shape[0] ** 0.5)
    return weights


def tower_weights(shapes, seed):
    """Weights of a bare VisionTransformer (names without prefix): generated under the `visual.` prefix so that the tuning
    above applies to a tower inside a CLIP and to a bare one alike."""
    w = tune_tower_weights(O.procedural_weights({'visual.' + k: s for k, s in shapes.items()}, seed=seed))
    return {k[len('visual.'):]: t for k, t in w.items()}


def tower_images(cfg):
    g = torch.Generator().manual_seed(cfg['input_seed'])
    return torch.randn(cfg['batch'], 3, cfg['resolution'], cfg['resolution'], generator=g)


def clip_state_dict(shapes, seed):
    """A procedural OpenAI-CLIP state dict whose every tensor is fp16-representable, as the published checkpoints are: the
    reference's build_model converts the Linear / conv / attention / projection weights to fp16 on the way in
    (openai_model.py:483), which is then the identity."""
    w = tune_tower_weights(O.procedural_weights(shapes, seed=seed))
    return {k: t.half().float() for k, t in w.items()}


def clip_shapes(c=None):
    """name -> shape of the tiny CLIP's state dict (what build_model infers the constructor arguments from)."""
    c = c or CLIP
    W, T, P, g = c['vision_width'], c['text_width'], c['patch'], c['resolution'] // c['patch']
    s = {'positional_embedding': (c['context'], T), 'text_projection': (T, c['embed']), 'logit_scale': (),
         'visual.class_embedding': (W,), 'visual.positional_embedding': (g * g + 1, W), 'visual.proj': (W, c['embed']),
         'visual.conv1.weight': (W, 3, P, P), 'visual.ln_pre.weight': (W,), 'visual.ln_pre.bias': (W,),
         'visual.ln_post.weight': (W,), 'visual.ln_post.bias': (W,), 'token_embedding.weight': (c['vocab'], T),
         'ln_final.weight': (T,), 'ln_final.bias': (T,)}
    for pre, n, d in (('visual.transformer', c['vision_layers'], W), ('transformer', c['text_layers'], T)):
        for i in range(n):
            b = f'{pre}.resblocks.{i}.'
            s.update({b + 'attn.in_proj_weight': (3 * d, d), b + 'attn.in_proj_bias': (3 * d,),
                      b + 'attn.out_proj.weight': (d, d), b + 'attn.out_proj.bias': (d,),
                      b + 'ln_1.weight': (d,), b + 'ln_1.bias': (d,), b + 'ln_2.weight': (d,), b + 'ln_2.bias': (d,),
                      b + 'mlp.c_fc.weight': (4 * d, d), b + 'mlp.c_fc.bias': (4 * d,),
                      b + 'mlp.c_proj.weight': (d, 4 * d), b + 'mlp.c_proj.bias': (d,)})
    return s


def clip_inputs(c=None):
    """(images [B,3,H,W], clip [B,3,T,H,W], tokens [B, context]): captions of ragged lengths, SOT = vocab - 2 first, EOT =
    vocab - 1 (the highest id: argmax finds it, openai_model.py:395), zero padding behind."""
    c = c or CLIP
    g = torch.Generator().manual_seed(c['input_seed'])
    images = torch.randn(c['batch'], 3, c['resolution'], c['resolution'], generator=g)
    video, _ = O.synthetic_batch(c['batch'], c['frames'], c['resolution'], seed=c['input_seed'] + 1, spread=True)
    tokens = torch.zeros(c['batch'], c['context'], dtype=torch.long)
    for b in range(c['batch']):
        n = c['context'] - 3 * b                      # 16, 13, 10 positions: the longest caption fills the context
        tokens[b, 0] = c['vocab'] - 2
        tokens[b, 1:n - 1] = torch.randint(1, c['vocab'] - 2, (n - 2,), generator=g)
        tokens[b, n - 1] = c['vocab'] - 1
    return images, video, tokens


def pack_gradients(grads):
    """format-2 gradient record (oracle/gen_golden.py): norms of all, small tensors in full, four rows of the larger ones."""
    full = {k: g.clone() for k, g in grads.items() if g.numel() <= FULL_MAX}
    slices = {}
    for k, g in grads.items():
        if g.numel() > FULL_MAX:
            g2 = g.reshape(g.shape[0], -1)
            rows = slice_rows(g2.shape[0])
            slices[k] = (rows, g2[rows].clone())
    return {'grad_norms': {k: g.norm().item() for k, g in grads.items()}, 'grads': full, 'grad_slices': slices}
