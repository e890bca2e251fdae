"""Writes tests/golden/vit_tower.pt: results of the UNMODIFIED reference's per-frame OpenAI CLIP modules
(lavila/models/openai_model.py VisionTransformer / CLIP / build_model, narrator.py VCLM_HF's VisionTransformer branch,
loss.py CLIPLoss / CaptionLoss; imported through oracle/ref_import.py), float32 on the CPU. Data only, format 2 of
oracle/gen_golden.py: the weights and inputs are procedural (tests/vit_tower_helpers.py rebuilds them from the seeds), the
file holds the recorded results.

  towers[name]     VisionTransformer at width 128 / 2 heads / 3 layers, 16- and 14-pixel patches: `cls_proj`, `cls`
                   (apply_project=False), `tokens` (cls_at_last=False), the state dict's names and shapes
  clip             the tiny openai_model.CLIP built by build_model from a procedural state dict: encode_image on images and
                   on a 2-frame clip, encode_text, the forward dict, CLIPLoss and the gradient record
  narrator         VCLM_HF around that tower with the `freq2_plain` decoder of narrator_decoder.pt's configuration: image
                   tokens, logits, CaptionLoss, the gradient record, greedy generate ids
  real_shapes      names and shapes of the state dicts of the four CLIP_OPENAI_VIT* geometries (built on the meta device)

    python tools/gen_vit_tower_golden.py        (needs the reference tree; see oracle/ref_import.py)
"""
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import vit_tower_helpers as V  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle.gen_golden import DECODER, NARRATOR, decoder_weights  # noqa: E402
from oracle.ref_import import load_reference_narrator  # noqa: E402

REAL = {      # openai_clip.py:31-41's ViT checkpoints: the constructor arguments build_model infers from them
    'ViT-B/32': (512, 224, 12, 768, 32, 77, 49408, 512, 8, 12),
    'ViT-B/16': (512, 224, 12, 768, 16, 77, 49408, 512, 8, 12),
    'ViT-L/14': (768, 224, 24, 1024, 14, 77, 49408, 768, 12, 12),
    'ViT-L/14@336px': (768, 336, 24, 1024, 14, 77, 49408, 768, 12, 12),
}


def run_towers(ref):
    out = {}
    for name, c in V.TOWERS.items():
        torch.manual_seed(0)
        vis = ref.openai_model.VisionTransformer(c['resolution'], c['patch'], c['width'], c['layers'], c['heads'],
                                                 c['output_dim'])
        shapes = {k: tuple(v.shape) for k, v in vis.state_dict().items()}
        vis.load_state_dict(V.tower_weights(shapes, c['weight_seed']), strict=True)
        vis.eval()
        x = V.tower_images(c)
        with torch.no_grad():
            out[name] = {'config': c, 'shapes': shapes, 'state_dict_keys': list(shapes),
                         'cls_proj': vis(x), 'cls': vis(x, apply_project=False), 'tokens': vis(x, cls_at_last=False),
                         'tokens_noproj': vis(x, apply_project=False, cls_at_last=False)}
        assert torch.equal(out[name]['tokens'], out[name].pop('tokens_noproj'))
        print(f'[golden] tower {name}: cls_proj {tuple(out[name]["cls_proj"].shape)} mean |.| '
              f'{out[name]["cls_proj"].abs().mean():.3f}, tokens {tuple(out[name]["tokens"].shape)}')
    return out


def build_clip(ref):
    c = V.CLIP
    shapes = V.clip_shapes(c)
    sd = V.clip_state_dict(shapes, c['weight_seed'])
    model = ref.openai_model.build_model(dict(sd)).float()
    got = model.state_dict()
    assert set(got) == set(sd)
    assert all(torch.equal(got[k], sd[k]) for k in sd), 'build_model changed an fp16-representable value'
    return model, shapes


def run_clip(ref):
    c = V.CLIP
    model, shapes = build_clip(ref)
    model.eval()
    images, video, tokens = V.clip_inputs(c)
    with torch.no_grad():
        rec = {'config': c, 'shapes': shapes, 'state_dict_keys': list(model.state_dict().keys()),
               'encode_image_4d': model.encode_image(images), 'encode_image_5d': model.encode_image(video),
               'encode_image_5d_noproj': model.encode_image(video, apply_project=False),
               'encode_text': model.encode_text(tokens)}
    out = model(video, tokens)
    crit = ref.loss.CLIPLoss(use_vissl=False, cache_labels=True, rank=0, world_size=1)
    ld = crit(out)
    ld['loss'].backward()
    li = (out['logit_scale'] * out['image_embed'] @ out['text_embed'].T).detach()
    grads = {k: p.grad.detach() for k, p in model.named_parameters() if p.grad is not None}
    missing = [k for k, p in model.named_parameters() if p.grad is None]
    rec.update({'format': 2, 'image_embed': out['image_embed'].detach(), 'text_embed': out['text_embed'].detach(),
                'logit_scale': out['logit_scale'].detach(), 'logits_per_image': li, 'loss': ld['loss'].detach(),
                'clip_acc': ld['clip_acc'].detach(), 'no_gradient': missing, **V.pack_gradients(grads)})
    e = rec['image_embed']
    off = ~torch.eye(e.shape[0], dtype=torch.bool)
    print(f'[golden] clip: loss {ld["loss"].item():.4f}, image cosines {(e @ e.T)[off].tolist()}, {len(rec["grads"])} full '
          f'gradients, {len(rec["grad_slices"])} sliced, without gradient: {missing}')
    return rec


def run_narrator(ref):
    from transformers import GPT2Config
    c, d, var = NARRATOR, DECODER, DECODER['variants']['freq2_plain']
    vis = build_clip(ref)[0].visual
    base = GPT2Config(vocab_size=d['vocab'], n_positions=d['positions'], n_embd=c['text_width'], n_layer=d['layers'],
                      n_head=c['pool_heads'], use_cache=False, bos_token_id=d['vocab'] - 1, eos_token_id=d['vocab'] - 1)
    dec = ref.gpt2_gated.GPT2LMHeadModel(ref.gpt2_gated.augment_gpt2_config(base, **var))
    model = ref.narrator.VCLM_HF(vision_width=V.CLIP['vision_width'], vision_model=vis, text_width=c['text_width'],
                                 text_decoder=dec, num_img_queries=c['queries'], dim_head=64, heads=c['pool_heads'])
    shapes, keep, weights = decoder_weights(model, seed=V.NARRATOR_SEED)
    V.tune_tower_weights(weights)
    model.load_state_dict(weights, strict=True)
    dec.lm_head.weight = dec.transformer.wte.weight
    model.eval()
    video, _ = O.synthetic_batch(c['batch'], V.CLIP['frames'], V.CLIP['resolution'], seed=V.NARRATOR_INPUT_SEED, spread=True)
    g = torch.Generator().manual_seed(V.NARRATOR_INPUT_SEED)
    bos = d['vocab'] - 1
    text = torch.randint(1, d['vocab'] - 1, (c['batch'], d['text_len']), generator=g)
    text[:, 0] = bos
    text[1, 9:] = 0                                              # pad (id 0) tail
    tok = SimpleNamespace(bos_token_id=bos, eos_token_id=-1, pad_token_id=0)
    with torch.no_grad():
        image_tokens = model.encode_image(video)
        free_ids, free_ppl = model.generate(image_tokens, tok, max_text_length=d['max_text_length'], top_k=1)
    fwd = model(video, text)
    crit = ref.loss.CaptionLoss(tokenizer=SimpleNamespace(pad_token_id=0))
    res = crit(fwd)
    res['loss'].backward()
    grads = {k: p.grad.detach() for k, p in model.named_parameters() if p.grad is not None}
    missing = [k for k, p in model.named_parameters() if p.grad is None]
    rec = {'format': 2, 'variant': var, 'shapes': shapes, 'kept_buffers': keep, 'text': text, 'bos': bos, 'pad': 0,
           'max_text_length': d['max_text_length'], 'image_tokens': image_tokens,
           'logits': fwd['text_tokens_logits'].detach(), 'labels': fwd['labels'], 'loss': res['loss'].detach(),
           'free_ids': free_ids, 'free_ppl': free_ppl, 'no_gradient': missing, **V.pack_gradients(grads)}
    print(f'[golden] narrator: loss {res["loss"].item():.4f}, greedy {free_ids[0].tolist()}, {len(rec["grads"])} full '
          f'gradients, {len(rec["grad_slices"])} sliced, without gradient: {missing}')
    return rec


def run_real_shapes(ref):
    out = {}
    for name, args in REAL.items():
        with torch.device('meta'):
            m = ref.openai_model.CLIP(*args)
        out[name] = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    return out


def main():
    ref = load_reference_narrator()
    out = {'format': 2, 'towers': run_towers(ref), 'clip': run_clip(ref), 'narrator': run_narrator(ref),
           'real_shapes': run_real_shapes(ref)}
    path = os.path.join(ROOT, 'tests', 'golden', 'vit_tower.pt')
    torch.save(out, path)
    print(f'[golden] -> {path} ({os.path.getsize(path)} bytes)')


if __name__ == '__main__':
    main()
