"""Writes tests/golden/narrator_train.pt: the gradients of one training step of the UNMODIFIED reference narrator
(lavila/models/narrator.py VCLM_HF + gpt2_gated.py + coca.py + timesformer.py + loss.py CaptionLoss, imported through
oracle.ref_import.load_reference_narrator()), float32 on the CPU, `.eval()` (so that the reference's dropout -- transformers'
GPT2Config defaults resid / embd / attn_pdrop to 0.1 -- is the identity), gradients enabled. The two variants of
tests/golden/narrator_decoder.pt (`freq1_gated`, `freq2_plain`): same procedural weights, same video, same text. Data only,
in the format-2 scheme of oracle/gen_golden.py:

  variants[name]['loss']         the reference's CaptionLoss
  variants[name]['grad_norms']   the norm of every parameter's gradient
  variants[name]['grads']        the full gradient of every tensor of at most 4096 elements
  variants[name]['grad_slices']  rows (0, 1, a middle one, the last) of the larger ones, seen as [shape[0], -1]

    python tools/gen_narrator_train_golden.py        (needs the reference tree; see oracle/ref_import.py)
"""
import os
import sys
from types import SimpleNamespace

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from oracle import oracle as O  # noqa: E402
from oracle.gen_golden import DECODER, NARRATOR, decoder_weights  # noqa: E402
from oracle.ref_import import load_reference_narrator  # noqa: E402

FULL_MAX = 4096


def slice_rows(n):
    return sorted({0, 1, n // 2, n - 1} & set(range(n)))


def main():
    from transformers import GPT2Config
    ref = load_reference_narrator()
    c, d = NARRATOR, DECODER
    stored = torch.load(os.path.join(ROOT, 'tests', 'golden', 'narrator_decoder.pt'), weights_only=False)
    out = {'format': 2, 'variants': {}}
    for vi, (name, var) in enumerate(d['variants'].items()):
        v = stored['variants'][name]
        torch.manual_seed(0)
        vis = ref.timesformer.SpaceTimeTransformer(
            img_size=c['img'], patch_size=c['patch'], embed_dim=c['dim'], depth=c['depth'], num_heads=c['heads'],
            num_frames=c['frames'], time_init='zeros', attention_style='frozen-in-time', ln_pre=True,
            act_layer=ref.openai_model.QuickGELU, is_tanh_gating=False)
        vis.head = vis.pre_logits = vis.fc = nn.Identity()
        base = GPT2Config(vocab_size=d['vocab'], n_positions=d['positions'], n_embd=c['text_width'], n_layer=d['layers'],
                          n_head=c['pool_heads'], use_cache=False, bos_token_id=d['vocab'] - 1, eos_token_id=d['vocab'] - 1)
        dec = ref.gpt2_gated.GPT2LMHeadModel(ref.gpt2_gated.augment_gpt2_config(base, **var))
        model = ref.narrator.VCLM_HF(vision_width=c['dim'], vision_model=vis, text_width=c['text_width'],
                                     text_decoder=dec, num_img_queries=c['queries'], dim_head=64, heads=c['pool_heads'])
        shapes, keep, weights = decoder_weights(model, seed=v['weight_seed'])
        assert shapes == v['shapes']
        model.load_state_dict(weights, strict=True)
        dec.lm_head.weight = dec.transformer.wte.weight
        model.eval()
        video, _ = O.synthetic_batch(c['batch'], c['frames'], c['img'], seed=v['input_seed'])
        fwd = model(video, v['text'])
        assert torch.equal(fwd['text_tokens_logits'].detach(), v['logits'])          # the stored forward, bit for bit
        crit = ref.loss.CaptionLoss(tokenizer=SimpleNamespace(pad_token_id=v['pad']))
        res = crit(fwd)
        res['loss'].backward()
        grads = {k: p.grad.detach() for k, p in model.named_parameters()}
        assert all(g is not None for g in grads.values())
        full = {k: g.clone() for k, g in grads.items() if g.numel() <= FULL_MAX}
        slices = {}
        for k, g in grads.items():
            if g.numel() > FULL_MAX:
                g2 = g.reshape(g.shape[0], -1)
                rows = slice_rows(g2.shape[0])
                slices[k] = (rows, g2[rows].clone())
        out['variants'][name] = {'loss': res['loss'].item(), 'grad_norms': {k: g.norm().item() for k, g in grads.items()},
                                 'grads': full, 'grad_slices': slices}
        zero = [k for k, g in grads.items() if not g.any()]
        print(f'[golden] {name}: loss {res["loss"].item():.4f}, {len(full)} full gradients, {len(slices)} sliced, '
              f'all-zero tensors: {zero}')
    path = os.path.join(ROOT, 'tests', 'golden', 'narrator_train.pt')
    torch.save(out, path)
    print(f'[golden] -> {path} ({os.path.getsize(path)} bytes)')


if __name__ == '__main__':
    main()
