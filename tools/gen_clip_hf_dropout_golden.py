"""Writes tests/golden/clip_hf_distilbert_dropout.pt: the UNMODIFIED reference CLIP_HF (oracle.ref_import) around
transformers' own DistilBertModel in `.train()` WITH the dropout that DistilBertConfig() carries (dropout =
attention_dropout = 0.1), eager attention, float32 on the CPU. Data only. CONFIG, seeds and inputs() are those of
tools/gen_clip_hf_golden.py.

The reference draws its masks from torch's generator; this tower draws them from Philox4x32-10 over (seed, site, element)
inside its kernels (include/lavila_hip.h, the text tower's mask contract). So that one step can be compared,
torch.nn.functional.dropout is replaced FOR THE DURATION OF A FORWARD by a function that multiplies by the restated mask
(tests/distilbert_dropout_reference.py) of the next site times 1 / (1 - p). modeling_distilbert.py calls it 1 + 2 n_layers
times, in site order: the embedding [B, L, D], per layer the attention probabilities [B, H, L, L] and the output of ffn.lin2
[B, L, D]. Calls with p == 0 (the video tower's nn.Dropout(0.)) pass through and consume no site. Nothing of the
reference's or transformers' program text is touched or copied.

Assertions that run with the tool: an all-ones injection reproduces the `.eval()` outputs bit for bit, and every site is
used exactly once per forward, with the shape of its kind.

  (A) one training step of the dual encoder with CLIPLoss on mask set A (its longest caption fills all 21 positions, so the
      trim changes no index): last_hidden_state, embeddings, logit_scale, loss, gradients.
  (B) the text tower alone on mask set B (holes, key 0 hidden, one visible key) with the stored upstream.
Gradients as gen_clip_hf_golden.py stores them: 1-D tensors in full, four rows of every 2-D one.

The seed is chosen from the reference's own numbers alone, before any kernel runs (tools/gen_narrator_dropout_golden.py):
SEED0 + i * SEED_STEP for the first i at which no parameter's gradient norm under dropout, in (A) or (B), falls below a
tenth of its norm in the tool's own p = 0 run. Rejected candidates are printed; the index is stored as `seed_index`.

    python tools/gen_clip_hf_dropout_golden.py        (needs the reference tree and transformers; see oracle/ref_import.py)
"""
import contextlib
import io
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

import distilbert_dropout_reference as DD  # noqa: E402
import dropout_reference as DR  # noqa: E402
from gen_clip_hf_golden import CONFIG, INPUT_SEED, WEIGHT_SEED, inputs, select  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle.ref_import import load_reference  # noqa: E402

SEED0, SEED_STEP = 0x5EEDC0DE0B5E55ED, 0x9E3779B97F4A7C15
MAX_CANDIDATES = 32
MIN_NORM_RATIO = 0.1


def build(ref, c, hf):
    from transformers import DistilBertConfig, DistilBertModel
    with contextlib.redirect_stdout(io.StringIO()):
        vis = ref.timesformer.SpaceTimeTransformer(
            img_size=c['img'], patch_size=c['patch'], embed_dim=c['dim'], depth=c['depth'], num_heads=c['heads'],
            num_frames=c['frames'], time_init='zeros', attention_style='frozen-in-time', ln_pre=True,
            act_layer=ref.openai_model.QuickGELU)
        vis.head = vis.pre_logits = vis.fc = nn.Identity()
        cfg = DistilBertConfig(vocab_size=c['vocab'], max_position_embeddings=c['positions'], dim=c['t_dim'],
                               n_heads=c['t_heads'], n_layers=c['t_layers'], hidden_dim=c['t_hidden'],
                               dropout=hf['dropout'], attention_dropout=hf['attention_dropout'])
        cfg._attn_implementation = 'eager'
        text = DistilBertModel(cfg)
        model = ref.models.CLIP_HF(embed_dim=c['embed'], vision_width=c['dim'], vision_model=vis, text_width=c['t_dim'],
                                   text_model=text, text_use_cls_token=True, text_is_regressive=False)
    return model


@contextlib.contextmanager
def injected(seed, n_layers, heads, identity=False):
    """torch.nn.functional.dropout -> the restated mask of the next site, for the forwards inside; yields the list of
    (site, shape) used."""
    used = []
    orig = F.dropout

    def dropout(input, p=0.5, training=True, inplace=False):
        if p == 0.0 or not training:
            return orig(input, p, training, inplace)
        site = len(used)
        used.append((site, tuple(input.shape)))
        assert site < 1 + 2 * n_layers, used
        if input.dim() == 4:
            assert site % 2 == 1, used
            B, H, L, Tk = input.shape
            assert H == heads and L == Tk
            keep = DD.attn_keep(seed, site, B, H, L, Tk, 0.0 if identity else p)
        else:
            assert site % 2 == 0 and input.dim() == 3, used
            B, L, D = input.shape
            keep = DD.row_keep(seed, site, B * L, D, 0.0 if identity else p).reshape(B, L, D)
        scale = 1.0 if identity else float(DR.scale(p))
        return input * (torch.from_numpy(keep).to(input.dtype) * scale)

    F.dropout = torch.nn.functional.dropout = dropout
    try:
        yield used
    finally:
        F.dropout = torch.nn.functional.dropout = orig


def check_sites(used, c, B, L):
    want = [(0, (B, L, c['t_dim']))]
    for n in range(c['t_layers']):
        want += [(1 + 2 * n, (B, c['t_heads'], L, L)), (2 + 2 * n, (B, L, c['t_dim']))]
    assert used == want, (used, want)          # every site exactly once, in order, with the shape of its kind


def run(ref, model, c, data, seed, identity):
    """(A) and (B) of one seed: two dicts with outputs and name -> gradient."""
    video, ids, mask_a, mask_b, upstream = data
    B, L = ids.shape
    model.train()
    model.zero_grad(set_to_none=True)
    kept = {}
    h = model.textual.register_forward_hook(lambda m, i, o: kept.__setitem__('lhs', o.last_hidden_state.detach().clone()))
    with injected(seed, c['t_layers'], c['t_heads'], identity) as used:
        out = model(video, ids, mask=mask_a, norm_embed=True)
    h.remove()
    check_sites(used, c, B, L)
    ld = ref.loss.CLIPLoss(use_vissl=False, cache_labels=True, rank=0, world_size=1)(out)
    ld['loss'].backward()
    ga = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    a = {'last_hidden_state': kept['lhs'], 'image_embed': out['image_embed'].detach(), 'text_embed': out['text_embed'].detach(),
         'logit_scale': out['logit_scale'].detach(), 'loss': ld['loss'].detach()}
    model.zero_grad(set_to_none=True)
    with injected(seed, c['t_layers'], c['t_heads'], identity) as used:
        lhs = model.textual(ids, attention_mask=mask_b).last_hidden_state
    check_sites(used, c, B, L)
    (lhs * upstream * mask_b[..., None]).sum().backward()
    gb = {k: p.grad.detach().clone() for k, p in model.textual.named_parameters()}
    return (a, ga), ({'last_hidden_state': lhs.detach().clone()}, gb)


def main():
    from transformers import DistilBertConfig
    ref = load_reference()
    c = CONFIG
    d = DistilBertConfig()
    hf = {'dropout': float(d.dropout), 'attention_dropout': float(d.attention_dropout)}
    model = build(ref, c, hf)
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    print(model.load_state_dict(O.procedural_weights(dict(shapes), seed=WEIGHT_SEED), strict=True))
    data = inputs(c, INPUT_SEED)
    video, ids, mask_a, mask_b, upstream = data

    # the all-ones injection is the .eval() forward, bit for bit (nothing else of the model depends on train mode)
    model.eval()
    with torch.no_grad():
        ev = model(video, ids, mask=mask_a, norm_embed=True)
        ev_lhs = model.textual(ids, attention_mask=mask_b).last_hidden_state
    (a0, ga0), (b0, gb0) = run(ref, model, c, data, SEED0, identity=True)
    assert torch.equal(a0['image_embed'], ev['image_embed']) and torch.equal(a0['text_embed'], ev['text_embed'])
    assert torch.equal(b0['last_hidden_state'], ev_lhs), 'the identity injection changed the forward'
    plain_a = {k: g.norm().item() for k, g in ga0.items()}
    plain_b = {k: g.norm().item() for k, g in gb0.items()}

    for index in range(MAX_CANDIDATES):
        seed = (SEED0 + index * SEED_STEP) & 0xFFFFFFFFFFFFFFFF
        (a, ga), (b, gb) = run(ref, model, c, data, seed, identity=False)
        weak = [(w, k, g.norm().item(), pl[k]) for w, gs, pl in (('A', ga, plain_a), ('B', gb, plain_b)) for k, g in gs.items()
                if g.norm().item() < MIN_NORM_RATIO * pl[k]]
        if not weak:
            break
        print(f'[golden] seed candidate {index} ({seed:#x}) rejected: gradient norms below {MIN_NORM_RATIO} of the p = 0 '
              f'run\'s: {[(w, k, round(x, 6), round(y, 6)) for w, k, x, y in weak]}')
    else:
        raise SystemExit('no seed candidate gave a non-degenerate fixture')
    assert not torch.equal(a['text_embed'], a0['text_embed'])
    assert float(ga['textual.embeddings.word_embeddings.weight'][0].abs().max()) == 0          # padding_idx
    for part, grads in ((a, ga), (b, gb)):
        part['grads'], part['grad_slices'] = select(grads)
        part['grad_norms'] = {k: g.norm().item() for k, g in grads.items()}
    fx = {'config': c, 'weight_seed': WEIGHT_SEED, 'input_seed': INPUT_SEED, 'seed': seed, 'seed_index': index,
          'dropout': hf, 'sites': list(range(1 + 2 * c['t_layers'])), 'A': a, 'B': b,
          'plain_grad_norms': {'A': plain_a, 'B': plain_b}}
    path = os.path.join(ROOT, 'tests', 'golden', 'clip_hf_distilbert_dropout.pt')
    torch.save(fx, path)
    assert os.path.getsize(path) < 1_000_000, os.path.getsize(path)
    print(f'[golden] seed {seed:#x} (candidate {index}), (A) loss {a["loss"].item():.6f} (p = 0: {a0["loss"].item():.6f}) '
          f'-> {path} ({os.path.getsize(path)} bytes)')


if __name__ == '__main__':
    main()
