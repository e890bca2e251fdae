"""Writes tests/golden/narrator_dropout.pt: one training step of the UNMODIFIED reference narrator WITH its decoder's
dropout (transformers' GPT2Config defaults resid / embd / attn_pdrop to 0.1; gpt2_gated.py:186-187, 230, 354, 389-395, 737,
899), float32 on the CPU, `.train()`. The reference draws its masks from torch's generator; this decoder draws them from
Philox4x32-10 over (seed, site, element) inside its kernels (lavila_amd/csrc/dropout.h). So that one step can be compared,
every nn.Dropout INSTANCE of the reference decoder is replaced at run time by a module that multiplies by an injected mask
times 1 / (1 - p), the masks coming from the numpy restatement tests/dropout_reference.py: same seed, same site numbering
(the reference's execution order), same element mapping, attention masks as [B, H, L, Tk]. Nothing of the reference's
program text is touched or copied. Fixtures and format as tools/gen_narrator_train_golden.py (`freq1_gated`, `freq2_plain`,
procedural weights, format 2):

  seed, seed_index, pdrop        the 64-bit seed (see below) and the three probabilities (read from transformers.GPT2Config())
  variants[name]['loss']         the reference's CaptionLoss under the injected masks
  variants[name]['grad_norms']   the norm of every parameter's gradient
  variants[name]['grads']        the full gradient of every tensor of at most 4096 elements
  variants[name]['grad_slices']  rows (0, a middle one, the last) of the larger ones, seen as [shape[0], -1]
  variants[name]['sites']        the site ids used by the forward, each exactly once

Two assertions run with the tool: injection with p = 0 reproduces the stored `.eval()` logits bit for bit (the hooks change
nothing else, and nothing else of the model depends on train mode), and every site id is used exactly once per forward.

The seed. A fixture must not be degenerate (tests/test_narrator_train_cpu.py::test_fixture_gradients_are_not_degenerate asks
that of the `.eval()` step). Under dropout one more way to degenerate opens: the gradient of a tanh gate is ONE number, the sum
of B L D products of order one, and a mask can make that sum cancel -- with the first seed tried, 0x5EEDC0DE0B5E55ED, the
reference's d alpha_cattn of block 0 is -0.0152 where the `.eval()` step has -1.33 (and d alpha_dense of block 1 -0.026 against
-1.24). A comparison RELATIVE to such a number measures the rounding of the 88 times larger terms, in any arithmetic. So the
seed is chosen from the reference's own numbers alone, before any kernel runs: SEED0 + i * SEED_STEP for the first i at which
no parameter's gradient norm under dropout falls below a tenth of its norm in tests/golden/narrator_train.pt, in both variants.
The candidates that were rejected are printed, and the chosen index is stored as `seed_index`.

    python tools/gen_narrator_dropout_golden.py        (needs the reference tree; see oracle/ref_import.py)
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import dropout_reference as R  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle.gen_golden import DECODER, NARRATOR, decoder_weights  # noqa: E402
from oracle.ref_import import load_reference_narrator  # noqa: E402

FULL_MAX = 4096
SEED0, SEED_STEP = 0x5EEDC0DE0B5E55ED, 0x9E3779B97F4A7C15          # non-zero high words; see "The seed" above
MAX_CANDIDATES = 32
MIN_NORM_RATIO = 0.1


def slice_rows(n):
    return sorted({0, n // 2, n - 1} & set(range(n)))


class InjectedDropout(nn.Module):
    """Stands where an nn.Dropout stood: x * mask / (1 - p) with the restated mask of its site."""

    def __init__(self, state, site, p, attention):
        super().__init__()
        self.state, self.site, self.p, self.attention = state, site, p, attention

    def forward(self, x):
        self.state['used'].append(self.site)
        seed = self.state['seed']
        if self.attention:
            B, H, L, Tk = x.shape
            keep = R.attn_mask(seed, self.site, B, H, L, Tk, self.p)
        else:
            B, L, D = x.shape
            keep = R.row_mask(seed, self.site, B * L, D, self.p).reshape(B, L, D)
        return x * (torch.from_numpy(np.ascontiguousarray(keep)).to(x.dtype) * float(R.scale(self.p)))


def inject(dec, state, pdrop):
    """Replaces every nn.Dropout of the reference decoder; -> the site ids a forward with image tokens must use."""
    tr = dec.transformer
    assert isinstance(tr.drop, nn.Dropout)
    tr.drop = InjectedDropout(state, 0, pdrop['embd_pdrop'], False)
    expect = [0]
    for i, blk in enumerate(tr.h):
        slots = [('attn', 3, 4), ('mlp', None, 5)]
        if hasattr(blk, 'crossattention'):
            slots += [('crossattention', 0, 1), ('mlp_crossattention', None, 2)]
        for name, k_attn, k_resid in slots:
            mod = getattr(blk, name)
            if k_attn is not None:
                assert isinstance(mod.attn_dropout, nn.Dropout) and isinstance(mod.resid_dropout, nn.Dropout)
                mod.attn_dropout = InjectedDropout(state, R.site_of(i, k_attn), pdrop['attn_pdrop'], True)
                mod.resid_dropout = InjectedDropout(state, R.site_of(i, k_resid), pdrop['resid_pdrop'], False)
                expect += [R.site_of(i, k_attn), R.site_of(i, k_resid)]
            else:
                assert isinstance(mod.dropout, nn.Dropout)
                mod.dropout = InjectedDropout(state, R.site_of(i, k_resid), pdrop['resid_pdrop'], False)
                expect.append(R.site_of(i, k_resid))
    left = [n for n, m in dec.named_modules() if isinstance(m, nn.Dropout)]
    assert not left, left
    return sorted(expect)


def build_variants(ref, pdrop):
    """The reference narrators of both fixtures with injected dropout modules, after the p = 0 check."""
    from transformers import GPT2Config
    c, d = NARRATOR, DECODER
    stored = torch.load(os.path.join(ROOT, 'tests', 'golden', 'narrator_decoder.pt'), weights_only=False)
    built = {}
    for name, var in d['variants'].items():
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
        video, _ = O.synthetic_batch(c['batch'], c['frames'], c['img'], seed=v['input_seed'])
        model.train()
        # the hooks with p = 0: the stored .eval() forward, bit for bit
        state = {'seed': SEED0, 'used': []}
        expect = inject(dec, state, dict.fromkeys(pdrop, 0.0))
        with torch.no_grad():
            fwd = model(video, v['text'])
        assert torch.equal(fwd['text_tokens_logits'], v['logits']), 'p = 0 injection changed the forward'
        assert sorted(state['used']) == expect, (sorted(state['used']), expect)
        assert inject_again(dec, pdrop) == len(expect)
        built[name] = (model, state, expect, video, v)
    return built


def step(ref, model, state, expect, video, v, seed):
    """One training step of the reference under the masks of `seed`: (loss, name -> gradient)."""
    state['seed'], state['used'] = seed, []
    model.zero_grad(set_to_none=True)
    fwd = model(video, v['text'])
    assert sorted(state['used']) == expect, (sorted(state['used']), expect)      # every site exactly once
    assert not torch.equal(fwd['text_tokens_logits'].detach(), v['logits'])
    res = ref.loss.CaptionLoss(tokenizer=SimpleNamespace(pad_token_id=v['pad']))(fwd)
    res['loss'].backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    assert all(g is not None for g in grads.values())
    return res['loss'].item(), grads


def main():
    from transformers import GPT2Config
    ref = load_reference_narrator()
    hf = GPT2Config()
    pdrop = {k: float(getattr(hf, k)) for k in ('resid_pdrop', 'embd_pdrop', 'attn_pdrop')}
    plain = torch.load(os.path.join(ROOT, 'tests', 'golden', 'narrator_train.pt'), weights_only=False)['variants']
    built = build_variants(ref, pdrop)
    for index in range(MAX_CANDIDATES):
        seed = (SEED0 + index * SEED_STEP) & 0xFFFFFFFFFFFFFFFF
        steps = {name: step(ref, m, st, ex, video, v, seed) for name, (m, st, ex, video, v) in built.items()}
        weak = [(name, k, g.norm().item(), plain[name]['grad_norms'][k]) for name, (_, grads) in steps.items()
                for k, g in grads.items() if g.norm().item() < MIN_NORM_RATIO * plain[name]['grad_norms'][k]]
        if not weak:
            break
        print(f'[golden] seed candidate {index} ({seed:#x}) rejected: gradient norms below {MIN_NORM_RATIO} of the .eval() '
              f'step\'s: {[(n, k, round(a, 5), round(b, 5)) for n, k, a, b in weak]}')
    else:
        raise SystemExit('no seed candidate gave a non-degenerate fixture')
    out = {'format': 2, 'seed': seed, 'seed_index': index, 'pdrop': pdrop, 'variants': {}}
    for name, (loss, grads) in steps.items():
        full = {k: g.clone() for k, g in grads.items() if g.numel() <= FULL_MAX}
        slices = {}
        for k, g in grads.items():
            if g.numel() > FULL_MAX:
                g2 = g.reshape(g.shape[0], -1)
                rows = slice_rows(g2.shape[0])
                slices[k] = (rows, g2[rows].clone())
        out['variants'][name] = {'loss': loss, 'grad_norms': {k: g.norm().item() for k, g in grads.items()},
                                 'grads': full, 'grad_slices': slices, 'sites': built[name][2]}
        print(f'[golden] {name}: seed {seed:#x} (candidate {index}), loss {loss:.4f}, sites {built[name][2]}, '
              f'{len(full)} full gradients, {len(slices)} sliced')
    path = os.path.join(ROOT, 'tests', 'golden', 'narrator_dropout.pt')
    torch.save(out, path)
    print(f'[golden] -> {path} ({os.path.getsize(path)} bytes)')


def inject_again(dec, pdrop):
    """Sets the probabilities of the injected modules (attention sites attn_pdrop, site 0 embd_pdrop, the rest resid_pdrop)."""
    n = 0
    for m in dec.modules():
        if isinstance(m, InjectedDropout):
            m.p = pdrop['attn_pdrop'] if m.attention else pdrop['embd_pdrop' if m.site == 0 else 'resid_pdrop']
            n += 1
    return n


if __name__ == '__main__':
    main()
