"""CPU: the host side of narrator training -- the float64 oracle's gradients against the reference's own
(tests/golden/narrator_train.pt, written by tools/gen_narrator_train_golden.py from the unmodified narrator.py +
gpt2_gated.py + CaptionLoss in `.eval()`), which is what entitles the GPU tests to use the oracle; the `VCLM_*` criterion and
metric names; the decoder's dropout refusal and the dropout fields of gpt2_config().

The reference's losses on these fixtures are 10.51 (freq1_gated) and 11.86 (freq2_plain): sum of the token losses over
B * T positions, pads counted in the denominator, as loss.py:234-236 computes it."""
import math
import types

import pytest
import torch

from caption_loss_reference import rows_forward
from conftest import load_golden
from oracle import oracle as O

VARIANTS = ['freq1_gated', 'freq2_plain']
_cache = {}


def _oracle_step(variant):
    """One float64 step of the oracle on the fixture of narrator_decoder.pt: (loss, name -> gradient)."""
    if variant not in _cache:
        fx = load_golden('narrator_decoder.pt')
        c, v = fx['config'], fx['variants'][variant]
        w = O.narrator_weights(v['shapes'], seed=v['weight_seed'])
        wo = {k: t.double().requires_grad_(True) for k, t in w.items()}
        wo['text_decoder.lm_head.weight'] = wo['text_decoder.transformer.wte.weight']
        video, _ = O.synthetic_batch(c['batch'], c['frames'], c['img'], seed=v['input_seed'])
        out = O.narrator_forward(video.double(), v['text'], wo, c['heads'], c['pool_heads'], c['pool_heads'])
        logits, labels = out['text_tokens_logits'], out['labels']
        B, V, T = logits.shape
        _, nll, _, _, _ = rows_forward(logits.permute(0, 2, 1).reshape(B * T, V), labels.reshape(-1), v['pad'])
        loss = nll.sum() / (B * T)
        loss.backward()
        _cache[variant] = (loss.item(), {k: t.grad for k, t in wo.items() if k != 'text_decoder.lm_head.weight'})
    return _cache[variant]


@pytest.mark.parametrize('variant', VARIANTS)
def test_oracle_gradients_match_reference(variant):
    """Every stored gradient, slice and norm: ||got - want|| <= max(1e-3 ||want||, 1e-6 scale), scale = the RMS norm of a
    parameter's gradient (1e-3: the project's fp32 parity bar; the reference ran in float32)."""
    g = load_golden('narrator_train.pt')['variants'][variant]
    loss, grads = _oracle_step(variant)
    assert set(grads) == set(g['grad_norms'])
    assert abs(loss - g['loss']) <= 1e-3 * abs(g['loss'])
    scale = math.sqrt(sum(n * n for n in g['grad_norms'].values()) / len(g['grad_norms']))
    worst = (0.0, None)
    for k, n in g['grad_norms'].items():
        d = abs(grads[k].norm().item() - n)
        assert d <= max(1e-3 * n, 1e-6 * scale), (k, d, n)
    for k, want in g['grads'].items():
        d, n = (grads[k] - want.double()).norm().item(), want.double().norm().item()
        worst = max(worst, (d / max(n, 1e-300) if n > 1e-3 * scale else 0.0, k))
        assert d <= max(1e-3 * n, 1e-6 * scale), (k, d, n)
    for k, (rows, want) in g['grad_slices'].items():
        got = grads[k].reshape(grads[k].shape[0], -1)[rows]
        d, n = (got - want.double()).norm().item(), want.double().norm().item()
        worst = max(worst, (d / max(n, 1e-300) if n > 1e-3 * scale else 0.0, k))
        assert d <= max(1e-3 * n, 1e-6 * scale), (k, d, n)
    assert len(g['grads']) + len(g['grad_slices']) == len(grads)
    print(f'[oracle vs reference {variant}] loss {loss:.4f} / {g["loss"]:.4f}; worst relative L2 {worst[0]:.2e} ({worst[1]}); '
          f'scale {scale:.3g}')


@pytest.mark.parametrize('variant', VARIANTS)
def test_fixture_gradients_are_not_degenerate(variant):
    _, grads = _oracle_step(variant)
    zero = [k for k, t in grads.items() if t is None or not t.any()]
    assert not zero, zero


def test_vclm_metric_names_and_loss():
    from lavila.models import models
    name = 'VCLM_OPENAI_TIMESFORMER_BASE_GPT2'
    assert models.get_metric_names(name) == ['loss', 'caption_loss', 'caption_acc', 'ppl']
    args = type('A', (), dict(contrastive_use_vissl=True, rank=0, world_size=1))
    crit = models.get_loss(name, args, tokenizer=types.SimpleNamespace(pad_token_id=7))
    assert isinstance(crit, models.loss.CaptionLoss) and crit.pad_id == 7
    with pytest.raises(NotImplementedError, match='pad id'):
        models.get_loss(name, args)
    with pytest.raises(NotImplementedError):
        models.get_metric_names('SOMETHING_ELSE')


def test_gpt2_config_has_explicit_zero_dropout():
    from lavila_amd.gpt2_gated import augment_gpt2_config, gpt2_config
    cfg = gpt2_config('gpt2')
    assert (cfg.resid_pdrop, cfg.embd_pdrop, cfg.attn_pdrop) == (0.0, 0.0, 0.0)
    aug = augment_gpt2_config(gpt2_config('gpt2', attn_pdrop=0.1))
    assert aug.attn_pdrop == 0.1 and aug.resid_pdrop == 0.0


def test_decoder_refuses_to_train_with_dropout():
    """A non-zero dropout field + training mode + the training plan: NotImplementedError naming the fields, raised before any
    device work (so it shows on a machine without a GPU); float32 with gradients keeps its own refusal."""
    from lavila_amd.gpt2_gated import GPT2LMHeadModel, augment_gpt2_config, gpt2_config
    cfg = augment_gpt2_config(gpt2_config('gpt2', vocab_size=50, n_positions=16, n_embd=64, n_layer=1, n_head=1,
                                          resid_pdrop=0.1, attn_pdrop=0.2))
    dec = GPT2LMHeadModel(cfg).bfloat16()
    ids = torch.ones(1, 4, dtype=torch.long)
    dec.train()
    with pytest.raises(NotImplementedError, match='resid_pdrop / attn_pdrop'):
        dec(ids)
    dec.float()
    with pytest.raises(NotImplementedError, match='bf16'):
        dec(ids)
