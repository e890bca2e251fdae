"""GPU: CLIP_HF with the DistilBERT text tower under text dropout (distilbert.TEXT_DROPOUT) against the committed results of
the unmodified reference under injected masks (tests/golden/clip_hf_distilbert_dropout.pt) at the bars of
tests/test_gpu_clip_hf.py, against the float64 restatement on a trimmed batch, and the switch's exactness: pinned seeds,
torch.manual_seed, and everything that must reach the calls and bits of the tower without dropout."""
import contextlib
import io

import pytest
import torch

import clip_hf_helpers as H
import distilbert_dropout_reference as DD
import distilbert_reference as R
from conftest import load_golden
from test_gpu_clip_hf import GTOL, TOL

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _fx():
    return load_golden('clip_hf_distilbert_dropout.pt')


@pytest.fixture
def switched_on(monkeypatch):
    from lavila_amd import distilbert
    monkeypatch.setattr(distilbert, 'TEXT_DROPOUT', True)


def _model(train=True, **text):
    fx = H.fixture()
    m = H.build_model(fx['config'])
    for k, v in text.items():
        setattr(m.textual.config, k, v)
    m.load_state_dict(H.weights(), strict=True)
    m.to(DEV)
    return m.train() if train else m.eval()


def _step(model, mask, amp=None, seed=None):
    from lavila.models.loss import CLIPLoss
    from lavila_amd.gpt2_gated import fixed_dropout_seed
    fx = H.fixture()
    ctx = torch.autocast('cuda', dtype=amp) if amp is not None else contextlib.nullcontext()
    pin = fixed_dropout_seed(seed) if seed is not None else contextlib.nullcontext()
    with ctx, pin:
        out = model(H.video().to(DEV), fx['ids'].to(DEV), mask=None if mask is None else mask.to(DEV), norm_embed=True)
        ld = CLIPLoss(use_vissl=False, cache_labels=True, rank=0, world_size=1)(out)
    ld['loss'].backward()
    torch.cuda.synchronize()
    return out, ld, {k: p.grad.clone() for k, p in model.named_parameters()}


@pytest.mark.parametrize('cls_last', [True, False])
def test_training_step_matches_the_reference_under_its_masks(cls_last, switched_on, monkeypatch):
    """float32 (A) and (B) at TOL / GTOL, with the row-0 last layer on and off."""
    from lavila_amd import timesformer
    from lavila_amd.gpt2_gated import fixed_dropout_seed
    monkeypatch.setattr(timesformer, 'CLS_ONLY_LAST_BLOCK', cls_last)
    fx, base = _fx(), H.fixture()
    A, Bp = fx['A'], fx['B']
    model = _model()
    assert model.textual.config.dropout == fx['dropout']['dropout']
    assert model.textual.config.attention_dropout == fx['dropout']['attention_dropout']
    out, ld, grads = _step(model, base['mask_a'], seed=fx['seed'])
    for k in ('image_embed', 'text_embed', 'logit_scale'):
        err = (out[k].detach().cpu() - A[k]).abs().max().item()
        print(f'[clip_hf dropout fp32 cls_last={cls_last}] {k}: max abs error {err:.2e}')
        torch.testing.assert_close(out[k].detach().cpu(), A[k], **TOL, msg=lambda m, k=k: f'{k}: {m}')
    assert not torch.allclose(out['text_embed'].detach().cpu(), base['A']['text_embed'], atol=1e-2, rtol=0), 'nothing dropped'
    torch.testing.assert_close(ld['loss'].detach().cpu(), A['loss'], **TOL)
    assert H.check_selected(grads, A, **GTOL, what='A') == len(base['param_names'])
    for k, want in A['grad_norms'].items():
        got = grads[k].norm().item()
        assert abs(got - want) <= 5e-3 * want + 1e-6, (k, got, want)
    # (B): the tower alone, all rows, masks with holes
    t = model.textual
    model.zero_grad(set_to_none=True)
    with fixed_dropout_seed(fx['seed']):
        lhs = t(base['ids'].to(DEV), attention_mask=base['mask_b'].to(DEV)).last_hidden_state
    (lhs * base['upstream_b'].to(DEV) * base['mask_b'].to(DEV)[..., None]).sum().backward()
    vis = base['mask_b'].bool()
    torch.testing.assert_close(lhs.detach().cpu()[vis], Bp['last_hidden_state'][vis], **TOL)
    assert torch.isfinite(lhs).all()
    H.check_selected({k: p.grad for k, p in t.named_parameters()}, Bp, **GTOL, what='B')


def test_bf16_autocast_tracks_the_reference(switched_on):
    fx, base = _fx(), H.fixture()
    A = fx['A']
    out, ld, grads = _step(_model(), base['mask_a'], amp=torch.bfloat16, seed=fx['seed'])
    for k in ('image_embed', 'text_embed'):
        print(f'[clip_hf dropout bf16] {k}: max abs error {(out[k].float().cpu() - A[k]).abs().max().item():.2e}')
        torch.testing.assert_close(out[k].detach().float().cpu(), A[k], atol=4e-2, rtol=4e-2)
    assert abs(ld['loss'].item() - A['loss'].item()) < 0.1
    k = 'textual.transformer.layer.0.ffn.lin1.bias'
    g = grads[k]
    assert torch.isfinite(g).all() and g.dtype == torch.float32
    cos = torch.nn.functional.cosine_similarity(g.float().cpu().flatten(), A['grads'][k].flatten(), dim=0)
    assert cos > 0.98, cos


@pytest.mark.parametrize('cls_last', [True, False])
def test_trimmed_batch_matches_the_restatement_on_17_positions(cls_last, switched_on, monkeypatch):
    """A batch whose longest caption is 17 of 21 positions: the tower runs on 17, and so does the mask index."""
    from lavila_amd import timesformer
    from lavila_amd.gpt2_gated import fixed_dropout_seed
    monkeypatch.setattr(timesformer, 'CLS_ONLY_LAST_BLOCK', cls_last)
    fx, base = _fx(), H.fixture()
    c = base['config']
    pd, pa = fx['dropout']['dropout'], fx['dropout']['attention_dropout']
    model = _model()
    mask17 = base['mask_a'].clone()
    mask17[:, 17:] = 0
    with fixed_dropout_seed(fx['seed']):
        te = model.encode_text(base['ids'].to(DEV), attention_mask=mask17.to(DEV))
    up = torch.randn(te.shape, generator=torch.Generator().manual_seed(3))
    (te * up.to(DEV)).sum().backward()
    w = R.doubles({k[len('textual.'):]: v for k, v in H.weights().items() if k.startswith('textual.')})
    proj = H.weights()['text_projection'].double()
    te64 = DD.tower(base['ids'][:, :17], mask17[:, :17], w, c['t_heads'], fx['seed'], pd, pa)[:, 0] @ proj
    (te64 * up.double()).sum().backward()
    torch.testing.assert_close(te.detach().cpu().double(), te64.detach(), **TOL)
    other = DD.tower(base['ids'], mask17, w, c['t_heads'], fx['seed'], pd, pa)[:, 0] @ proj       # the untrimmed index
    assert (other.detach() - te64.detach()).abs().max() > 1e-2
    for k in ('embeddings.position_embeddings.weight', 'transformer.layer.1.attention.k_lin.weight',
              'transformer.layer.0.ffn.lin2.weight'):
        torch.testing.assert_close(dict(model.textual.named_parameters())[k].grad.cpu().double(), w[k].grad, **GTOL,
                                   msg=lambda m, k=k: f'{k}: {m}')


def test_pinned_seed_is_reproducible_and_seeds_differ(switched_on):
    fx, base = _fx(), H.fixture()
    runs = []
    for seed in (fx['seed'], fx['seed'], fx['seed'] + 1):
        out, ld, grads = _step(_model(), base['mask_a'], amp=torch.bfloat16, seed=seed)
        runs.append((ld['loss'].detach().clone(), grads))
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])
    assert not torch.equal(runs[0][1]['text_projection'], runs[2][1]['text_projection'])


def test_manual_seed_reproduces_unpinned_runs(switched_on):
    base = H.fixture()
    runs = []
    for k in (11, 11, 12):
        torch.manual_seed(k)
        out, ld, grads = _step(_model(), base['mask_a'])
        runs.append(grads)
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])
    assert not torch.equal(runs[0]['text_projection'], runs[2]['text_projection'])


def test_without_dropout_the_switch_changes_no_bit(monkeypatch):
    """.eval(), no_grad and p = 0 under the switch: the bits of the switch-off model."""
    from lavila_amd import distilbert
    base = H.fixture()
    ids, mask = base['ids'].to(DEV), base['mask_a'].to(DEV)
    monkeypatch.setattr(distilbert, 'TEXT_DROPOUT', False)
    off = _model()
    out0, ld0, g0 = _step(off, base['mask_a'])
    with torch.no_grad():
        te0 = off.encode_text(ids, attention_mask=mask)
    te0_eval = off.eval().encode_text(ids, attention_mask=mask).detach()
    monkeypatch.setattr(distilbert, 'TEXT_DROPOUT', True)
    on = _model()
    assert on.textual.config.dropout == 0.1
    with torch.no_grad():                                              # train mode, no_grad
        assert torch.equal(on.encode_text(ids, attention_mask=mask), te0)
    on.eval()
    assert torch.equal(on.encode_text(ids, attention_mask=mask).detach(), te0_eval)  # .eval() with grad
    zero = _model(dropout=0.0, attention_dropout=0.0)                  # p = 0 in training
    out1, ld1, g1 = _step(zero, base['mask_a'])
    assert torch.equal(out0['text_embed'], out1['text_embed']) and torch.equal(ld0['loss'], ld1['loss'])
    assert all(torch.equal(g0[k], g1[k]) for k in g0)
    out2, _, _ = _step(on.train(), base['mask_a'])
    assert not torch.equal(out2['text_embed'], out0['text_embed'])


def test_text_tower_with_dropout_runs_on_the_own_gemms_in_bf16(switched_on):
    from lavila_amd.guards import forbid_library_gemm
    base = H.fixture()
    c = dict(base['config'], embed=256)
    with contextlib.redirect_stdout(io.StringIO()):
        model = H.build_model(c)
    model.to(DEV).train()
    assert model.textual.config.dropout == 0.1
    ids, mask = base['ids'].to(DEV), base['mask_a'].to(DEV)
    with forbid_library_gemm():
        with torch.autocast('cuda', dtype=torch.bfloat16):
            te = model.encode_text(ids, attention_mask=mask)
        assert te.dtype == torch.bfloat16 and te.shape == (c['batch'], 256)
        te.float().square().sum().backward()
    torch.cuda.synchronize()
    for k, p in model.textual.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k


def test_float32_stream_with_text_dropout_is_refused(switched_on, monkeypatch):
    from lavila_amd import ops
    monkeypatch.setattr(ops, 'RESIDUAL_F32', True)
    base = H.fixture()
    model = _model()
    with torch.autocast('cuda', dtype=torch.bfloat16):
        with pytest.raises(NotImplementedError, match='LAVILA_RESIDUAL_F32'):
            model.encode_text(base['ids'].to(DEV), attention_mask=base['mask_a'].to(DEV))
