"""GPU (-m gpu): the OpenAI CLIP image tower end to end -- openai_model.VisionTransformer, openai_model.CLIP (the per-frame
zero-shot baseline) and VCLM_HF around the tower (the per-frame narrators) -- against the UNMODIFIED reference's recorded
results (tests/golden/vit_tower.pt, tools/gen_vit_tower_golden.py; weights and inputs rebuilt from seeds by
tests/vit_tower_helpers.py).

float32: 1e-3 on embeddings / logits / loss (the project's parity bar), gradients by helpers.check_fixture_gradients with the
figures test_gpu_f32_class applies to format-2 fixtures. bf16: the criteria of test_tsfb_bf16_training_step_vs_oracle_f32
(embeddings 2.5e-2 relative L2, logits 0.1, loss 2e-2; gradients through test_gpu_narrator_train._compare_step, which is
that test's gradient criterion) -- derived there for 12 blocks, held here by 3."""
import contextlib
import io
import types

import pytest
import torch

import vit_tower_helpers as V
from conftest import load_golden
from helpers import check_fixture_gradients
from lavila_amd.guards import forbid_library_gemm
from oracle import oracle as O
from oracle.gen_golden import DECODER, NARRATOR
from test_gpu_full_attention import full_attention_f64
from test_gpu_narrator_train import _compare_step

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF = torch.bfloat16
F32 = dict(atol=1e-3, rtol=1e-3)


@pytest.fixture(scope='module')
def golden():
    return load_golden('vit_tower.pt')


def _rel(a, b):
    return ((a.float().cpu() - b).norm() / b.norm().clamp_min(1e-30)).item()


def _tower(name, fx):
    from lavila.models.openai_model import VisionTransformer
    c = V.TOWERS[name]
    vis = VisionTransformer(c['resolution'], c['patch'], c['width'], c['layers'], c['heads'], c['output_dim'])
    vis.load_state_dict(V.tower_weights(fx['towers'][name]['shapes'], c['weight_seed']), strict=True)
    return vis.to(DEV).eval(), V.tower_images(c).to(DEV)


def _clip():
    from lavila.models.openai_model import build_model
    return build_model(V.clip_state_dict(V.clip_shapes(), V.CLIP['weight_seed']))


def _narrator(fx, width=None, heads=None, vis=None):
    from lavila_amd.gpt2_gated import GPT2LMHeadModel, augment_gpt2_config, gpt2_config
    from lavila_amd.narrator import VCLM_HF
    c, d, v = NARRATOR, DECODER, fx['narrator']
    width, heads = width or c['text_width'], heads or c['pool_heads']
    vis = vis or _clip().visual
    base = gpt2_config('gpt2', vocab_size=d['vocab'], n_positions=d['positions'], n_embd=width, n_layer=d['layers'],
                       n_head=heads)
    dec = GPT2LMHeadModel(augment_gpt2_config(base, **v['variant']))
    m = VCLM_HF(vision_width=vis.conv1.weight.shape[0], vision_model=vis, text_width=width, text_decoder=dec,
                num_img_queries=c['queries'], dim_head=64, heads=heads)
    own = m.state_dict()
    if width == c['text_width']:              # the golden's model: its procedural weights
        w = V.tune_tower_weights(O.narrator_weights(v['shapes'], seed=V.NARRATOR_SEED))
        assert set(v['shapes']) | set(v['kept_buffers']) | {'text_decoder.lm_head.weight'} == set(own)
    else:
        shapes = {k: tuple(t.shape) for k, t in own.items()
                  if k not in v['kept_buffers'] and k != 'text_decoder.lm_head.weight'}
        w = V.tune_tower_weights(O.narrator_weights(shapes, seed=V.NARRATOR_SEED))
    for k in v['kept_buffers']:
        w[k] = own[k]
    m.load_state_dict(w, strict=True)
    video, _ = O.synthetic_batch(c['batch'], V.CLIP['frames'], vis.input_resolution, seed=V.NARRATOR_INPUT_SEED, spread=True)
    tok = types.SimpleNamespace(bos_token_id=v['bos'], eos_token_id=-1, pad_token_id=v['pad'])
    return m.to(DEV).eval(), video.to(DEV), tok


def _golden_items(rec, grads):
    """(got, want) over what the golden holds: full gradients and the recorded rows of the larger tensors."""
    got, want = {}, {}
    for k, g in rec['grads'].items():
        got[k], want[k] = grads[k].detach().float().cpu(), g.double()
    for k, (rows, g) in rec['grad_slices'].items():
        t = grads[k].detach().float().cpu()
        got[k + '[rows]'], want[k + '[rows]'] = t.reshape(t.shape[0], -1)[rows], g.double()
    return got, want


# ----------------------------------------------------------------------------------------------------------------------
# the tower
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(V.TOWERS))
def test_tower_float32_matches_the_reference(name, golden):
    """Both modes and both projections, 16-pixel patches and 14-pixel ones (588 contraction elements); the 5-D entry gives
    the rows of the per-image entry in (b, t) order; fp16 in -> fp16 out."""
    vis, x = _tower(name, golden)
    fx = golden['towers'][name]
    with torch.no_grad():
        got = {'cls_proj': vis(x), 'cls': vis(x, apply_project=False), 'tokens': vis(x, cls_at_last=False)}
        clip = torch.stack([x, x.flip(0)], dim=2)                                # [B, 3, T=2, H, W]
        rows = vis.forward_clip(clip)
        rows_tok = vis.forward_clip(clip, cls_at_last=False)
        half = vis.half()(x.half())                                              # model.half(): bf16 inside, fp16 back
    for k, t in got.items():
        assert t.dtype == torch.float32 and t.shape == fx[k].shape, k
        print(f'[tower {name}] {k}: max |d| {(t.cpu() - fx[k]).abs().max():.2e}')
        torch.testing.assert_close(t.cpu(), fx[k], **F32, msg=lambda m: f'{k}: {m}')
    B = x.shape[0]
    want_rows = torch.stack([got['cls_proj'], got['cls_proj'].flip(0)], dim=1).reshape(2 * B, -1)
    torch.testing.assert_close(rows, want_rows, atol=1e-5, rtol=1e-5)            # same kernels, other row order
    want_tok = torch.stack([got['tokens'], got['tokens'].flip(0)], dim=1).reshape(2 * B, *got['tokens'].shape[1:])
    torch.testing.assert_close(rows_tok, want_tok, atol=1e-5, rtol=1e-5)
    assert half.dtype == torch.float16
    assert _rel(half, fx['cls_proj']) < 2.5e-2


@pytest.mark.parametrize('name', sorted(V.TOWERS))
def test_tower_bf16_autocast(name, golden):
    vis, x = _tower(name, golden)
    fx = golden['towers'][name]
    with torch.no_grad(), torch.autocast('cuda', dtype=BF):
        got = {'cls_proj': vis(x), 'cls': vis(x, apply_project=False), 'tokens': vis(x, cls_at_last=False)}
    for k, t in got.items():
        assert t.dtype == BF, k
        e = _rel(t, fx[k])
        print(f'[tower {name} bf16] {k}: rel L2 {e:.2e}')
        assert e < 2.5e-2, (k, e)          # measured 6.1e-3 .. 8.5e-3 (3 blocks; the bar is the 12-block one)


# ----------------------------------------------------------------------------------------------------------------------
# openai_model.CLIP
# ----------------------------------------------------------------------------------------------------------------------
def _clip_step(model, video, tokens, autocast=False, use_checkpoint=False):
    from lavila.models.loss import CLIPLoss
    model.zero_grad(set_to_none=True)
    crit = CLIPLoss(use_vissl=False, cache_labels=True, rank=0, world_size=1)
    with torch.autocast('cuda', dtype=BF) if autocast else contextlib.nullcontext():
        out = model(video, tokens, use_checkpoint=use_checkpoint)
        ld = crit(out)
    ld['loss'].backward()
    logits = crit.debug_slabs(out)['logits'][0]
    torch.cuda.synchronize()
    return out, ld, logits, {k: p.grad for k, p in model.named_parameters()}


@pytest.fixture(scope='module')
def clip_f32():
    """One float32 training step of the tiny CLIP, shared by the tests that compare against it."""
    model = _clip().to(DEV)
    images, video, tokens = (t.to(DEV) for t in V.clip_inputs())
    out, ld, logits, grads = _clip_step(model, video, tokens)
    keep = {k: g.clone() for k, g in grads.items()}
    return model, (images, video, tokens), out, ld, logits, keep


def test_clip_float32_matches_the_reference(golden, clip_f32):
    fx = golden['clip']
    model, (images, video, tokens), out, ld, logits, grads = clip_f32
    assert not fx['no_gradient'] and all(g is not None for g in grads.values())
    with torch.no_grad():
        enc = {'encode_image_4d': model.encode_image(images), 'encode_image_5d': model.encode_image(video),
               'encode_image_5d_noproj': model.encode_image(video, apply_project=False),
               'encode_text': model.encode_text(tokens)}
    for k, t in enc.items():
        print(f'[clip f32] {k}: max |d| {(t.cpu() - fx[k]).abs().max():.2e}')
        torch.testing.assert_close(t.cpu(), fx[k], **F32, msg=lambda m: f'{k}: {m}')
    assert set(out) == {'image_embed', 'text_embed', 'logit_scale'}
    for k in ('image_embed', 'text_embed', 'logit_scale'):
        torch.testing.assert_close(out[k].detach().cpu(), fx[k], **F32, msg=lambda m: f'{k}: {m}')
    torch.testing.assert_close(logits.cpu(), fx['logits_per_image'], **F32)
    torch.testing.assert_close(ld['loss'].detach().cpu(), fx['loss'], **F32)
    torch.testing.assert_close(ld['clip_acc'].detach().cpu().float(), fx['clip_acc'].float())
    worst = check_fixture_gradients(fx, grads, rtol=2e-3, norm_rtol=5e-3, tag='tiny openai CLIP ')
    print(f'[clip f32] |d loss| {abs(ld["loss"].item() - fx["loss"].item()):.2e}, worst gradient tensor (own scale) {worst:.2e}')


def test_clip_bf16_autocast_step(golden):
    fx = golden['clip']
    model = _clip().to(DEV)
    _, video, tokens = (t.to(DEV) for t in V.clip_inputs())
    out, ld, logits, grads = _clip_step(model, video, tokens, autocast=True)
    e_img, e_txt = _rel(out['image_embed'], fx['image_embed']), _rel(out['text_embed'], fx['text_embed'])
    dlogit = (logits.float().cpu() - fx['logits_per_image']).abs().max().item()
    print(f'[clip bf16] rel L2 image {e_img:.2e} text {e_txt:.2e}, max |d logit| {dlogit:.3f}')
    # measured: 8.1e-3 / 1.0e-2 / 0.068; gradients aggregate 2.1e-2, worst tensor 3.6e-2, |d loss| 5.8e-3
    assert e_img < 2.5e-2 and e_txt < 2.5e-2 and dlogit < 0.1, (e_img, e_txt, dlogit)
    got, want = _golden_items(fx, grads)
    _compare_step('tiny openai CLIP bf16', got, want, ld['loss'].item(), fx['loss'].item())


def test_clip_last_block_on_the_cls_rows_equals_the_whole_block(clip_f32, monkeypatch):
    """CLS_ONLY_LAST_BLOCK off: the last block of both towers runs on every row, as the reference does. Same outputs and
    gradients at the float32 bar."""
    from lavila_amd import timesformer
    model, (_, video, tokens), out, ld, logits, grads = clip_f32
    assert timesformer.CLS_ONLY_LAST_BLOCK
    monkeypatch.setattr(timesformer, 'CLS_ONLY_LAST_BLOCK', False)
    out2, ld2, logits2, grads2 = _clip_step(model, video, tokens)
    for k in ('image_embed', 'text_embed'):
        torch.testing.assert_close(out2[k], out[k], **F32)
    torch.testing.assert_close(logits2, logits, **F32)
    torch.testing.assert_close(ld2['loss'], ld['loss'], **F32)
    for k, g in grads.items():
        scale = g.abs().max().item()
        assert (grads2[k] - g).abs().max().item() <= 2e-3 * scale + 1e-9, k        # check_fixture_gradients' own-scale figure


def test_clip_block_checkpointing_gives_the_plain_gradients(clip_f32):
    """use_checkpoint=True recomputes every block with the kernels of the plain forward: the same values, up to the order of
    float32 atomic additions (1e-6 of every tensor's own scale)."""
    model, (_, video, tokens), out, ld, logits, grads = clip_f32
    out2, ld2, _, grads2 = _clip_step(model, video, tokens, use_checkpoint=True)
    assert abs(ld2['loss'].item() - ld['loss'].item()) <= 1e-6 * abs(ld['loss'].item())
    for k, g in grads.items():
        assert (grads2[k] - g).abs().max().item() <= 1e-6 * g.abs().max().item() + 1e-12, k


# ----------------------------------------------------------------------------------------------------------------------
# the per-frame narrator
# ----------------------------------------------------------------------------------------------------------------------
def test_narrator_float32_forward_and_greedy_decode(golden):
    from lavila.models.loss import CaptionLoss
    fx = golden['narrator']
    m, video, tok = _narrator(golden)
    text = fx['text'].to(DEV)
    with torch.no_grad():
        img = m.encode_image(video)
        out = m(video, text)
        torch.testing.assert_close(img.cpu(), fx['image_tokens'], **F32)
        assert torch.equal(out['labels'].cpu(), fx['labels'])
        print(f'[vit narrator f32] max |d image_tokens| {(img.cpu() - fx["image_tokens"]).abs().max():.2e}, max |d logit| '
              f'{(out["text_tokens_logits"].cpu() - fx["logits"]).abs().max():.2e}')
        torch.testing.assert_close(out['text_tokens_logits'].cpu(), fx['logits'], **F32)
        loss = CaptionLoss(tokenizer=tok)(out)['loss']
        torch.testing.assert_close(loss.float().cpu().reshape(()), fx['loss'].reshape(()), **F32)
        for cache, graph in ((True, True), (True, False), (False, False)):          # cached (graph / eager) and recomputed
            ids, ppl = m.generate(img, tok, max_text_length=fx['max_text_length'], top_k=1, kv_cache=cache, graph=graph)
            assert torch.equal(ids.cpu(), fx['free_ids']), (cache, graph)
            torch.testing.assert_close(ppl.cpu(), fx['free_ppl'], atol=0, rtol=5e-3)      # test_gpu_narrator's figure


@pytest.mark.parametrize('use_checkpoint', [False, True])
def test_narrator_bf16_training_step(golden, use_checkpoint, monkeypatch):
    """forward -> CaptionLoss -> backward through decoder, pooler and the per-frame tower under bf16 autocast (the decoder
    trains in bf16 only), plain and with block checkpointing; packed captions and the decoder-side switches are
    decoder-side: one packed step gives the same loss and gradients."""
    from lavila.models.loss import CaptionLoss
    from lavila_amd import narrator
    fx = golden['narrator']
    m, video, tok = _narrator(golden)
    text = fx['text'].to(DEV)
    crit = CaptionLoss(tokenizer=tok)

    def step():
        m.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=BF):
            res = crit(m(video, text, use_checkpoint=use_checkpoint))
        res['loss'].backward()
        torch.cuda.synchronize()
        return res['loss'].item(), {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}

    loss, grads = step()
    assert sorted(k for k, g in grads.items() if g is None) == sorted(fx['no_gradient'])      # ln_post / proj: not on this path
    got, want = _golden_items(fx, grads)
    _compare_step(f'vit narrator bf16 (checkpoint={use_checkpoint})', got, want, loss, fx['loss'].item())
    if not use_checkpoint:
        monkeypatch.setattr(narrator, 'PACK_CAPTIONS', True)
        loss_p, grads_p = step()
        got_p, _ = _golden_items(fx, grads_p)
        _compare_step('vit narrator bf16, packed captions', got_p, want, loss_p, fx['loss'].item())


# ----------------------------------------------------------------------------------------------------------------------
# own GEMMs at tiling widths; one block at the real geometries
# ----------------------------------------------------------------------------------------------------------------------
def test_wide_tower_and_clip_train_without_library_gemms(golden):
    """256-wide towers (every Linear tiles lvl_linear_tn / lvl_linear_wgrad; 14-pixel patches: the zero-pad-to-640 patch
    embedding), bf16 autocast, every library GEMM entry point of torch forbidden: a CLIP step end to end, and the
    narrator's tower forward + backward on all patch rows. (The narrator's pooling projection to_kv has 128 outputs and
    trains on the library GEMM, as it does around the TimeSformer towers: the whole narrator step runs without the guard.)"""
    from lavila.models.loss import CaptionLoss
    from lavila.models.openai_model import CLIP
    torch.manual_seed(1)
    with contextlib.redirect_stdout(io.StringIO()):
        model = CLIP(256, 28, 2, 256, 14, 16, 64, 256, 4, 2).to(DEV).train()
    _, _, tokens = V.clip_inputs()
    video, _ = O.synthetic_batch(3, 2, 28, seed=9, spread=True)
    video, tokens = video.to(DEV), tokens.to(DEV)
    with forbid_library_gemm():
        out, ld, logits, grads = _clip_step(model, video, tokens, autocast=True)
    assert torch.isfinite(ld['loss']) and all(g is not None and torch.isfinite(g).all() for g in grads.values())
    vis = model.visual
    vis.zero_grad(set_to_none=True)
    with forbid_library_gemm(), torch.autocast('cuda', dtype=BF):
        x = vis.forward_clip(video, cls_at_last=False, use_checkpoint=True)
        assert x.shape == (6, 4, 256)
        x.float().square().mean().backward()
    missing = sorted(k for k, p in vis.named_parameters() if p.grad is None)
    assert missing == ['ln_post.bias', 'ln_post.weight', 'proj'], missing
    assert all(torch.isfinite(p.grad).all() and p.grad.any() for p in vis.parameters() if p.grad is not None)
    m, _, tok = _narrator(golden, width=256, heads=4, vis=vis.cpu())
    m.train()
    text = golden['narrator']['text'].to(DEV)
    with torch.autocast('cuda', dtype=BF):
        res = CaptionLoss(tokenizer=tok)(m(video, text))
    res['loss'].backward()
    assert torch.isfinite(res['loss']) and all(p.grad is None or torch.isfinite(p.grad).all() for p in m.parameters())


def _block_f64(x, w, heads):
    """openai_model.py:206-216 without a mask, float64, batch-major."""
    def ln(t, g, b):
        return torch.nn.functional.layer_norm(t, t.shape[-1:], g, b, 1e-5)
    h = ln(x, w['ln_1.weight'], w['ln_1.bias'])
    qkv = h @ w['attn.in_proj_weight'].t() + w['attn.in_proj_bias']
    x = x + full_attention_f64(qkv, heads) @ w['attn.out_proj.weight'].t() + w['attn.out_proj.bias']
    u = ln(x, w['ln_2.weight'], w['ln_2.bias']) @ w['mlp.c_fc.weight'].t() + w['mlp.c_fc.bias']
    return x + (u * torch.sigmoid(1.702 * u)) @ w['mlp.c_proj.weight'].t() + w['mlp.c_proj.bias']


@pytest.mark.parametrize('width,heads,B,L', [(768, 12, 2, 197), (1024, 16, 1, 577)])
def test_one_block_at_the_real_geometries_bf16_vs_float64(width, heads, B, L):
    """ResidualAttentionBlock without a mask at ViT-B/16's and ViT-L/14-at-336's token counts, forward + backward under bf16
    autocast, no library GEMM, no generic attention kernel; against float64 on the same bf16-representable weights and
    input. One block: a third of the roundings the 2.5e-2 / _compare_step criteria were derived for."""
    from lavila.models.openai_model import ResidualAttentionBlock
    from lavila_amd import _cabi as C
    torch.manual_seed(width)
    blk = ResidualAttentionBlock(width, heads)
    shapes = {k: tuple(t.shape) for k, t in blk.state_dict().items()}
    w = {k: t.to(BF).float() for k, t in O.procedural_weights(shapes, seed=width, spread=True).items()}
    blk.load_state_dict(w, strict=True)
    blk.to(DEV).train()
    g = torch.Generator().manual_seed(L)
    x = torch.randn(B, L, width, generator=g).to(BF).float()
    up = torch.randn(B, L, width, generator=g).to(BF).float() / (B * L)
    w64 = {k: t.double().requires_grad_(True) for k, t in w.items()}
    x64 = x.double().requires_grad_(True)
    o64 = _block_f64(x64, w64, heads)
    loss64 = (o64 * up.double()).sum()
    loss64.backward()
    C.lib().lvl_debug_generic_attention_calls(1)
    xg = x.to(DEV, BF).requires_grad_(True)             # the tower's stream is bf16 under autocast (ln_pre keeps the token dtype)
    with forbid_library_gemm(), torch.autocast('cuda', dtype=BF):
        x1, y, b = blk.chain(xg, None, None)
        out = x1.float() + y.float() + b
        loss = (out * up.to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert C.lib().lvl_debug_generic_attention_calls(1) == 0
    e = _rel(out.detach(), o64.detach().float())
    assert e < 2.5e-2, e                  # measured 6.3e-3 / 6.4e-3; gradients aggregate 9.5e-3 / 9.7e-3, worst tensor 1.1e-2
    got = {k: p.grad for k, p in blk.named_parameters()}
    got['input'] = xg.grad
    want = {k: t.grad for k, t in w64.items()}
    want['input'] = x64.grad
    _compare_step(f'vit block {width} x {L}', got, want, loss.item(), loss64.item(), extra=[('rel L2 out', e)])
