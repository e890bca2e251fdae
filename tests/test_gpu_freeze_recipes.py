"""GPU (-m gpu): the reference's freeze recipes as training steps.

The reference trains almost nothing with every parameter trainable: --timesformer-freeze-space for the dual-encoder
pretrain, --freeze-lm-vclm / --freeze-visual-vclm / --freeze-visual-vclm-temporal for the narrator, frozen temperatures.
Frozen parameters change which code runs (ctx.needs_input_grad branches pick kernels and entry points and drop GEMMs,
rebuilds and tokens). Every recipe here is held to:

  (a) frozen parameters have no gradient, trainable ones a finite one;
  (b) the loss and every trainable gradient equal the unfrozen step on the same inputs to the bit (exceptions:
      freeze_recipes.BITWISE_EXCEPTIONS -- one: the fully frozen 192-wide tower of the golden narrator);
  (c) the trainable subset meets the bars of test_gpu_narrator_train._compare_step (1e-1 per tensor above 1e-3 of the scale,
      5e-2 aggregate, |d loss| <= 2e-2) against the float64 oracle of the unfrozen model;
  (d) with the tower fully frozen nothing of the tower runs in backward (counted);
  (e) a second step is bit-identical;
  (f) after one AdamW step frozen tensors are unchanged to the bit and trainable ones moved.

Stochastic depth has no oracle (the masks are drawn on the device): those cases keep (a), (b), (e), (f)."""
import contextlib
import copy
import io
import math

import pytest
import torch

import freeze_recipes as FR
from helpers import build_model
from oracle import oracle as O
from test_gpu_narrator import _golden_model
from test_gpu_narrator_train import _caption_loss64, _compare_step

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF = torch.bfloat16
DEPTH, BATCH = 2, 2
TOWERS = {'tsfb_4f': dict(img=224, dim=768, heads=12, frames=4),          # _tower of test_gpu_selective_recompute.py
          'small_4f': dict(img=32, dim=256, heads=4, frames=4),           # own kernels, register time kernels
          'small_8f': dict(img=32, dim=256, heads=4, frames=8)}           # own kernels, MFMA time kernels
MODES = {'plain': False, 'block': 'block', 'selective': 'selective'}
_cache = {}


def _build_tower(key, drop_path=0.0):
    from lavila.models.openai_model import QuickGELU
    from lavila.models.timesformer import SpaceTimeTransformer
    t = TOWERS[key]
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        vis = SpaceTimeTransformer(img_size=t['img'], patch_size=16, embed_dim=t['dim'], depth=DEPTH, num_heads=t['heads'],
                                   num_frames=t['frames'], time_init='rand', attention_style='frozen-in-time', ln_pre=True,
                                   act_layer=QuickGELU, num_classes=0, drop_path_rate=drop_path)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in vis.parameters():
            if p.ndim > 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
            else:                      # LayerNorm weights around 1, biases around 0: every gradient is alive
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    return vis.to(DEV).train()


def _tower_case(key, drop_path=0.0):
    """The tower, its inputs and (without stochastic depth) the float64 oracle step; built once per module run."""
    ck = (key, drop_path)
    if ck not in _cache:
        t = TOWERS[key]
        vis = _build_tower(key, drop_path)
        g = torch.Generator().manual_seed(3)
        video = torch.randn(BATCH, 3, t['frames'], t['img'], t['img'], generator=g)
        cot = torch.randn(BATCH, t['dim'], generator=g) / math.sqrt(BATCH * t['dim'])       # a loss of order 1
        oracle = None
        if not drop_path:
            wo = {k: v.detach().double().cpu().requires_grad_(True) for k, v in vis.state_dict().items()}
            loss = (O.vision_tower(video.double(), wo, t['heads'], prefix='') * cot.double()).sum()
            loss.backward()
            oracle = (loss.item(), {k: v.grad for k, v in wo.items()})
        _cache[ck] = (vis, video.to(DEV), cot.to(DEV), oracle, {})
    return _cache[ck]


def _tower_step(vis, video, cot, mode, seed=None):
    vis.zero_grad(set_to_none=True)
    if seed is not None:
        torch.manual_seed(seed)
    with torch.autocast('cuda', dtype=BF):
        out = vis(video, use_checkpoint=mode)
    loss = (out.float() * cot).sum()
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: (None if p.grad is None else p.grad.clone()) for k, p in vis.named_parameters()}


def _check_frozen_step(tag, flags, frozen, again, unfrozen, oracle, exceptions=()):
    """(a), (b), (c), (e) for one recipe: `frozen` / `again` two steps under the recipe, `unfrozen` the step with every parameter
    trainable, each (loss, {name: grad or None}). exceptions: the recipe's entry of FR.BITWISE_EXCEPTIONS (name patterns)."""
    assert any(flags.values()) and not all(flags.values()), tag
    loss, grads = frozen
    assert bool(torch.isfinite(loss)), tag
    if '' not in exceptions:
        assert torch.equal(loss, unfrozen[0]), f'{tag}: the loss differs from the unfrozen step'
    assert torch.equal(loss, again[0]), f'{tag}: the second step has another loss'
    for k, on in flags.items():
        if not on:
            assert grads[k] is None and again[1][k] is None, f'{tag}: frozen {k} has a gradient'
            continue
        assert grads[k] is not None and bool(torch.isfinite(grads[k]).all()), f'{tag}: {k}'
        assert torch.equal(grads[k], again[1][k]), f'{tag}: {k} differs in the second step'
        if not any(pat in k for pat in exceptions):
            assert torch.equal(grads[k], unfrozen[1][k]), \
                f'{tag}: {k} differs from the unfrozen step in {int((grads[k] != unfrozen[1][k]).sum())} of {grads[k].numel()}'
    if oracle is not None:
        on = [k for k, v in flags.items() if v]
        _compare_step(tag, {k: grads[k] for k in on}, {k: oracle[1][k] for k in on}, loss.item(), oracle[0])


def _check_adamw(tag, model, flags, step):
    """(f): one AdamW step after `step()` moves every trainable tensor and leaves every frozen one as it was, to the bit.
    The parameters are put back afterwards (the model is shared by the cases of this module)."""
    before = copy.deepcopy(model.state_dict())
    step()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-2, weight_decay=0.1)
    opt.step()
    after = model.state_dict()
    try:
        for k, on in flags.items():
            same = torch.equal(after[k], before[k])
            assert same != on, f'{tag}: {k} {"did not move" if on else "moved though frozen"}'
    finally:
        model.load_state_dict(before)
        model.zero_grad(set_to_none=True)


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('recipe', FR.VIDEO_RECIPES)
@pytest.mark.parametrize('tower', list(TOWERS))
def test_video_tower_recipe_step(tower, recipe, mode):
    vis, video, cot, oracle, unfrozen = _tower_case(tower)
    m = MODES[mode]
    if mode not in unfrozen:
        FR.apply_recipe(vis, 'none')
        unfrozen[mode] = _tower_step(vis, video, cot, m)
        _compare_step(f'{tower} unfrozen {mode}', unfrozen[mode][1], oracle[1], unfrozen[mode][0].item(), oracle[0])
    flags = FR.apply_recipe(vis, recipe)
    try:
        first, again = _tower_step(vis, video, cot, m), _tower_step(vis, video, cot, m)
        _check_frozen_step(f'{tower} {recipe} {mode}', flags, first, again, unfrozen[mode], oracle)
        _check_adamw(f'{tower} {recipe} {mode}', vis, flags, lambda: _tower_step(vis, video, cot, m))
    finally:
        FR.apply_recipe(vis, 'none')


@pytest.mark.parametrize('recipe', FR.VIDEO_RECIPES)
@pytest.mark.parametrize('tower', list(TOWERS))
def test_video_tower_recipe_step_f32_residual_stream(tower, recipe, monkeypatch):
    """RESIDUAL_F32: the stream and its gradient in float32, the LayerNorm sites on the mixed kernels."""
    from lavila_amd import ops
    monkeypatch.setattr(ops, 'RESIDUAL_F32', True)
    vis, video, cot, oracle, _ = _tower_case(tower)
    FR.apply_recipe(vis, 'none')
    unfrozen = _tower_step(vis, video, cot, False)
    flags = FR.apply_recipe(vis, recipe)
    try:
        first, again = _tower_step(vis, video, cot, False), _tower_step(vis, video, cot, False)
        _check_frozen_step(f'{tower} {recipe} f32 stream', flags, first, again, unfrozen, oracle)
    finally:
        FR.apply_recipe(vis, 'none')


def _dropping_seed(vis):
    """The first seed whose two mask draws (space branch, MLP branch: the only draws of a step) drop some sample and keep some
    sample in each branch."""
    for seed in range(7, 64):
        torch.manual_seed(seed)
        c = torch.stack([vis.blocks[1].drop_path.sample_scale(BATCH, DEV) for _ in range(2)])
        if bool((c == 0).any()) and bool((c != 0).any(1).all()):
            return seed
    raise AssertionError('no seed drops anything')


@pytest.mark.parametrize('mode', ['plain', 'block'])
@pytest.mark.parametrize('recipe', FR.VIDEO_RECIPES)
@pytest.mark.parametrize('tower', ['small_4f', 'tsfb_4f'])
def test_video_tower_recipe_step_with_stochastic_depth(tower, recipe, mode):
    """drop_path_rate 0.5 (block 1 drops its space and its MLP branch per sample), the masks pinned by the seed."""
    vis, video, cot, _, _ = _tower_case(tower, drop_path=0.5)
    assert vis.blocks[1]._stochastic() and not vis.blocks[0]._stochastic()
    m, seed = MODES[mode], _dropping_seed(vis)
    FR.apply_recipe(vis, 'none')
    unfrozen = _tower_step(vis, video, cot, m, seed)
    flags = FR.apply_recipe(vis, recipe)
    try:
        first, again = _tower_step(vis, video, cot, m, seed), _tower_step(vis, video, cot, m, seed)
        _check_frozen_step(f'{tower} {recipe} {mode} drop path', flags, first, again, unfrozen, None)
        _check_adamw(f'{tower} {recipe} {mode} drop path', vis, flags, lambda: _tower_step(vis, video, cot, m, seed))
    finally:
        FR.apply_recipe(vis, 'none')


# ----------------------------------------------------------------------------------------------------------------------------------
# CLIP step: freeze-space tower + frozen logit_scale; SSL loss with freeze_scale
# ----------------------------------------------------------------------------------------------------------------------------------
CLIP_CFG = dict(img=32, patch=16, frames=4, dim=256, depth=2, heads=4, t_width=256, t_heads=4, t_layers=2, vocab=512, embed=256,
                batch=4, gated=False)


def _clip_case():
    if 'clip' not in _cache:
        c = CLIP_CFG
        model = build_model(c)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        w = O.procedural_weights(shapes, seed=23)
        model.load_state_dict(w)
        model.to(DEV).train()
        video, tokens = O.synthetic_batch(c['batch'], c['frames'], c['img'], seed=31)
        tokens = tokens % (c['vocab'] - 2) + 1
        ind = torch.tensor([1, 0, 1, 0])
        wo = {k: (v.double().requires_grad_(True) if v.is_floating_point() else v.clone()) for k, v in w.items()}
        pseudo = torch.tensor(math.log(1 / 0.08), dtype=torch.float64)
        oo = O.clip_forward(video.double(), tokens, wo, c['heads'], c['t_heads'], norm_embed=True)
        lo = O.clip_loss(oo['image_embed'], oo['text_embed'], oo['logit_scale'])['loss']
        lo.backward()
        clip = (lo.item(), {k: v.grad.clone() for k, v in wo.items() if v.requires_grad})
        for v in wo.values():
            v.grad = None
        oo = O.clip_forward(video.double(), tokens, wo, c['heads'], c['t_heads'], norm_embed=True)
        ls = O.ssl_clip_loss(oo['image_embed'], oo['text_embed'], ind, oo['logit_scale'], pseudo.exp())['loss']
        ls.backward()
        ssl = (ls.item(), {k: v.grad.clone() for k, v in wo.items() if v.requires_grad})
        _cache['clip'] = (model, video.to(DEV), tokens.to(DEV), ind.to(DEV), clip, ssl)
    return _cache['clip']


@pytest.mark.parametrize('loss_kind', ['clip', 'ssl'])
def test_clip_step_with_freeze_space_and_frozen_temperatures(loss_kind):
    from lavila.models.loss import CLIPLoss, SSLCLIPLoss
    model, video, tokens, ind, clip_oracle, ssl_oracle = _clip_case()
    oracle = clip_oracle if loss_kind == 'clip' else ssl_oracle

    def make_crit(freeze):
        if loss_kind == 'clip':
            return CLIPLoss()
        return SSLCLIPLoss(freeze_scale=freeze).to(DEV)

    def step(crit):
        model.zero_grad(set_to_none=True)
        crit.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=BF):
            out = model(video, tokens, norm_embed=True)
            loss = (crit(out) if loss_kind == 'clip' else crit(out, ind))['loss']
        loss.backward()
        torch.cuda.synchronize()
        grads = {k: (None if p.grad is None else p.grad.clone()) for k, p in model.named_parameters()}
        grads.update({'crit.' + k: (None if p.grad is None else p.grad.clone()) for k, p in crit.named_parameters()})
        return loss.detach().clone(), grads

    def set_flags(freeze):
        for p in model.parameters():
            p.requires_grad = True
        if freeze:
            FR.apply_freeze_space(model.visual)
            model.logit_scale.requires_grad = False
        return {k: p.requires_grad for k, p in model.named_parameters()}

    try:
        set_flags(False)
        unfrozen = step(make_crit(False))
        assert all(v is not None for v in unfrozen[1].values())
        flags = set_flags(True)
        assert not flags['logit_scale'] and flags['visual.cls_token'] and not flags['visual.blocks.0.attn.qkv.bias']
        crit = make_crit(True)
        flags.update({'crit.' + k: p.requires_grad for k, p in crit.named_parameters()})
        assert loss_kind == 'clip' or flags['crit.logit_scale_pseudo'] is False
        first, again = step(crit), step(crit)
        model_flags = {k: v for k, v in flags.items() if not k.startswith('crit.')}
        for k, on in flags.items():
            if k.startswith('crit.'):
                assert first[1][k] is None and unfrozen[1][k] is not None
        _check_frozen_step(f'CLIP step, freeze space, {loss_kind} loss', model_flags, first, again, unfrozen, oracle)
        _check_adamw(f'CLIP step, freeze space, {loss_kind} loss', model, model_flags, lambda: step(crit))
    finally:
        set_flags(False)


# ----------------------------------------------------------------------------------------------------------------------------------
# narrator
# ----------------------------------------------------------------------------------------------------------------------------------
NARRATOR_RECIPES = [('lm',), ('visual',), ('visual_temporal',), ('lm', 'visual'), ('lm', 'visual', 'visual_temporal')]


def _narrator_flags(m, recipe):
    for p in m.parameters():
        p.requires_grad = True
    with contextlib.redirect_stdout(io.StringIO()):
        if 'lm' in recipe:
            m.text_decoder.freeze_lm_weights()
        if 'visual' in recipe:
            m.visual.freeze_spatial_weights()
        if 'visual_temporal' in recipe:
            m.visual.freeze_temporal_weights()
    return {k: p.requires_grad for k, p in m.named_parameters()}


def _count_calls(monkeypatch, obj, names, counts):
    for name in names:
        def wrap(*a, _f=getattr(obj, name), _n=name, **k):
            counts[_n] = counts.get(_n, 0) + 1
            return _f(*a, **k)
        monkeypatch.setattr(obj, name, wrap)


@pytest.mark.parametrize('packed', [False, True], ids=['padded', 'packed'])
def test_narrator_recipes(packed, monkeypatch):
    from lavila.models.loss import CaptionLoss
    from lavila_amd import _cabi as C
    from lavila_amd import narrator as N
    from lavila_amd import ops
    m, c, d, v, video, tok = _golden_model('freq1_gated')
    text_cpu = v['text'].clone()
    if packed:
        text_cpu[2, 2:] = v['pad']                       # ragged captions, as test_narrator_end_to_end_with_packed_captions
        monkeypatch.setattr(N, 'PACK_CAPTIONS', True)
    text = text_cpu.to(DEV)
    wo = {k: t.double().requires_grad_(True) for k, t in O.narrator_weights(v['shapes'], seed=v['weight_seed']).items()}
    wo['text_decoder.lm_head.weight'] = wo['text_decoder.transformer.wte.weight']
    oo = O.narrator_forward(video.cpu().double(), text_cpu, wo, c['heads'], c['pool_heads'], c['pool_heads'])
    loss_want = _caption_loss64(oo['text_tokens_logits'], oo['labels'], v['pad'])
    loss_want.backward()
    crit = CaptionLoss(tokenizer=tok)
    counts, tower_out = {}, []
    attn_bwd = ('lvl_divided_attn_bwd', 'lvl_divided_attn_bwd_bias', 'lvl_cls_attn_bwd')
    _count_calls(monkeypatch, C.lib(), attn_bwd, counts)
    _count_calls(monkeypatch, ops, ('_wgrad', '_wgrad_f32', 'linear_skinny_raw'), counts)
    features = m.visual._features_from_tokens           # VCLM_HF.encode_image enters the tower here

    def watched(*a, **k):
        tower_out.append(features(*a, **k))
        return tower_out[-1]
    monkeypatch.setattr(m.visual, '_features_from_tokens', watched)

    def step():
        m.zero_grad(set_to_none=True)
        counts.clear()
        tower_out.clear()
        with torch.autocast('cuda', dtype=BF):
            res = crit(m(video, text))
        res['loss'].backward()
        torch.cuda.synchronize()
        return res['loss'].detach().clone(), {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}

    try:
        _narrator_flags(m, ())
        unfrozen = step()
        assert sum(counts.get(k, 0) for k in attn_bwd) == 2 * len(m.visual.blocks) and tower_out[0].requires_grad
        oracle = (loss_want.item(), {k: wo[k].grad for k in unfrozen[1]})
        wgrads, skinny = {}, counts.get('linear_skinny_raw', 0)
        for recipe in NARRATOR_RECIPES:
            tag = f'narrator {"packed" if packed else "padded"} freeze {"+".join(recipe)}'
            flags = _narrator_flags(m, recipe)
            first = step()
            wgrads[recipe] = counts.get('_wgrad', 0) + counts.get('_wgrad_f32', 0)
            exceptions = FR.BITWISE_EXCEPTIONS.get('narrator ' + '+'.join(recipe), {})
            # the routing an exception names is what differs: the tower's Linears leave the library GEMM for ops.linear's
            # inference kernel -- at least the patch embedding and four per block -- exactly when the exception applies. With the
            # spatial part frozen the patch embedding alone does (nothing in front of it wants a gradient), bit-equal results.
            more = counts.get('linear_skinny_raw', 0) - skinny
            want_more = 'visual' in recipe
            assert (more >= 4 * len(m.visual.blocks) + 1) if exceptions else (more == int(want_more)), (tag, counts, skinny)
            if set(recipe) >= {'visual', 'visual_temporal'}:
                # (d) the tower is fully frozen: its output is no part of the graph, no attention backward runs, and the
                # weight-gradient GEMMs are those of the {lm, visual} step minus the ones that step still ran in the tower
                assert not any(flags[k] for k in flags if k.startswith('visual.'))
                assert not tower_out[0].requires_grad and tower_out[0].grad_fn is None
                assert sum(counts.get(k, 0) for k in attn_bwd) == 0, counts
                tower_trained = sum(1 for k, on in _narrator_flags(m, ('lm', 'visual')).items()
                                    if on and k.startswith('visual.') and k.endswith('.weight') and 'norm' not in k)
                assert tower_trained == 2 * len(m.visual.blocks)            # timeattn.qkv and timeattn.proj
                assert wgrads[recipe] == wgrads[('lm', 'visual')] - tower_trained, (wgrads, tower_trained)
                flags = _narrator_flags(m, recipe)
            else:
                assert sum(counts.get(k, 0) for k in attn_bwd) == 2 * len(m.visual.blocks), counts
            again = step()
            _check_frozen_step(tag, flags, first, again, unfrozen, oracle, exceptions)
            _check_adamw(tag, m, flags, step)
        assert set(FR.BITWISE_EXCEPTIONS) == {'narrator lm+visual+visual_temporal'}
    finally:
        _narrator_flags(m, ())
