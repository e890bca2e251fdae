"""GPU (-m gpu): stochastic depth on the fused residual chain (SpaceTimeBlock.chain / chain_cls with drop_path > 0 in training)
and the classification fine-tune's models (VideoClassifier, VideoClassifierMultiHead).

Masks are injected by replacing DropPath.sample_scale (the one place the chain draws a mask); the float64 reference is the
restatement of tests/test_video_classifier_cpu.py, which that file pins to the unmodified reference's logits, loss and
gradients (tests/golden/video_classifier.pt). Bars: one bf16 block against float64 at relative L2 2e-2
(test_gated_and_drop_path_blocks_stay_on_own_gemms); gradients by _compare_step of test_gpu_narrator_train.py (per tensor
1e-1 unless the tensor is below 1e-3 of the scale, aggregate 5e-2); float32 against the fixture at 1e-3 and
check_fixture_gradients' GPU rtol 2e-3."""
import contextlib
import io
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from helpers import check_fixture_gradients
from oracle import oracle as O
from lavila_amd.guards import forbid_library_gemm
from test_gpu_narrator_train import _compare_step
from test_video_classifier_cpu import (block_restated, build_classifier, classifier_restated, driver_loss, fixture_inputs,
                                       fixture_scales, inject_masks, tower_restated)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF = torch.bfloat16
D, HEADS, FR, N, B = 256, 4, 2, 16, 5
ARGS = ('b (f n) d', '(b f) n d', 'b (f n) d', '(b n) f d')
SPACE = torch.tensor([1., 0., 1., 0., 1.])
MLP = torch.tensor([1., 1., 0., 0., 1.])


def _rel(got, want):
    return ((got.double().cpu() - want.double().cpu()).norm() / want.double().norm()).item()


def _block(gated, seed=0):
    from lavila.models.openai_model import QuickGELU
    from lavila.models.timesformer import SpaceTimeBlock
    blk = SpaceTimeBlock(D, HEADS, qkv_bias=True, act_layer=QuickGELU, time_init='rand', is_tanh_gating=gated, drop_path=0.5)
    w = O.procedural_weights({k: tuple(v.shape) for k, v in blk.state_dict().items()}, seed=seed)
    if gated:
        w['alpha_timeattn'] = torch.tensor(0.3)
    blk.load_state_dict(w, strict=True)
    return blk.to(DEV).train(), w


def _fixed(monkeypatch, drop_path, pair):
    """drop_path.sample_scale returns pair[0], pair[1], pair[0], ... (space branch, MLP branch)."""
    n = [0]

    def sample(batch, device):
        c = pair[n[0] % 2]
        n[0] += 1
        return c.to(device=device, dtype=torch.float32)
    monkeypatch.setattr(drop_path, 'sample_scale', sample)
    return n


@pytest.mark.parametrize('gated', [False, True], ids=['plain', 'tanh_gated'])
def test_one_block_with_injected_masks(gated, monkeypatch):
    from lavila_amd import ops
    from lavila.models.timesformer import DropPath
    blk, w = _block(gated)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 1 + FR * N, D, generator=g).to(BF)
    up = (torch.randn(B, 1 + FR * N, D, generator=g) / 256).to(BF)
    c_s, c_m = SPACE / 0.5, MLP / 0.5
    draws = _fixed(monkeypatch, blk.drop_path, (c_s, c_m))

    def boom(*a, **k):
        raise AssertionError('a stochastic-depth block left the fused chain')
    calls = []
    real = ops.scaled_add_layer_norm
    monkeypatch.setattr(ops, 'bias_quick_gelu', boom)
    monkeypatch.setattr(DropPath, 'forward', boom)
    monkeypatch.setattr(F, 'linear', boom)
    monkeypatch.setattr(ops, 'scaled_add_layer_norm', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    xd = x.to(DEV).requires_grad_(True)
    with torch.autocast('cuda', dtype=BF):
        y = blk(xd, *ARGS, time_n=N, space_f=FR)
    loss = (y.float() * up.to(DEV).float()).sum()
    loss.backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert len(calls) == 2 and draws[0] == 2
    # sample 3 is dropped at both sites: the block is the identity on it, forward and backward
    assert torch.equal(y[3], xd.detach()[3])
    assert torch.equal(xd.grad[3], up.to(DEV)[3])
    assert not torch.equal(y[1], xd.detach()[1]) and not torch.equal(y[2], xd.detach()[2])
    w64 = {k: v.double().requires_grad_(True) for k, v in w.items()}
    x64 = x.double().requires_grad_(True)
    y64 = block_restated(x64, w64, '', HEADS, FR, N, c_s.double(), c_m.double())
    loss64 = (y64 * up.double()).sum()
    loss64.backward()
    rel = _rel(y, y64.detach())
    print(f'[drop-path block gated={gated}] output relative L2 {rel:.2e}')
    assert rel < 2e-2, rel
    got = {k: p.grad for k, p in blk.named_parameters()}
    got['input'] = xd.grad
    want = {k: v.grad for k, v in w64.items()}
    want['input'] = x64.grad
    _compare_step(f'drop-path block gated={gated}', got, want, loss.item(), loss64.item())


# ---- three-block tower -----------------------------------------------------------------------------------------------------
def _tower(rate, seed=3):
    from lavila.models.openai_model import QuickGELU
    from lavila.models.timesformer import SpaceTimeTransformer
    with contextlib.redirect_stdout(io.StringIO()):
        vis = SpaceTimeTransformer(img_size=64, patch_size=16, embed_dim=D, depth=3, num_heads=HEADS, num_frames=FR,
                                   time_init='rand', attention_style='frozen-in-time', ln_pre=True, act_layer=QuickGELU,
                                   num_classes=0, drop_path_rate=rate)
    w = O.procedural_weights({k: tuple(v.shape) for k, v in vis.state_dict().items()}, seed=seed)
    vis.load_state_dict(w, strict=True)
    return vis.to(DEV).train(), w


def _video(seed=4):
    return torch.randn(B, 3, FR, 64, 64, generator=torch.Generator().manual_seed(seed))


TOWER_SCALES = {1: (torch.tensor([1., 1., 0., 1., 0.]) / 0.75, torch.tensor([0., 1., 1., 1., 1.]) / 0.75),
                2: (SPACE / 0.5, MLP / 0.5)}


def _tower_step(vis, video, up, use_checkpoint=False, scales=None, monkeypatch=None):
    vis.zero_grad(set_to_none=True)
    if scales is not None:
        for i, pair in scales.items():
            _fixed(monkeypatch, vis.blocks[i].drop_path, pair)
    with torch.autocast('cuda', dtype=BF):
        feat = vis(video.to(DEV), use_checkpoint=use_checkpoint)
    loss = (feat.float() * up.to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return feat.detach(), loss.item(), {k: p.grad.detach().clone() for k, p in vis.named_parameters()}


def _aggregate(got, want):
    num = sum((got[k].double() - want[k].double()).norm().item() ** 2 for k in want)
    return math.sqrt(num / sum(want[k].double().norm().item() ** 2 for k in want))


def test_tower_takes_the_cls_path_and_matches_the_full_last_block(monkeypatch):
    import lavila_amd.timesformer as T
    vis, w = _tower(0.5)
    video = _video()
    up = torch.randn(B, D, generator=torch.Generator().manual_seed(6)) / 128
    taken = []
    real = T.SpaceTimeBlock.chain_cls
    monkeypatch.setattr(T.SpaceTimeBlock, 'chain_cls', lambda self, *a, **k: (taken.append(self), real(self, *a, **k))[1])
    feat, loss, grads = _tower_step(vis, video, up, scales=TOWER_SCALES, monkeypatch=monkeypatch)
    assert taken == [vis.blocks[2]]
    monkeypatch.setattr(T, 'CLS_ONLY_LAST_BLOCK', False)
    feat_full, loss_full, grads_full = _tower_step(vis, video, up, scales=TOWER_SCALES, monkeypatch=monkeypatch)
    assert len(taken) == 1
    rel, agg = _rel(feat, feat_full), _aggregate(grads, grads_full)
    print(f'[drop-path tower] cls-only last block against the full one: features {rel:.2e}, gradients (aggregate) {agg:.2e}')
    assert rel < 2e-2 and agg <= 5e-2
    # and both against float64 with the same masks
    w64 = {'visual.' + k: v.double().requires_grad_(True) for k, v in w.items()}
    f64 = tower_restated(video.double(), w64, HEADS, {i: tuple(c.double() for c in p) for i, p in TOWER_SCALES.items()})
    loss64 = (f64 * up.double()).sum()
    loss64.backward()
    assert _rel(feat, f64.detach()) < 3 * 2e-2               # three blocks at the one-block bar each
    _compare_step('drop-path tower', {'visual.' + k: v for k, v in grads.items()}, {k: v.grad for k, v in w64.items()},
                  loss, loss64.item())


def test_tower_checkpoint_modes():
    """Block checkpointing re-runs the same kernels with the same masks (the RNG state is restored for the recomputation):
    equal to the plain step to the bit under one seed. 'selective' keeps everything in the dropping blocks and rebuilds
    activations in the others: same criterion as against float64."""
    vis, _ = _tower(0.5)
    video = _video()
    up = torch.randn(B, D, generator=torch.Generator().manual_seed(6)) / 128
    torch.manual_seed(21)
    feat, loss, grads = _tower_step(vis, video, up)
    torch.manual_seed(21)
    feat_c, loss_c, grads_c = _tower_step(vis, video, up, use_checkpoint=True)
    assert loss == loss_c and torch.equal(feat, feat_c)
    for k in grads:
        assert torch.equal(grads[k], grads_c[k]), k
    torch.manual_seed(21)
    feat_s, loss_s, grads_s = _tower_step(vis, video, up, use_checkpoint='selective')
    rel, agg = _rel(feat_s, feat), _aggregate(grads_s, grads)
    print(f'[drop-path tower] selective against plain: features {rel:.2e}, gradients (aggregate) {agg:.2e}')
    assert rel < 2e-2 and agg <= 5e-2
    torch.manual_seed(22)
    assert not torch.equal(_tower_step(vis, video, up)[0], feat)          # another seed, other masks


def test_non_dropping_path_is_untouched(monkeypatch):
    """A tower with drop_path_rate = 0, and a dropping tower in eval mode, never reach the new op, and compute the same
    bits as each other -- whole towers and block by block through the reference-signature forward (the guard that the
    non-dropping path did not move: what differs between the two towers is only the presence of DropPath modules)."""
    from lavila_amd import ops
    dropping, w = _tower(0.5)
    plain, _ = _tower(0.0)
    video = _video().to(DEV)

    def boom(*a, **k):
        raise AssertionError('the non-dropping path reached the stochastic-depth op')
    monkeypatch.setattr(ops, 'scaled_add_layer_norm', boom)
    x = torch.randn(B, 1 + FR * N, D, generator=torch.Generator().manual_seed(8)).to(BF).to(DEV)
    with torch.autocast('cuda', dtype=BF):
        want = plain(video)                                   # training mode, rate 0
        assert torch.equal(plain.eval()(video), want)
        assert torch.equal(dropping.eval()(video), want)
        for a, b in zip(dropping.blocks, plain.blocks):
            assert torch.equal(a(x, *ARGS, time_n=N, space_f=FR), b(x, *ARGS, time_n=N, space_f=FR))
        with torch.no_grad():
            assert torch.equal(dropping(video), plain(video))


# ---- golden parity --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fx():
    return load_golden('video_classifier.pt')


def test_golden_eval_logits_float32(fx):
    model = build_classifier(fx, multi=False).to(DEV).eval()
    video, _ = fixture_inputs(fx)
    with torch.no_grad():
        logits = model(video.to(DEV))
    want = fx['single']['logits']
    d, rel = (logits.cpu() - want).abs().max().item(), _rel(logits, want)
    print(f'[classifier golden] eval logits: max |d| {d:.2e}, relative L2 {rel:.2e}')
    assert logits.dtype == torch.float32 and d <= 1e-3 and rel <= 1e-3


def test_golden_training_step_float32(fx, monkeypatch):
    c = fx['config']
    model = build_classifier(fx, multi=True).to(DEV).train()
    calls = inject_masks(monkeypatch, model, fixture_scales(fx, torch.float32))
    video, targets = fixture_inputs(fx)
    logits = model(video.to(DEV))
    assert isinstance(logits, list) and calls == [1, 1, 2, 2]
    crit = torch.nn.CrossEntropyLoss(label_smoothing=c['label_smoothing'])
    loss = sum(crit(lg, t.to(DEV)) for lg, t in zip(logits, targets))
    loss.backward()
    for got, want in zip(logits, fx['multi']['logits']):
        assert (got.detach().cpu() - want).abs().max().item() <= 1e-3
    assert abs(loss.item() - fx['multi']['loss']) <= 1e-3
    worst = check_fixture_gradients(fx['multi'], {k: p.grad for k, p in model.named_parameters()}, rtol=2e-3, norm_rtol=5e-3)
    print(f'[classifier golden] float32 step: |d loss| {abs(loss.item() - fx["multi"]["loss"]):.2e}, worst gradient tensor '
          f'(own scale) {worst:.2e}')


def test_golden_training_step_bf16(fx, monkeypatch):
    c = fx['config']
    model = build_classifier(fx, multi=True).to(DEV).train()
    inject_masks(monkeypatch, model, fixture_scales(fx, torch.float32))
    video, targets = fixture_inputs(fx)
    with torch.autocast('cuda', dtype=BF):
        logits = model(video.to(DEV))
        loss = sum(F.cross_entropy(lg.float(), t.to(DEV), label_smoothing=c['label_smoothing'])
                   for lg, t in zip(logits, targets))
    loss.backward()
    w64 = {k: v.double().requires_grad_(True)
           for k, v in O.procedural_weights(fx['multi']['shapes'], seed=fx['weight_seed']).items()}
    heads = tuple(f'fc_cls.{i}.' for i in range(len(c['classes_multi'])))
    loss64 = driver_loss(classifier_restated(video.double(), w64, c['heads'], fixture_scales(fx), heads), targets,
                         c['label_smoothing'])
    loss64.backward()
    _compare_step('classifier golden bf16', {k: p.grad for k, p in model.named_parameters()},
                  {k: v.grad for k, v in w64.items()}, loss.item(), loss64.item())


# ---- heads ----------------------------------------------------------------------------------------------------------------
def test_every_head_draws_its_own_dropout_mask():
    """models.py:71: `[m(self.dropout(image_embed)) for m in self.fc_cls]` -- one draw per head, in head order."""
    from lavila.models import models
    import lavila_amd.models as impl
    vis, _ = _tower(0.0)
    model = models.VideoClassifierMultiHead(vis, dropout=0.5, num_classes_list=[7, 11, 13]).to(DEV)
    with torch.no_grad():
        for m in model.fc_cls:
            m.weight.normal_(0, 0.1)
            m.bias.normal_(0, 0.1)
    video = _video().to(DEV)
    with torch.autocast('cuda', dtype=BF):
        torch.manual_seed(31)
        got = model.train()(video)
        feat = model.eval().visual(video)                    # gradients enabled: the kernels of the training forward
        torch.manual_seed(31)
        want = [impl._classifier_head(F.dropout(feat, 0.5, True), m) for m in model.fc_cls]
        once = F.dropout(feat, 0.5, True)
    for a, b in zip(got, want):
        assert a.dtype == BF and torch.equal(a, b)
    assert not torch.equal(got[1], impl._classifier_head(once, model.fc_cls[1]))


def test_ek100_heads_run_on_own_gemms():
    """The class counts of EK-100 (97 verbs, 300 nouns, 3806 actions) on a width-768 tower: forward and backward without
    a library GEMM; the zero class rows of the padded GEMM operands leak into nothing."""
    from lavila.models import models
    from lavila.models.openai_model import QuickGELU
    from lavila.models.timesformer import SpaceTimeTransformer
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        vis = SpaceTimeTransformer(img_size=32, patch_size=16, embed_dim=768, depth=1, num_heads=12, num_frames=2,
                                   time_init='rand', attention_style='frozen-in-time', ln_pre=True, act_layer=QuickGELU,
                                   num_classes=0, drop_path_rate=0.0)
    vis.load_state_dict(O.procedural_weights({k: tuple(v.shape) for k, v in vis.state_dict().items()}, seed=5))
    classes = [97, 300, 3806]
    model = models.VideoClassifierMultiHead(vis, dropout=0.0, num_classes_list=classes).to(DEV).train()
    with torch.no_grad():
        for m in model.fc_cls:
            m.weight.normal_(0, 0.05)
            m.bias.normal_(0, 0.05)
    g = torch.Generator().manual_seed(2)
    video = torch.randn(4, 3, 2, 32, 32, generator=g).to(DEV)
    targets = [torch.randint(0, n, (4,), generator=g).to(DEV) for n in classes]
    feats = []
    model.visual.register_forward_hook(lambda mod, args, out: feats.append(out.detach()))
    with forbid_library_gemm():
        with torch.autocast('cuda', dtype=BF):
            logits = model(video)
            loss = sum(F.cross_entropy(lg.float(), t, label_smoothing=0.1) for lg, t in zip(logits, targets))
        loss.backward()
    torch.cuda.synchronize()
    assert [tuple(lg.shape) for lg in logits] == [(4, n) for n in classes]
    f64 = feats[0].double().cpu()
    for i, (m, t) in enumerate(zip(model.fc_cls, targets)):
        assert m.weight.grad.shape == m.weight.shape and m.bias.grad.shape == m.bias.shape
        w64 = m.weight.detach().double().cpu().requires_grad_(True)
        b64 = m.bias.detach().double().cpu().requires_grad_(True)
        lg64 = F.linear(f64, w64, b64)
        F.cross_entropy(lg64, t.cpu(), label_smoothing=0.1).backward()
        rl, rw, rb = _rel(logits[i], lg64.detach()), _rel(m.weight.grad, w64.grad), _rel(m.bias.grad, b64.grad)
        print(f'[classifier heads] {classes[i]} classes: logits {rl:.2e}, d weight {rw:.2e}, d bias {rb:.2e} (relative L2)')
        assert rl <= 2.0 ** -7 and rw <= 2.0 ** -7 and rb <= 2.0 ** -7
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


def test_half_model_returns_half(fx):
    """model.half() with fp16 clips (the --use-half recipes): fp16 logits, computed in bf16."""
    video, _ = fixture_inputs(fx)
    video = video.to(DEV).half()
    for multi in (False, True):
        model = build_classifier(fx, multi).to(DEV).half().eval()
        with torch.no_grad():
            out = model(video)
        for lg in (out if multi else [out]):
            assert lg.dtype == torch.float16 and bool(torch.isfinite(lg).all())
        if not multi:
            rel = _rel(out, fx['single']['logits'])
            print(f'[classifier half] logits against the float32 reference: relative L2 {rel:.2e}')
            assert rel < 3 * 2e-2                       # three bf16 blocks at the one-block bar each
