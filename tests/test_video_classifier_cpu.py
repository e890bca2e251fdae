"""CPU: the classification fine-tune's model classes (`VideoClassifier`, `VideoClassifierMultiHead`; reference
models.py:24-72) against tests/golden/video_classifier.pt, which tools/gen_classifier_golden.py wrote from the unmodified
reference, and the float64 restatement of a tower WITH stochastic depth that the GPU tests compare the kernels with.

The restatement (block_restated / tower_restated / classifier_restated) is built from oracle.oracle's functions; the per-sample
factors c = keep_mask / keep_probability of every dropping site are arguments. It is pinned here against the reference's own
logits, loss and gradients under the masks the reference drew (recovered by the generator through forward hooks)."""
import inspect

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import load_golden
from helpers import check_fixture_gradients
from oracle import oracle as O


# ---- the restatement ------------------------------------------------------------------------------------------------------
def block_restated(x, w, prefix, heads, frames, n, c_space=None, c_mlp=None, eps=1e-6):
    """oracle.space_time_block with stochastic depth (timesformer.py:183-196): the space branch and the MLP branch are
    multiplied by one factor per sample (timm's DropPath: mask / keep); the time branch carries none."""
    p = prefix
    t_out = O.var_attention(O.layer_norm(x, w[p + 'norm3.weight'], w[p + 'norm3.bias'], eps), w, p + 'timeattn.', heads,
                            frames, n, 'time')
    if p + 'alpha_timeattn' in w:
        t_out = torch.tanh(w[p + 'alpha_timeattn']) * t_out
    s_out = O.var_attention(O.layer_norm(x + t_out, w[p + 'norm1.weight'], w[p + 'norm1.bias'], eps), w, p + 'attn.', heads,
                            frames, n, 'space')
    if c_space is not None:
        s_out = s_out * c_space.to(s_out.dtype).view(-1, 1, 1)
    x1 = x + s_out
    h = O.quick_gelu(F.linear(O.layer_norm(x1, w[p + 'norm2.weight'], w[p + 'norm2.bias'], eps), w[p + 'mlp.fc1.weight'],
                              w[p + 'mlp.fc1.bias']))
    m = F.linear(h, w[p + 'mlp.fc2.weight'], w[p + 'mlp.fc2.bias'])
    if c_mlp is not None:
        m = m * c_mlp.to(m.dtype).view(-1, 1, 1)
    return x1 + m


def tower_restated(video_bcthw, w, heads, scales, prefix='visual.', cls_at_last=True):
    """oracle.vision_tower with stochastic depth. scales: {block index: (c_space, c_mlp)}; blocks not listed drop nothing."""
    p = prefix
    B, C, Fr, H, W = video_bcthw.shape
    pw = w[p + 'patch_embed.proj.weight']
    P = pw.shape[-1]
    N = (H // P) * (W // P)
    depth = 1 + max(int(k[len(p) + 7:].split('.')[0]) for k in w if k.startswith(p + 'blocks.'))
    x = O.patch_embed(video_bcthw, pw, w.get(p + 'patch_embed.proj.bias'))
    x = torch.cat([w[p + 'cls_token'].expand(B, -1, -1), x], 1)
    x = x + O.total_pos_embed(w[p + 'pos_embed'], w[p + 'temporal_embed'], N, Fr)
    if p + 'ln_pre.weight' in w:
        x = O.layer_norm(x, w[p + 'ln_pre.weight'], w[p + 'ln_pre.bias'], 1e-5)
    for i in range(depth):
        x = block_restated(x, w, f'{p}blocks.{i}.', heads, Fr, N, *scales.get(i, (None, None)))
    x = O.layer_norm(x, w[p + 'norm.weight'], w[p + 'norm.bias'], 1e-6)
    return x[:, 0] if cls_at_last else x


def classifier_restated(video_bcthw, w, heads, scales, head_prefixes):
    """[fc(features) for every head]; head_prefixes: ('fc_cls.',) or ('fc_cls.0.', 'fc_cls.1.', ...)."""
    feat = tower_restated(video_bcthw, w, heads, scales)
    return [F.linear(feat, w[h + 'weight'], w[h + 'bias']) for h in head_prefixes]


def driver_loss(logits, targets, label_smoothing):
    """main_finetune_classification.py:333-343: the sum of one label-smoothed cross-entropy per head."""
    return sum(F.cross_entropy(lg, t, label_smoothing=label_smoothing) for lg, t in zip(logits, targets))


# ---- the fixture's procedural data ----------------------------------------------------------------------------------------
def fixture_inputs(fx):
    """The clip and the targets as the generator drew them (torch.manual_seed(seed), clip first)."""
    c = fx['config']
    state = torch.random.get_rng_state()
    torch.manual_seed(fx['input_seed'])
    video = torch.randn(c['batch'], 3, c['frames'], c['img'], c['img'])
    targets = [torch.randint(0, n, (c['batch'],)) for n in c['classes_multi']]
    torch.random.set_rng_state(state)
    return video, targets


def fixture_scales(fx, dtype=torch.float64, device='cpu'):
    """{block index: (c_space, c_mlp)} from the keep masks of the fixture and the tower's linspace of rates."""
    c = fx['config']
    rates = [r.item() for r in torch.linspace(0, c['drop_path_rate'], c['depth'])]
    out = {}
    for name, site in fx['multi']['masks'].items():
        i = int(name.split('.')[1])
        out[i] = tuple((site[k].to(dtype) / (1.0 - rates[i])).to(device) for k in ('space', 'mlp'))
    return out


def build_classifier(fx, multi, dropout=0.0, drop_path_rate=None):
    import contextlib
    import io
    from lavila.models import models
    from lavila.models.openai_model import QuickGELU
    from lavila.models.timesformer import SpaceTimeTransformer
    c = fx['config']
    with contextlib.redirect_stdout(io.StringIO()):
        vis = SpaceTimeTransformer(
            img_size=c['img'], patch_size=c['patch'], embed_dim=c['dim'], depth=c['depth'], num_heads=c['heads'],
            num_frames=c['frames'], time_init='rand', attention_style='frozen-in-time', ln_pre=True, act_layer=QuickGELU,
            num_classes=0, drop_path_rate=c['drop_path_rate'] if drop_path_rate is None else drop_path_rate)
    if multi:
        model = models.VideoClassifierMultiHead(vis, dropout=dropout, num_classes_list=list(c['classes_multi']))
        shapes = fx['multi']['shapes']
    else:
        model = models.VideoClassifier(vis, dropout=dropout, num_classes=c['classes_single'])
        shapes = fx['single']['shapes']
    model.load_state_dict(O.procedural_weights(shapes, seed=fx['weight_seed']), strict=True)
    return model


def inject_masks(monkeypatch, model, scales):
    """Replaces DropPath.sample_scale of every dropping block by the fixture's factors: space branch first, then the MLP
    branch, again from the start when a block is re-run (activation checkpointing)."""
    calls = []
    for i, blk in enumerate(model.visual.blocks if hasattr(model, 'visual') else model.blocks):
        if i not in scales:
            continue

        def sample(batch, device, _pair=scales[i], _n=[0], _i=i):
            c = _pair[_n[0] % 2]
            _n[0] += 1
            calls.append(_i)
            assert c.numel() == batch
            return c.to(device=device, dtype=torch.float32)
        monkeypatch.setattr(blk.drop_path, 'sample_scale', sample)
    return calls


# ---- tests ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fx():
    return load_golden('video_classifier.pt')


def test_class_names_signatures_and_state_dict(fx):
    from lavila.models import models
    import lavila_amd.models as impl
    assert models.VideoClassifier is impl.VideoClassifier and models.VideoClassifierMultiHead is impl.VideoClassifierMultiHead
    for name, multi in (('VideoClassifier', False), ('VideoClassifierMultiHead', True)):
        cls = getattr(models, name)
        assert cls.__name__ == name
        assert str(inspect.signature(cls.__init__)) == fx['signatures'][name]['init']
        assert str(inspect.signature(cls.forward)) == fx['signatures'][name]['forward']
        got = [(k, tuple(v.shape)) for k, v in build_classifier(fx, multi).state_dict().items()]
        assert got == [(k, tuple(s)) for k, s in fx['state_dict'][name]]


class _Tower(nn.Module):
    num_features = 768


def test_head_init_and_kwargs():
    from lavila.models import models
    torch.manual_seed(0)
    m = models.VideoClassifierMultiHead(_Tower(), dropout=0.5, num_classes_list=[97, 300, 3806], some_unknown_option=3)
    assert isinstance(m.fc_cls, nn.ModuleList) and [h.out_features for h in m.fc_cls] == [97, 300, 3806]
    big = m.fc_cls[2]
    assert tuple(big.weight.shape) == (3806, 768)
    assert abs(big.weight.std().item() - 0.01) <= 0.1 * 0.01 and abs(big.weight.mean().item()) < 1e-4
    assert all(bool((h.bias == 0).all()) for h in m.fc_cls)
    assert isinstance(m.dropout, nn.Dropout) and m.dropout.p == 0.5
    s = models.VideoClassifier(_Tower(), dropout=0.1, num_classes=3806, another_option=None)
    assert abs(s.fc_cls.weight.std().item() - 0.01) <= 0.1 * 0.01 and bool((s.fc_cls.bias == 0).all())
    assert s.visual is not None and s.dropout.p == 0.1


def test_cpu_tensors_raise(fx):
    from lavila_amd._cabi import HipExtensionError
    video, _ = fixture_inputs(fx)
    for multi in (False, True):
        model = build_classifier(fx, multi).eval()
        with pytest.raises(HipExtensionError):
            model(video)


def test_multi_head_returns_a_list_of_the_right_shapes(fx, monkeypatch):
    """The forward's plumbing with the tower replaced by a stand-in (no kernels on this machine): a list for the multi-head
    class, one tensor for the single head -- through the module's own head function on a float32 CPU feature tensor."""
    import lavila_amd.models as impl
    c = fx['config']
    feats = torch.randn(c['batch'], c['dim'])
    monkeypatch.setattr(impl, '_features', lambda visual, image, use_checkpoint: feats)
    monkeypatch.setattr(impl, '_classifier_head', lambda x, fc: F.linear(x, fc.weight, fc.bias))
    out = build_classifier(fx, True).eval()(torch.zeros(1))
    assert isinstance(out, list) and [tuple(o.shape) for o in out] == [(c['batch'], n) for n in c['classes_multi']]
    one = build_classifier(fx, False).eval()(torch.zeros(1), use_checkpoint=True)
    assert torch.is_tensor(one) and tuple(one.shape) == (c['batch'], c['classes_single'])


def test_restatement_reproduces_the_eval_logits(fx):
    video, _ = fixture_inputs(fx)
    w = {k: v.double() for k, v in O.procedural_weights(fx['single']['shapes'], seed=fx['weight_seed']).items()}
    (logits,) = classifier_restated(video.double(), w, fx['config']['heads'], {}, ('fc_cls.',))
    err = (logits - fx['single']['logits'].double()).abs().max().item()
    print(f'[classifier restatement] eval logits: max |d| {err:.2e}')
    assert err <= 1e-3


def test_restatement_reproduces_the_training_step(fx):
    c = fx['config']
    video, targets = fixture_inputs(fx)
    assert all(torch.equal(a, b) for a, b in zip(targets, fx['multi']['targets']))
    w = {k: v.double().requires_grad_(True)
         for k, v in O.procedural_weights(fx['multi']['shapes'], seed=fx['weight_seed']).items()}
    heads = tuple(f'fc_cls.{i}.' for i in range(len(c['classes_multi'])))
    logits = classifier_restated(video.double(), w, c['heads'], fixture_scales(fx), heads)
    for got, want in zip(logits, fx['multi']['logits']):
        assert (got - want.double()).abs().max().item() <= 1e-3
    loss = driver_loss(logits, targets, c['label_smoothing'])
    assert abs(loss.item() - fx['multi']['loss']) <= 1e-3
    loss.backward()
    worst = check_fixture_gradients(fx['multi'], {k: v.grad for k, v in w.items()}, rtol=1e-3, norm_rtol=2e-3)
    print(f'[classifier restatement] training step: loss {loss.item():.6f} (reference {fx["multi"]["loss"]:.6f}), worst '
          f'gradient distance {worst:.2e}')
    # the masks matter: without them the logits leave the bar by orders of magnitude
    plain = classifier_restated(video.double(), {k: v.detach() for k, v in w.items()}, c['heads'], {}, heads)
    assert max((a - b.double()).abs().max().item() for a, b in zip(plain, fx['multi']['logits'])) > 1e-2


def test_sample_scale_values_and_seed():
    from lavila.models.timesformer import DropPath
    dp = DropPath(0.25)
    torch.manual_seed(5)
    a = dp.sample_scale(4096, 'cpu')
    torch.manual_seed(5)
    b = dp.sample_scale(4096, 'cpu')
    assert a.dtype == torch.float32 and tuple(a.shape) == (4096,) and torch.equal(a, b)
    keep = 0.75
    assert bool(((a == 0) | (a == 1 / keep)).all())
    assert abs((a != 0).float().mean().item() - keep) < 0.03
    # standalone use keeps timm's semantics
    dp.train()
    x = torch.ones(64, 3, 2)
    yv = dp(x)
    per = yv.reshape(64, -1)
    assert bool(((per == 0).all(1) | (per == 1 / keep).all(1)).all())
    assert dp.eval()(x) is x
