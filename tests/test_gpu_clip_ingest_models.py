"""The model entry points on an ingest.PendingClip (uint8 frames + crop blocks, turned into the patch matrix by one kernel)
against the same entry points on the float32 clip ClipIngest materialises: equal to the bit, in float32, under bf16
autocast and with use_checkpoint=True; one bf16 training step; the refusals. Tiny towers: 32 px / 16-pixel patches, and
28 px / 14-pixel patches at width 256, where the patch rows are written 640 wide and conv_patch_tokens skips its pad."""
import contextlib
import io

import pytest
import torch

import clip_hf_helpers as H
from conftest import load_golden
from helpers import build_model

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SRC_H, SRC_W = 37, 53

P16 = dict(img=32, patch=16, dim=128, depth=2, heads=2, frames=2, gated=False, embed=64, vocab=64, t_width=128, t_heads=2,
           t_layers=2)
P14 = dict(P16, img=28, patch=14, dim=256, heads=4, gated=True)          # 588 -> 640 columns (width % 256 == 0)
CONFIGS = {'p16': P16, 'p14_wide': P14}
MODES = [('f32', False, False), ('f32_ckpt', False, True), ('bf16', True, False), ('bf16_ckpt', True, True)]


def _source(S, B, Fr, seed=0):
    """(ClipIngest, device frames, host blocks, flips): a different RandomResizedCrop block and flip per clip"""
    from lavila_amd.ingest import OPENAI_MEAN_STD, ClipIngest, random_resized_crop_params
    g = torch.Generator().manual_seed(100 + seed)
    frames = torch.randint(0, 256, (B, Fr, SRC_H, SRC_W, 3), dtype=torch.uint8, generator=g)
    params = random_resized_crop_params(B, SRC_H, SRC_W, S, generator=g)
    flip = torch.arange(B) % 2
    return ClipIngest(S, *OPENAI_MEAN_STD), frames.to(DEV), params, flip


def _tokens(B, vocab, L=12, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(1, vocab - 1, (B, L), generator=g)
    for b in range(B):
        t[b, L - 1 - b] = vocab - 1          # EOT = the highest id, ragged lengths
        t[b, L - b:] = 0
    return t.to(DEV)


def _same(a, b, what):
    if isinstance(a, dict):
        assert set(a) == set(b)
        for k in a:
            _same(a[k], b[k], f'{what}[{k}]')
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f'{what}[{i}]')
    else:
        assert a.dtype == b.dtype and a.shape == b.shape, what
        a, b = a.detach(), b.detach()
        assert bool(a.isfinite().all()) and float(a.float().abs().max()) > 0, f'{what}: nothing to compare'
        assert torch.equal(a, b), f'{what}: max |d| {(a.float() - b.float()).abs().max().item():.3e}'


def _check(calls, S, B, Fr, mode):
    """calls: name -> f(x, use_checkpoint). Each on the float32 clip and on the PendingClip."""
    _, amp, ckpt = mode
    ci, frames, params, flip = _source(S, B, Fr)
    clip = ci(frames, params, flip)
    assert clip.dtype == torch.float32 and tuple(clip.shape) == (B, 3, Fr, S, S)
    for name, f in calls.items():
        with torch.autocast('cuda', dtype=torch.bfloat16) if amp else contextlib.nullcontext():
            want = f(clip, ckpt)
            pend = ci.pending(frames, params, flip)
            got = f(pend, ckpt)
        _same(got, want, name)


def _seeded(build):
    torch.manual_seed(1234)
    with contextlib.redirect_stdout(io.StringIO()):
        m = build()
    return m.to(DEV).train()


@pytest.fixture(scope='module', params=sorted(CONFIGS))
def clip_model(request):
    c = CONFIGS[request.param]
    return c, _seeded(lambda: build_model(c))


@pytest.mark.parametrize('mode', MODES, ids=[m[0] for m in MODES])
def test_clip_and_its_video_tower(clip_model, mode):
    c, model = clip_model
    tok = _tokens(3, c['vocab'])
    _check({'CLIP.encode_image': lambda x, k: model.encode_image(x, use_checkpoint=k),
            'CLIP.encode_image(no projection)': lambda x, k: model.encode_image(x, use_checkpoint=k, apply_project=False),
            'CLIP.forward': lambda x, k: model(x, tok, use_checkpoint=k),
            'CLIP.forward(norm_embed)': lambda x, k: model(x, tok, use_checkpoint=k, norm_embed=True),
            'SpaceTimeTransformer.forward': lambda x, k: model.visual(x, use_checkpoint=k)}, c['img'], 3, c['frames'], mode)


def test_the_wide_patch_rows_skip_the_pad(clip_model, monkeypatch):
    """14 x 14 patches at a width the own GEMMs take: the PendingClip's patch matrix arrives 640 wide and F.pad is not called
    on it; the float clip pays the pad"""
    import torch.nn.functional as F
    c, model = clip_model
    ci, frames, params, flip = _source(c['img'], 2, c['frames'])
    padded = []
    real = F.pad
    monkeypatch.setattr(F, 'pad', lambda t, *a, **k: (padded.append(tuple(t.shape)), real(t, *a, **k))[1])
    with torch.no_grad():
        model.visual(ci.pending(frames, params, flip))
        on_pending = [s for s in padded if s[-1] == 3 * c['patch'] ** 2 and len(s) == 3]
        padded.clear()
        model.visual(ci(frames, params, flip))
        on_clip = [s for s in padded if s[-1] == 3 * c['patch'] ** 2 and len(s) == 3]
    assert on_pending == []
    assert len(on_clip) == (1 if c['patch'] == 14 else 0)


@pytest.mark.parametrize('mode', MODES, ids=[m[0] for m in MODES])
def test_clip_hf(mode):
    c = H.fixture()['config']
    model = _seeded(lambda: H.build_model(c))
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(1, c['vocab'], (3, 10), generator=g).to(DEV)
    mask = (torch.arange(10)[None, :] < torch.tensor([10, 7, 4])[:, None]).to(DEV)
    _check({'CLIP_HF.encode_image': lambda x, k: model.encode_image(x, use_checkpoint=k),
            'CLIP_HF.forward': lambda x, k: model(x, tok, mask=mask, use_checkpoint=k)}, c['img'], 3, c['frames'], mode)


def _openai_clip(resolution, patch, width):
    from lavila_amd import openai_model
    return _seeded(lambda: openai_model.CLIP(embed_dim=64, image_resolution=resolution, vision_layers=2, vision_width=width,
                                             vision_patch_size=patch, context_length=16, vocab_size=64, transformer_width=128,
                                             transformer_heads=2, transformer_layers=2))


@pytest.mark.parametrize('mode', MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize('tower', [(32, 16, 128), (28, 14, 256)], ids=['p16', 'p14_wide'])
def test_openai_clip_per_frame_tower(tower, mode):
    model = _openai_clip(*tower)
    tok = _tokens(3, 64)
    _check({'openai CLIP.encode_image': lambda x, k: model.encode_image(x, use_checkpoint=k),
            'VisionTransformer.forward_clip(tokens)':
                lambda x, k: model.visual.forward_clip(x, use_checkpoint=k, cls_at_last=False),
            'openai CLIP.forward': lambda x, k: model(x, tok, use_checkpoint=k)}, tower[0], 3, 2, mode)


@pytest.mark.parametrize('mode', MODES, ids=[m[0] for m in MODES])
def test_narrator(mode):
    from test_gpu_vit_tower import _narrator
    golden = load_golden('vit_tower.pt')
    m, video, _ = _narrator(golden)
    m.train()
    text = golden['narrator']['text'].to(DEV)
    B, _, Fr, S, _ = video.shape
    assert text.shape[0] == B

    def forward(x, k):
        # the gated decoder trains in bf16 only: its float32 forward runs without a graph, as in the float32 parity tests
        with contextlib.nullcontext() if torch.is_autocast_enabled() else torch.no_grad():
            return {n: t for n, t in m(x, text, use_checkpoint=k).items() if torch.is_floating_point(t)}
    _check({'VCLM_HF.encode_image': lambda x, k: m.encode_image(x, use_checkpoint=k), 'VCLM_HF.forward': forward},
           S, B, Fr, mode)


@pytest.mark.parametrize('mode', MODES, ids=[m[0] for m in MODES])
def test_video_classifiers(mode):
    from lavila.models import models
    from lavila.models.openai_model import QuickGELU
    from lavila.models.timesformer import SpaceTimeTransformer

    def tower():
        return SpaceTimeTransformer(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_frames=2,
                                    time_init='rand', attention_style='frozen-in-time', ln_pre=True, act_layer=QuickGELU,
                                    num_classes=0)
    single = _seeded(lambda: models.VideoClassifier(tower(), dropout=0.0, num_classes=7))
    multi = _seeded(lambda: models.VideoClassifierMultiHead(tower(), dropout=0.0, num_classes_list=[5, 9, 11]))
    _check({'VideoClassifier': lambda x, k: single(x, use_checkpoint=k),
            'VideoClassifierMultiHead': lambda x, k: multi(x, use_checkpoint=k)}, 32, 3, 2, mode)


def test_one_bf16_training_step_gives_the_same_gradients(clip_model):
    from lavila.models.loss import CLIPLoss
    c, model = clip_model
    B = 4
    ci, frames, params, flip = _source(c['img'], B, c['frames'], seed=9)
    tok = _tokens(B, c['vocab'], seed=9)
    crit = CLIPLoss(use_vissl=False, cache_labels=True, rank=0, world_size=1)

    def step(x):
        model.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            ld = crit(model(x, tok))
        ld['loss'].backward()
        torch.cuda.synchronize()
        return ld['loss'].detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}

    loss_a, grads_a = step(ci(frames, params, flip))
    loss_b, grads_b = step(ci.pending(frames, params, flip))
    assert torch.equal(loss_a, loss_b) and set(grads_a) == set(grads_b) and len(grads_a) > 20
    assert float(grads_a['visual.patch_embed.proj.weight'].abs().max()) > 0
    for k in grads_a:
        assert torch.equal(grads_a[k], grads_b[k]), k


def test_refusals(clip_model):
    from lavila_amd import _cabi
    from lavila_amd.graph_step import GraphedTrainStep
    c, model = clip_model
    ci, frames, params, flip = _source(c['img'], 2, c['frames'])
    pend = ci.pending(frames, params, flip)
    fm = 'frame-major'
    with pytest.raises(TypeError, match='materialize'):
        model.visual.forward_features(pend)
    with pytest.raises(TypeError, match='materialize'):
        model.visual.patch_embed(pend)
    with pytest.raises(TypeError, match='materialize') as e:
        GraphedTrainStep.__call__(None, pend, None)
    assert fm not in str(e.value)
    host = ci.pending(frames.cpu(), params, flip)
    tok = _tokens(2, c['vocab'])
    single = __import__('lavila_amd.models', fromlist=['x']).VideoClassifier(model.visual, 0.0, 3).to(DEV)
    for call in (lambda: model.encode_image(host), lambda: model(host, tok), lambda: model.visual(host), lambda: single(host)):
        with pytest.raises(_cabi.HipExtensionError, match='need a ROCm device tensor'):
            call()
    # a tower built for another size says so, as it does for a tensor
    other = ci.__class__(c['img'] * 2).pending(torch.zeros(1, c['frames'], 70, 70, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match='patch tokens'):
        model.visual(other)
