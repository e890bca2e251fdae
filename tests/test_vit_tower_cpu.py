"""CPU: the host side of the OpenAI CLIP image tower -- openai_model.VisionTransformer / CLIP / build_model /
convert_weights and the eight constructors CLIP_OPENAI_VIT* / VCLM_OPENAI_VIT* (reference models.py:723-884, 1201-1218):
names and shapes against the reference's (tests/golden/vit_tower.pt, tools/gen_vit_tower_golden.py), the build_model round
trip, the weight import, the refusals. The full-size geometries are built on the meta device (shapes without storage)."""
import contextlib
import io
import warnings

import pytest
import torch

import vit_tower_helpers as V
from conftest import load_golden

CLIPS = {'CLIP_OPENAI_VITB32': 'ViT-B/32', 'CLIP_OPENAI_VITB16': 'ViT-B/16', 'CLIP_OPENAI_VITL14': 'ViT-L/14',
         'CLIP_OPENAI_VITL14_336PX': 'ViT-L/14@336px'}
# constructor -> (CLIP name, vision width, patches per frame, decoder width, decoder heads, decoder layers)
NARRATORS = {'VCLM_OPENAI_VITB16_GPT2_LARGE': ('ViT-B/16', 768, 196, 1280, 20, 36),
             'VCLM_OPENAI_VITB16_GPT2_XL': ('ViT-B/16', 768, 196, 1600, 25, 48),
             'VCLM_OPENAI_VITL14_GPT2_XL': ('ViT-L/14', 1024, 256, 1600, 25, 48),
             'VCLM_OPENAI_VITL14_336PX_GPT2_XL': ('ViT-L/14@336px', 1024, 576, 1600, 25, 48)}


@pytest.fixture(scope='module')
def golden():
    return load_golden('vit_tower.pt')


@contextlib.contextmanager
def quiet():
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter('ignore')
        yield


def _tiny_clip_state_dict():
    return V.clip_state_dict(V.clip_shapes(), V.CLIP['weight_seed'])


def test_reexport_resolves_to_the_new_classes():
    import lavila.models.openai_model as shim
    import lavila_amd.openai_model as impl
    for name in ('QuickGELU', 'ResidualAttentionBlock', 'Transformer', 'VisionTransformer', 'CLIP', 'build_model',
                 'convert_weights'):
        assert getattr(shim, name) is getattr(impl, name)
    from lavila.models import models
    assert models.build_model is impl.build_model


@pytest.mark.parametrize('ctor', sorted(CLIPS))
def test_clip_constructors_match_the_reference_state_dict(ctor, golden, monkeypatch):
    """Without LAVILA_CLIP_WEIGHTS_DIR: built from the published hyperparameters (with the warning), float32, eval mode;
    state dict names, order and shapes are the reference's."""
    from lavila.models import models, openai_model
    monkeypatch.delenv('LAVILA_CLIP_WEIGHTS_DIR', raising=False)
    with torch.device('meta'), contextlib.redirect_stdout(io.StringIO()), pytest.warns(UserWarning, match='NOT loaded'):
        m = getattr(models, ctor)(pretrained=True, project_embed_dim=256)          # unknown kwargs are swallowed
    assert isinstance(m, openai_model.CLIP) and isinstance(m.visual, openai_model.VisionTransformer)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == golden['real_shapes'][CLIPS[ctor]]
    assert m.dtype == torch.float32 and not m.training
    assert m.visual.conv1.bias is None and m.transformer.resblocks[0].attn_mask is not None
    assert m.visual.transformer.resblocks[0].attn_mask is None
    assert models.get_metric_names(ctor) == ['loss', 'clip_loss', 'clip_acc']
    args = type('A', (), dict(contrastive_use_vissl=False, rank=0, world_size=1))
    assert isinstance(models.get_loss(ctor, args), models.loss.CLIPLoss)


@pytest.mark.parametrize('ctor', sorted(NARRATORS))
def test_narrator_constructors(ctor, golden, monkeypatch):
    import types
    from lavila.models import models, openai_model
    clip_name, width, patches, text_width, heads, layers = NARRATORS[ctor]
    for var in ('LAVILA_CLIP_WEIGHTS_DIR', 'LAVILA_GPT2_WEIGHTS_DIR'):
        monkeypatch.delenv(var, raising=False)
    with pytest.raises(KeyError):                       # as in the reference: kwargs.pop('text_use_cls_token')
        with torch.device('meta'), quiet():
            getattr(models, ctor)()
    with torch.device('meta'), quiet():
        m = getattr(models, ctor)(text_use_cls_token=False, freeze_lm_vclm=True, gated_xattn=True)
    assert isinstance(m.visual, openai_model.VisionTransformer)
    want = [(k[len('visual.'):], s) for k, s in golden['real_shapes'][clip_name] if k.startswith('visual.')]
    assert [(k, tuple(v.shape)) for k, v in m.visual.state_dict().items()] == want
    assert m.visual.positional_embedding.shape == (patches + 1, width) and m.vision_width == width
    assert m.img_queries.shape == (256, text_width) and m.img_attn_pool.heads == heads
    assert m.img_attn_pool.to_kv.weight.shape == (128, width)
    dec = m.text_decoder
    assert len(dec.transformer.h) == layers and dec.transformer.wte.weight.shape[1] == text_width
    assert [b.has_cross for b in dec.transformer.h] == [i % 2 == 0 for i in range(layers)]          # cross_attn_freq=2
    assert dec.lm_head.weight is dec.transformer.wte.weight
    # freeze_lm_vclm: the plain GPT-2 is frozen, the cross-attention additions and the tower train
    assert not dec.transformer.h[0].attn.c_attn.weight.requires_grad and dec.transformer.h[0].alpha_cattn.requires_grad
    assert all(p.requires_grad for p in m.visual.parameters())
    assert models.get_metric_names(ctor) == ['loss', 'caption_loss', 'caption_acc', 'ppl']
    args = type('A', (), dict(contrastive_use_vissl=False, rank=0, world_size=1))
    crit = models.get_loss(ctor, args, tokenizer=types.SimpleNamespace(pad_token_id=0))
    assert isinstance(crit, models.loss.CaptionLoss)


@pytest.mark.parametrize('flag', ['freeze_visual_vclm', 'freeze_visual_vclm_temporal'])
def test_visual_freeze_flags_are_refused_by_name(flag, monkeypatch):
    """The reference calls vision_model.freeze_spatial_weights() / freeze_temporal_weights(), which VisionTransformer does
    not have (AttributeError there): refused here before anything is built."""
    from lavila.models import models
    monkeypatch.delenv('LAVILA_CLIP_WEIGHTS_DIR', raising=False)
    with pytest.raises(NotImplementedError, match=flag):
        models.VCLM_OPENAI_VITB16_GPT2_XL(text_use_cls_token=False, **{flag: True})


def test_tiny_tower_and_clip_match_the_reference_names(golden):
    from lavila.models import openai_model
    for name, c in V.TOWERS.items():
        vis = openai_model.VisionTransformer(c['resolution'], c['patch'], c['width'], c['layers'], c['heads'], c['output_dim'])
        assert list(vis.state_dict().keys()) == golden['towers'][name]['state_dict_keys']
        assert {k: tuple(v.shape) for k, v in vis.state_dict().items()} == golden['towers'][name]['shapes']
        vis.load_state_dict(V.tower_weights(golden['towers'][name]['shapes'], c['weight_seed']), strict=True)
    assert V.clip_shapes() == golden['clip']['shapes']


def test_initialisation_draws_follow_the_reference_order():
    """Same seed, same constructor arguments -> the same draws in the same order as the reference (conv1, class / positional
    embedding, the blocks, proj): two constructions agree, the text tower is re-initialised with the reference's standard
    deviations and the image tower keeps its scale * randn parameters."""
    from lavila.models import openai_model
    torch.manual_seed(3)
    a = openai_model.CLIP(64, 32, 2, 128, 16, 16, 64, 128, 2, 2)
    torch.manual_seed(3)
    b = openai_model.CLIP(64, 32, 2, 128, 16, 16, 64, 128, 2, 2)
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
    assert abs(a.visual.positional_embedding.std().item() - 128 ** -0.5) < 0.02
    assert abs(a.token_embedding.weight.std().item() - 0.02) < 2e-3
    assert abs(a.transformer.resblocks[0].mlp.c_fc.weight.std().item() - 256 ** -0.5) < 5e-3
    assert abs(a.logit_scale.item() - 2.6592600) < 1e-5
    mask = a.build_attention_mask()
    assert mask.shape == (16, 16) and mask[0, 1] == float('-inf') and mask[1, 0] == 0 and mask[5, 5] == 0


def test_build_model_round_trip_reproduces_every_tensor():
    from lavila.models import openai_model
    c = V.CLIP
    sd = _tiny_clip_state_dict()
    extra = dict(sd, input_resolution=torch.tensor(c['resolution']), context_length=torch.tensor(c['context']),
                 vocab_size=torch.tensor(c['vocab']))                 # the TorchScript archives carry these three
    keys = list(extra)
    m = openai_model.build_model(extra)
    assert list(extra) == keys                                         # the caller's dict is left alone
    got = m.state_dict()
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    assert all(v.dtype == torch.float32 for v in got.values()) and not m.training
    v = m.visual
    assert (v.input_resolution, v.output_dim, v.conv1.kernel_size, len(v.transformer.resblocks)) == \
        (c['resolution'], c['embed'], (c['patch'], c['patch']), c['vision_layers'])
    assert v.transformer.resblocks[0].attn.num_heads == c['vision_width'] // 64
    assert (m.context_length, m.vocab_size, m.transformer.width, m.transformer.layers) == \
        (c['context'], c['vocab'], c['text_width'], c['text_layers'])
    with pytest.raises(RuntimeError, match='Missing key'):
        openai_model.build_model({k: t for k, t in sd.items() if k != 'visual.ln_post.bias'})


def test_convert_weights_halves_what_the_reference_halves():
    from lavila.models import openai_model
    m = openai_model.build_model(_tiny_clip_state_dict())
    openai_model.convert_weights(m)
    half = {k for k, t in m.state_dict().items() if t.dtype == torch.float16}
    keep = {k for k, t in m.state_dict().items() if t.dtype == torch.float32}
    assert all(('.ln_' in k or k.startswith(('ln_final', 'visual.ln_')) or k in (
        'positional_embedding', 'logit_scale', 'token_embedding.weight', 'visual.class_embedding',
        'visual.positional_embedding')) for k in keep), sorted(keep)
    assert {'visual.conv1.weight', 'visual.proj', 'text_projection', 'transformer.resblocks.0.attn.in_proj_weight',
            'transformer.resblocks.0.attn.in_proj_bias', 'visual.transformer.resblocks.2.attn.out_proj.bias',
            'visual.transformer.resblocks.0.mlp.c_fc.weight'} <= half
    sd = _tiny_clip_state_dict()              # fp16-representable values: the conversion and .float() lose nothing
    assert all(torch.equal(t.float(), sd[k]) for k, t in m.state_dict().items())


def test_weights_are_imported_through_the_weights_dir(tmp_path, monkeypatch):
    from lavila.models import models, openai_model
    sd = _tiny_clip_state_dict()
    torch.save(sd, tmp_path / 'ViT-B-32.pt')
    monkeypatch.setenv('LAVILA_CLIP_WEIGHTS_DIR', str(tmp_path))
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter('error')                    # no "NOT loaded" warning on this path
        m = models.CLIP_OPENAI_VITB32()
    assert isinstance(m, openai_model.CLIP) and not m.training
    assert all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    with pytest.raises(RuntimeError, match='not found'):
        models.CLIP_OPENAI_VITB16()
    # the narrator takes the same checkpoint's tower
    torch.save(sd, tmp_path / 'ViT-B-16.pt')
    with torch.device('meta'), quiet():
        n = models.VCLM_OPENAI_VITB16_GPT2_LARGE(text_use_cls_token=True)
    assert n.visual.conv1.weight.shape == sd['visual.conv1.weight'].shape


def test_graphed_step_refuses_the_per_frame_models():
    from lavila.models import openai_model
    from lavila_amd.graph_step import GraphedTrainStep
    from lavila_amd.narrator import VCLM_HF
    clip = openai_model.build_model(_tiny_clip_state_dict())
    narrator = VCLM_HF(vision_width=128, vision_model=clip.visual, text_width=192, text_decoder=None, num_img_queries=8,
                       heads=3)
    for net in (clip, narrator):
        with pytest.raises(NotImplementedError, match='per-frame OpenAI CLIP'):
            GraphedTrainStep(net, None, None, (2, 3, 2, 32, 32), (2, 16), 'cuda')


def test_refusals():
    from lavila.models import openai_model
    from lavila_amd._cabi import HipExtensionError
    with pytest.raises(NotImplementedError, match='ModifiedResNet'):
        openai_model.CLIP(64, 224, (3, 4, 6, 3), 64, None, 77, 49408, 512, 8, 12)
    with pytest.raises(NotImplementedError, match='ModifiedResNet'):
        openai_model.build_model({'visual.layer1.0.conv1.weight': torch.zeros(64, 64, 1, 1)})
    with pytest.raises(NotImplementedError, match='causal'):
        openai_model.ResidualAttentionBlock(128, 2, torch.zeros(5, 5))
    with pytest.raises(NotImplementedError, match='causal'):
        openai_model.ResidualAttentionBlock(128, 2, torch.full((5, 5), float('-inf')).tril_(-1))
    with pytest.raises(NotImplementedError, match='head_dim 64'):
        openai_model.ResidualAttentionBlock(96, 2)
    masked = openai_model.ResidualAttentionBlock(128, 2, torch.full((5, 5), float('-inf')).triu_(1))
    plain = openai_model.ResidualAttentionBlock(128, 2)
    assert masked.attn_mask is not None and plain.attn_mask is None
    assert list(masked.state_dict()) == list(plain.state_dict())
    with pytest.raises(NotImplementedError, match='cls row'):
        plain.chain_rows(torch.zeros(2, 5, 128), None, None, torch.tensor([1, 2]))
    vis = openai_model.VisionTransformer(32, 16, 128, 1, 2, 64)
    with pytest.raises(ValueError, match='images'):
        vis(torch.zeros(1, 3, 2, 32, 32))
    with pytest.raises(ValueError, match='clips'):
        vis.forward_clip(torch.zeros(1, 3, 32, 32))
    with torch.no_grad(), pytest.raises(HipExtensionError):          # there is no CPU path
        vis(torch.zeros(1, 3, 32, 32))
