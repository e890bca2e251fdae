"""CPU (-m "not gpu"): CLIP_HF_TIMESFORMER_DISTILBERT_BASE at the drop-in boundary -- its signature, its state-dict names and
shapes against the reference's (tests/golden/gelu_tower_clip_hf.pt: the default-constructed SpaceTimeTransformer with a
patch-embedding bias and no ln_pre), load_pretrained_vit, get_loss / get_metric_names, and how Mlp classifies its activation.
The constructor is run at the fixture's size: the sizes it leaves to the classes' defaults are replaced (SpaceTimeTransformer's
img_size / embed_dim / depth / num_heads, the DistilBERT configuration), nothing it passes itself is."""
import functools
import inspect
import types
import warnings

import pytest
import torch
import torch.nn as nn

import clip_hf_helpers as CH
import gelu_tower_helpers as H

NAME = 'CLIP_HF_TIMESFORMER_DISTILBERT_BASE'


@pytest.fixture
def small(monkeypatch):
    """lavila.models.models with the size defaults of the two towers replaced by the fixture's."""
    from lavila.models import models
    c = H.fixture()['config']
    monkeypatch.setattr(models, 'SpaceTimeTransformer', functools.partial(
        models.SpaceTimeTransformer, img_size=c['img'], patch_size=c['patch'], embed_dim=c['dim'], depth=c['depth'],
        num_heads=c['heads']))
    monkeypatch.setattr(models, 'distilbert_config', lambda name: CH.text_config(c))
    return models


def _construct(models, **kwargs):
    c = H.fixture()['config']
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return getattr(models, NAME)(num_frames=c['frames'], project_embed_dim=c['embed'], **kwargs)


def test_signature_equals_the_references():
    from lavila.models import models
    assert str(inspect.signature(getattr(models, NAME))) == H.fixture()['signatures'][NAME]


def test_text_use_cls_token_is_popped_without_a_default(small):
    with pytest.raises(KeyError, match='text_use_cls_token'):
        _construct(small)


def test_state_dict_equals_the_references_and_loads_both_ways(small):
    fx = H.fixture()
    m = _construct(small, text_use_cls_token=False)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    # text_width = 768 is a constant of the constructor (distilbert-base-uncased), the fixture's text tower is 256 wide
    want = [(k, (768, s[1]) if k == 'text_projection' else s) for k, s in fx['state_dict']]
    assert got == want
    assert [k for k, _ in m.named_parameters()] == fx['param_names']
    keys = [k for k, _ in got]
    assert 'visual.patch_embed.proj.bias' in keys and not any(k.startswith('visual.ln_pre.') for k in keys)
    vis = m.visual
    assert vis.ln_pre is None and vis.norm.eps == 1e-6 and vis.blocks[0].norm1.eps == 1e-6
    assert all(isinstance(getattr(vis, k), nn.Identity) for k in ('head', 'pre_logits', 'fc'))
    assert isinstance(vis.blocks[0].mlp.act, nn.GELU) and vis.blocks[0].mlp.act.approximate == 'none'
    assert m.projection == 'default' and m.text_use_cls_token is True and m.text_is_regressive is False
    # the reference's weights load strictly, and this model's load strictly into a model built as the fixture's was
    tp = torch.randn(768, fx['config']['embed'], generator=torch.Generator().manual_seed(1))
    print(m.load_state_dict({**H.weights(), 'text_projection': tp}, strict=True))
    other = H.build_model(fx['config'])
    print(other.load_state_dict({**m.state_dict(), 'text_projection': H.weights()['text_projection']}, strict=True))
    for k, v in H.weights().items():
        assert torch.equal(other.state_dict()[k], v), k
    assert torch.equal(m.text_projection, tp)


def test_constructor_arguments_reach_the_model(small):
    m = _construct(small, text_use_cls_token=True, drop_path_rate=0.5, temperature_init=0.05)
    from lavila_amd.timesformer import DropPath
    assert isinstance(m.visual.blocks[1].drop_path, DropPath) and m.visual.blocks[1].drop_path.drop_prob == 0.5
    assert not isinstance(m.visual.blocks[0].drop_path, DropPath) or m.visual.blocks[0].drop_path.drop_prob == 0
    torch.testing.assert_close(m.logit_scale.detach(), torch.log(torch.tensor(1 / 0.05)))
    # time_init='zeros' (timesformer.py:159-163): qkv = 0, proj.weight = 1, proj.bias = 0
    ta = m.visual.blocks[0].timeattn
    assert not ta.qkv.weight.any() and not ta.qkv.bias.any() and not ta.proj.bias.any() and bool((ta.proj.weight == 1).all())
    with pytest.raises(NotImplementedError, match='frozen_in_time'):
        _construct(small, text_use_cls_token=True, projection='frozen_in_time')


def test_load_pretrained_vit(small, tmp_path, monkeypatch):
    fx = H.fixture()
    monkeypatch.delenv('LAVILA_VIT_WEIGHTS_DIR', raising=False)
    with pytest.warns(UserWarning, match='LAVILA_VIT_WEIGHTS_DIR'):
        assert small.load_pretrained_vit('vit_base_patch16_224') is None
    monkeypatch.setenv('LAVILA_VIT_WEIGHTS_DIR', str(tmp_path))
    with pytest.raises(RuntimeError, match='vit_base_patch16_224 not found'):
        small.load_pretrained_vit('vit_base_patch16_224')
    # a file in timm's layout: the keys a ViT shares with the TimeSformer, its 1000-class head (which the tower still has
    # while the file is loaded) and a key the tower does not know; the time attention, norm3 and temporal_embed are missing
    # from it -- loaded non-strictly, as the reference does
    w = H.weights()
    shared = {k[len('visual.'):]: v for k, v in w.items()
              if k.startswith('visual.') and not any(s in k for s in ('timeattn', 'norm3', 'temporal_embed'))}
    vit = dict(shared)
    vit['head.weight'], vit['head.bias'] = torch.zeros(1000, fx['config']['dim']), torch.zeros(1000)
    vit['fc_norm.weight'] = torch.ones(fx['config']['dim'])
    torch.save(vit, tmp_path / 'vit_base_patch16_224.pt')
    monkeypatch.setattr(small, 'load_pretrained_distilbert', lambda name: None)
    m = _construct(small, text_use_cls_token=False)
    sd = m.visual.state_dict()
    for k, v in shared.items():
        assert torch.equal(sd[k], v), k
    assert isinstance(m.visual.head, nn.Identity)
    assert not sd['blocks.0.timeattn.qkv.weight'].any()           # not in the file: keeps its initialisation (zeros)


def test_mlp_classifies_its_activation_once():
    from lavila.models.openai_model import QuickGELU
    from lavila_amd import ops
    from lavila_amd.timesformer import Mlp, QuickGELUAct, SpaceTimeBlock
    kinds = {QuickGELU: ops.ACT_QUICKGELU, QuickGELUAct: ops.ACT_QUICKGELU, nn.GELU: ops.ACT_GELU,
             functools.partial(nn.GELU, approximate='tanh'): None, nn.ReLU: None}
    for act_layer, want in kinds.items():
        m = Mlp(64, 256, act_layer=act_layer)
        assert m.act_kind == want, (act_layer, m.act_kind)
        assert m._fused_act == (want == ops.ACT_QUICKGELU)
    assert (ops.ACT_QUICKGELU, ops.ACT_GELU) == ('quickgelu', 'gelu')
    blk = SpaceTimeBlock(dim=64, num_heads=1, qkv_bias=True)                       # the class's own default
    assert blk.mlp.act_kind == ops.ACT_GELU
    with pytest.raises(ValueError, match='fused MLP'):
        ops.mlp(torch.zeros(2, 64), m.fc1.weight, m.fc1.bias, m.fc2.weight, 'relu')
    with pytest.raises(ValueError, match='fused MLP'):
        ops.mlp_residual_layer_norm(torch.zeros(2, 64), m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, torch.zeros(2, 64),
                                    torch.ones(64), torch.zeros(64), 1e-6, act=None)


def test_epilogue_constants_match_the_header():
    import os
    import re
    from lavila_amd import _cabi as C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'lavila_hip.h')).read()
    for name in ('BIAS_GELU', 'GELU_BWD', 'BIAS_GELU_DERIV'):
        m = re.search(r'LVL_EPI_%s = (\d+)' % name, text)
        assert m and int(m.group(1)) == getattr(C, 'EPI_' + name), name
    assert (C.EPI_BIAS_GELU, C.EPI_GELU_BWD, C.EPI_BIAS_GELU_DERIV) == (6, 7, 8)


def test_get_loss_and_metric_names():
    from lavila.models import loss, models
    args = types.SimpleNamespace(contrastive_use_vissl=False, rank=0, world_size=1)
    assert isinstance(models.get_loss(NAME, args), loss.CLIPLoss)
    assert models.get_metric_names(NAME) == ['loss', 'clip_loss', 'clip_acc']
