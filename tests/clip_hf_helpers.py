"""Shared by the CLIP_HF tests: the fixture, the small model of tests/golden/clip_hf_distilbert.pt built from lavila_amd
and its procedural weights. The fixture and every float64 result derived from it are loaded / computed once per process and
must not be modified."""
import contextlib
import functools
import io

import torch

from conftest import load_golden
from oracle import oracle as O


@functools.lru_cache(maxsize=None)
def fixture():
    return load_golden('clip_hf_distilbert.pt')


def text_config(c, **overrides):
    from lavila_amd.distilbert import distilbert_config
    kw = dict(vocab_size=c['vocab'], max_position_embeddings=c['positions'], dim=c['t_dim'], n_heads=c['t_heads'],
              n_layers=c['t_layers'], hidden_dim=c['t_hidden'])
    kw.update(overrides)
    return distilbert_config(**kw)


def build_text(c, **overrides):
    from lavila_amd.distilbert import DistilBertModel
    return DistilBertModel(text_config(c, **overrides))


def build_vision(c):
    from lavila.models.openai_model import QuickGELU
    from lavila.models.timesformer import SpaceTimeTransformer
    with contextlib.redirect_stdout(io.StringIO()):
        vis = SpaceTimeTransformer(img_size=c['img'], patch_size=c['patch'], embed_dim=c['dim'], depth=c['depth'],
                                   num_heads=c['heads'], num_frames=c['frames'], time_init='zeros',
                                   attention_style='frozen-in-time', ln_pre=True, act_layer=QuickGELU)
    vis.head = vis.pre_logits = vis.fc = torch.nn.Identity()
    return vis


def build_model(c, **kwargs):
    from lavila.models import models
    with contextlib.redirect_stdout(io.StringIO()):
        return models.CLIP_HF(embed_dim=c['embed'], vision_width=c['dim'], vision_model=build_vision(c),
                              text_width=c['t_dim'], text_model=build_text(c), text_use_cls_token=True,
                              text_is_regressive=False, **kwargs)


@functools.lru_cache(maxsize=None)
def weights():
    """name -> float32 tensor, the weights the fixture was generated with."""
    fx = fixture()
    return O.procedural_weights(dict(fx['state_dict']), seed=fx['weight_seed'])


@functools.lru_cache(maxsize=None)
def video():
    fx = fixture()
    c = fx['config']
    return O.synthetic_batch(c['batch'], c['frames'], c['img'], seed=fx['input_seed'])[0]


def check_selected(grads, part, atol, rtol, what, skip=()):
    """The stored gradients of a fixture part (1-D in full, four rows of every 2-D one) against name -> gradient."""
    n = 0
    for k, want in part['grads'].items():
        if k in skip:
            continue
        torch.testing.assert_close(grads[k].detach().cpu().double().reshape(want.shape), want.double(), atol=atol, rtol=rtol,
                                   msg=lambda m, k=k: f'{what} grad {k}: {m}')
        n += 1
    for k, (rows, want) in part['grad_slices'].items():
        if k in skip:
            continue
        g = grads[k].detach().cpu().double()
        g2 = g.reshape(-1, g.shape[-1]) if g.ndim == 3 else g.reshape(g.shape[0], -1)
        torch.testing.assert_close(g2[rows], want.double(), atol=atol, rtol=rtol,
                                   msg=lambda m, k=k: f'{what} grad rows of {k}: {m}')
        n += 1
    return n
