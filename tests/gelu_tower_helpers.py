"""Shared by the GELU-tower tests: the fixture tests/golden/gelu_tower_clip_hf.pt (the unmodified reference's CLIP_HF around
its default-constructed SpaceTimeTransformer: exact GELU, no ln_pre, eps 1e-6), the same model built from lavila_amd with
its procedural weights, the fixture's drop-path factors and their injection. The fixture and everything derived from it are
loaded / computed once per process and must not be modified."""
import contextlib
import functools
import io

import torch

import clip_hf_helpers as CH
from conftest import load_golden
from oracle import oracle as O


@functools.lru_cache(maxsize=None)
def fixture():
    return load_golden('gelu_tower_clip_hf.pt')


def build_vision(c, drop_path_rate=0.0, **kwargs):
    """The tower as CLIP_HF_TIMESFORMER_DISTILBERT_BASE builds it, at the fixture's size: act_layer, ln_pre and norm_layer
    stay at the class's defaults."""
    from lavila.models.timesformer import SpaceTimeTransformer
    with contextlib.redirect_stdout(io.StringIO()):
        vis = SpaceTimeTransformer(img_size=c['img'], patch_size=c['patch'], embed_dim=c['dim'], depth=c['depth'],
                                   num_heads=c['heads'], num_frames=c['frames'], time_init='zeros',
                                   attention_style='frozen-in-time', drop_path_rate=drop_path_rate, **kwargs)
    vis.head = vis.pre_logits = vis.fc = torch.nn.Identity()
    return vis


def build_model(c, drop_path_rate=0.0, **kwargs):
    from lavila.models import models
    with contextlib.redirect_stdout(io.StringIO()):
        return models.CLIP_HF(embed_dim=c['embed'], vision_width=c['dim'], vision_model=build_vision(c, drop_path_rate),
                              text_width=c['t_dim'], text_model=CH.build_text(c), text_use_cls_token=True,
                              text_is_regressive=False, **kwargs)


@functools.lru_cache(maxsize=None)
def weights():
    """name -> float32 tensor, the weights the fixture was generated with."""
    fx = fixture()
    return O.procedural_weights(dict(fx['state_dict']), seed=fx['weight_seed'])


@functools.lru_cache(maxsize=None)
def inputs():
    """video, ids, mask of the fixture (tools/gen_gelu_tower_golden.py: inputs)."""
    fx = fixture()
    c = fx['config']
    B, L = c['batch'], c['length']
    video = O.synthetic_batch(B, c['frames'], c['img'], seed=fx['input_seed'])[0]
    state = torch.random.get_rng_state()
    torch.manual_seed(fx['input_seed'])
    ids = torch.randint(1, c['vocab'], (B, L))
    torch.random.set_rng_state(state)
    mask = torch.zeros(B, L)
    for b, n in enumerate(fx['prefix_lengths']):
        mask[b, :n] = 1
    return video, ids * mask.long(), mask


def fixture_scales(device='cpu'):
    """{block index: (c_space, c_mlp)} float32 factors keep / (1 - rate) from the keep masks the reference drew."""
    fx = fixture()
    c = fx['config']
    rates = [r.item() for r in torch.linspace(0, c['drop_path_rate'], c['depth'])]
    out = {}
    for name, site in fx['drop']['masks'].items():
        i = int(name.split('.')[1])
        out[i] = tuple((site[k].float() / (1.0 - rates[i])).to(device) for k in ('space', 'mlp'))
    return out


def inject_masks(monkeypatch, model, scales):
    """Replaces DropPath.sample_scale of every dropping block by the fixture's factors: space branch first, then the MLP
    branch, again from the start when a block is re-run (activation checkpointing). Returns the list of calls."""
    calls = []
    for i, blk in enumerate(model.visual.blocks):
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


check_selected = CH.check_selected
