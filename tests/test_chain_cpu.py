"""CPU: what the fused residual chain (lavila_amd/chain.py, SpaceTimeBlock.chain / chain_cls) refuses, without a device."""
import contextlib
import io

import pytest
import torch

from lavila_amd import chain
from lavila_amd import timesformer as T
from lavila_amd._cabi import HipExtensionError


def _block(**kw):
    return T.SpaceTimeBlock(dim=64, num_heads=1, act_layer=T.QuickGELUAct, norm_layer=T.LayerNorm, time_init='rand', **kw)


@pytest.mark.parametrize('method', ['chain', 'chain_cls'])
def test_training_chain_refuses_mlp_dropout(method):
    """No constructor sets mlp.drop.p (below); set afterwards, a training step on the chain names it instead of skipping it."""
    blk = _block().train()
    x = torch.zeros(2, 1 + 2 * 4, 64)
    blk.mlp.drop.p = 0.1
    with pytest.raises(NotImplementedError, match=r'mlp\.drop\.p'):
        getattr(blk, method)(x, None, None, 2, 4)
    # in eval mode dropout is the identity: the call goes on to the kernels, which have no CPU path
    with pytest.raises(HipExtensionError):
        getattr(blk.eval(), method)(x, None, None, 2, 4)
    blk.train().mlp.drop.p = 0.0
    with pytest.raises(HipExtensionError):
        getattr(blk, method)(x, None, None, 2, 4)


def test_every_constructor_route_to_mlp_dropout_raises():
    assert _block().mlp.drop.p == 0.0
    with pytest.raises(NotImplementedError):
        _block(drop=0.1)
    with contextlib.redirect_stdout(io.StringIO()):
        tower = T.SpaceTimeTransformer(img_size=32, patch_size=16, embed_dim=64, depth=2, num_heads=1, num_frames=2)
        assert all(blk.mlp.drop.p == 0.0 for blk in tower.blocks) and tower.pos_drop.p == 0.0
        with pytest.raises(NotImplementedError, match='drop_rate'):
            T.SpaceTimeTransformer(img_size=32, patch_size=16, embed_dim=64, depth=2, num_heads=1, num_frames=2,
                                   drop_rate=0.1)


def test_close_and_compose_refuse_what_no_tower_does():
    norm = T.LayerNorm(64)
    res = torch.zeros(2, 9, 64)
    waiting = chain.PendingMlp(res, _block().mlp)
    with pytest.raises(NotImplementedError, match='PendingMlp'):
        chain.close(res, waiting, None, norm, rows=0)
    with pytest.raises(NotImplementedError, match='PendingMlp'):
        chain.close(res, waiting, None, norm, keep_sum=False)
    with pytest.raises(NotImplementedError, match='PendingMlp'):
        chain.compose(res, waiting, None)


def test_compose_and_take_rows_on_tensors():
    g = torch.Generator().manual_seed(0)
    res, y, b = torch.randn(3, 4, 8, generator=g), torch.randn(3, 4, 8, generator=g), torch.randn(8, generator=g)
    assert chain.compose(res, None, None) is res
    assert torch.equal(chain.compose(res, y, b), res + y + b)
    assert torch.equal(chain.compose(res, y, b, bias_first=True), res + (y + b))
    assert torch.equal(chain.take_rows(res, 0), res[:, 0])
    rows = torch.tensor([3, 0, 2])
    assert torch.equal(chain.take_rows(res, rows), torch.stack([res[0, 3], res[1, 0], res[2, 2]]))
    assert chain.triple((1, 2)) == (1, 2, None) and chain.triple((1, 2, 3)) == (1, 2, 3)
