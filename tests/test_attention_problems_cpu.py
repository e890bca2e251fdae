"""CPU: the tied-softmax problem builder (attention_problems.py) on every shape the GPU tests use. Its exact float64
reference must agree with the oracle's autograd, its preconditions must hold (the builder asserts them itself), and its
tie partners must straddle the tile boundaries the kernels use, so a broken builder is caught without a GPU."""
import pytest
import torch

import attention_problems as AP
from oracle import oracle as O


def _oracle(p):
    H = p.heads
    D = 64 * H
    x = p.qkv.clone().requires_grad_(True)
    if p.kind in ('space', 'time'):
        B, F, N, _ = p.shape
        out = O.divided_attention_core(x, H, F, N, p.kind)
        out.backward(p.dout)
        return out.detach(), x.grad
    if p.kind == 'causal':
        out = O.causal_attention_core(x, H)
        out.backward(p.dout)
        return out.detach(), x.grad
    q, kv = x[:, 0, :D], x[:, :, D:]
    out = O.cls_attention_core(q, kv, H)
    out.backward(p.dout[:, 0])
    return out.detach(), x.grad


@pytest.mark.parametrize('kind,shape', AP.all_cases(), ids=lambda v: str(v).replace(' ', ''))
def test_builder_matches_the_oracle(kind, shape):
    p = AP.make(kind, shape)
    out, grad = _oracle(p)
    want_out = p.out[:, 0] if kind == 'cls' else p.out
    # the oracle keeps the exp(-480) residue the builder flushes: agreement to far below the 2^-6 quantum
    assert (out - want_out).abs().max().item() < 1e-12
    assert (grad - p.dqkv).abs().max().item() < 1e-9
    D = 64 * p.heads
    assert torch.equal(p.dbias[D:2 * D], torch.zeros(D, dtype=torch.float64))


@pytest.mark.parametrize('kind,shape', AP.all_cases(), ids=lambda v: str(v).replace(' ', ''))
def test_builder_preconditions(kind, shape):
    """What the builder asserts, spelled out once more on the returned problem (a builder whose _check went soft would
    fail here)."""
    p = AP.make(kind, shape)
    D = 64 * p.heads
    for x in (p.qkv, p.dout, p.out, p.dqkv):
        assert torch.equal(x.to(torch.bfloat16).double(), x)
    assert torch.equal(p.qkv[..., :2 * D].to(torch.float8_e4m3fn).double(), p.qkv[..., :2 * D])
    m = p.mult[:, :, sorted({int(i) for q, _, _ in p.blocks for i in q.reshape(-1)})]
    assert bool(((m == 1) | (m == 2) | (m == 4)).all())
    nz = p.dqkv[p.dqkv != 0].abs()
    assert nz.numel() == 0 or nz.min().item() >= 2.0 ** -6
    dq = p.dqkv[..., :D].reshape(*p.dqkv.shape[:2], p.heads, 64)
    dk = p.dqkv[..., D:2 * D].reshape(*p.dqkv.shape[:2], p.heads, 64)
    if kind in ('space', 'time', 'cls') and int(p.mult[:, :, 0].max()) > 1:
        assert bool((dq[:, 0] != 0).any()) and bool((dk[:, 0] != 0).any()), 'cls row: dq and dk must be nonzero'
    if kind in ('space', 'time', 'causal'):
        tied = p.key_tied[None, :, None].expand_as(dk[..., 0])
        assert (dk != 0).any(-1)[tied].double().mean().item() >= 0.9
        tied_q = p.mult.permute(0, 2, 1) > 1
        assert (dq != 0).any(-1)[tied_q].double().mean().item() >= 0.9


@pytest.mark.parametrize('kind,shape', [('space', (2, 4, 196, 12)), ('time', (1, 16, 196, 12)), ('time', (2, 5, 9, 4)),
                                        ('space', (1, 2, 576, 2)), ('space', (1, 1, 640, 1)), ('causal', (2, 272, 2)),
                                        ('cls', (2, 3137, 12))])
def test_every_row_of_the_benched_shapes_is_tied(kind, shape):
    """At the geometries the benchmark runs, (almost) every query row has a tied softmax and a nonzero dq."""
    p = AP.make(kind, shape)
    D = 64 * p.heads
    rows = sorted({int(i) for q, _, _ in p.blocks for i in q.reshape(-1)})
    dq = p.dqkv[:, rows, :D].reshape(p.qkv.shape[0], len(rows), p.heads, 64)
    assert (dq != 0).any(-1).double().mean().item() >= 0.9


def _slot_classes(n):
    cls, _, size = AP.group_layout(n)
    return cls, size


@pytest.mark.parametrize('n', [33, 65, 197, 257, 289, 577, 592, 641])
def test_space_tie_partners_straddle_the_kernel_tiles(n):
    """A group of n keys (slot 0 = cls): the cls key and the first / last key share a class, and classes straddle the
    fused backward's 32-key pairs, 16-key tiles and the streaming kernels' 64-key tiles."""
    cls, size = _slot_classes(n)
    assert int(size[cls[0]]) in (2, 4) and cls[0] == cls[n - 1]
    lo = torch.full((size.numel(),), n).scatter_reduce(0, cls, torch.arange(n), 'amin')
    hi = torch.full((size.numel(),), -1).scatter_reduce(0, cls, torch.arange(n), 'amax')
    for tile in (16, 32, 64):
        for b in range(tile, n, tile):
            crossing = int(((lo < b) & (hi >= b)).sum())
            assert crossing >= min(b, n - b) // 2, f'{crossing} classes cross the {tile}-key boundary at {b}'


@pytest.mark.parametrize('F', [4, 5, 8, 12, 16])
def test_time_tie_partners_include_the_first_and_last_frame(F):
    """A time group (slot 0 = cls, slot 1 + f = frame f): frames 0 and F-1 tie, and so does the cls key."""
    cls, size = _slot_classes(1 + F)
    assert int(size[cls[0]]) in (2, 4)
    if F >= 5:
        assert cls[1] == cls[F]
    else:
        assert cls[0] == cls[F]


@pytest.mark.parametrize('L', [77, 130, 256, 272])
def test_causal_tie_partners_cross_16_key_tiles(L):
    cls, _, size = AP.causal_layout(L)
    cross = 0
    for c in range(size.numel()):
        slots = torch.nonzero(cls == c).flatten()
        cross += int(slots.numel() > 1 and (slots // 16).unique().numel() > 1)
    assert cross >= 0.7 * size.numel()


def test_divided_problem_ties_the_cls_key_in_every_group():
    p = AP.divided_problem(1, 16, 9, 4, 'time', seed=1)
    assert int(p.key_tied[0]) == 1
    # the cls key's class has a member in every location group
    assert (p.tok_class[1:] == 0).sum().item() >= 9
