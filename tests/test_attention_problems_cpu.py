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


CASES = AP.all_cases() + AP.narrator_cases()


def _cross_or_mq_oracle(p):
    """The narrator's two query / key kinds through their own accessors (the C-ABI layouts) and the oracle's cores:
    (out, dq, dkv) of the oracle and of the builder."""
    if p.kind == 'cross':
        contexts, qrep, H, Tk = p.shape
        D = 64 * H
        q, kv, dout, out, dq, dkv = p.as_cross()
        qo, kvo = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
        oo = O.gpt2_attention_core(qo.reshape(contexts, qrep, D), kvo[..., :D], kvo[..., D:], H, causal=False)
        oo.backward(dout.reshape(contexts, qrep, D))
        return (oo.detach().reshape(-1, D), qo.grad, kvo.grad), (out, dq, dkv)
    B, NQ, H, Tk, shared = p.shape
    q, kv, dout, out, dq, dkv = p.as_mq()
    qo, kvo = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    oo = O.mq_cross_attention_core(qo[None].expand(B, -1, -1) if shared else qo, kvo, H)
    oo.backward(dout)
    return (oo.detach(), qo.grad, kvo.grad), (out, dq, dkv)


@pytest.mark.parametrize('kind,shape', CASES, ids=lambda v: str(v).replace(' ', ''))
def test_builder_matches_the_oracle(kind, shape):
    p = AP.make(kind, shape)
    if kind in ('cross', 'mq'):
        got, want = _cross_or_mq_oracle(p)
        assert (got[0] - want[0]).abs().max().item() < 1e-12
        assert (got[1] - want[1]).abs().max().item() < 1e-9 and (got[2] - want[2]).abs().max().item() < 1e-9
        return
    out, grad = _oracle(p)
    want_out = p.out[:, 0] if kind == 'cls' else p.out
    # the oracle keeps the exp(-480) residue the builder flushes: agreement to far below the 2^-6 quantum
    assert (out - want_out).abs().max().item() < 1e-12
    assert (grad - p.dqkv).abs().max().item() < 1e-9
    D = 64 * p.heads
    assert torch.equal(p.dbias[D:2 * D], torch.zeros(D, dtype=torch.float64))


@pytest.mark.parametrize('kind,shape', CASES, ids=lambda v: str(v).replace(' ', ''))
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
    if kind in ('cross', 'mq'):
        _check_query_key_problem(p)


def _check_query_key_problem(p):
    """'cross' / 'mq' through the accessors the GPU tests use: every reference tensor bf16-exact and at least 2^-6 where
    nonzero; at least 90 % of the tied rows have dq != 0; the keys that some query of their (context, head) ties are
    exactly the members of whole tie classes, at least 90 % of them have dk != 0 and no other key has; once there are
    as many queries as tied classes, that is every tied key of the layout, the last key among them."""
    nq, Tk = (p.shape[1], p.shape[3]) if p.kind == 'cross' else (p.shape[1] * p.shape[2], p.shape[3])
    H, B = p.heads, p.qkv.shape[0]
    q, kv, dout, out, dq, dkv = p.as_cross() if p.kind == 'cross' else p.as_mq()
    for x in (q, kv, dout, out, dq, dkv):
        assert torch.equal(x.to(torch.bfloat16).double(), x)
        assert x[x != 0].numel() == 0 or x[x != 0].abs().min().item() >= 2.0 ** -6
    cls, _, size = AP.group_layout(Tk)
    tied_cls = (size == 2) | (size == 4)
    target = torch.full((B, H, len(size) + 1), False)
    # the class a query targets is the class of the keys that share its code: read it back from q . k == 0
    qh = p.qkv[:, :nq, :64 * H].reshape(B, nq, H, 64).permute(0, 2, 1, 3)
    kh = p.qkv[:, nq:, 64 * H:128 * H].reshape(B, Tk, H, 64).permute(0, 2, 1, 3)
    hit = (qh @ kh.transpose(-1, -2)) == 0                                            # [B, H, nq, Tk]
    assert bool((hit.sum(-1) == size[cls][hit.int().argmax(-1)]).all()), 'a query scores 0 on part of a class'
    tied_k = (hit & tied_cls[cls]).any(2)                                             # [B, H, Tk]
    if nq >= int(tied_cls.sum()):
        assert bool((tied_k == tied_cls[cls]).all())
    if Tk >= 2:
        assert bool(tied_k[0, 0, 0]) and bool(tied_k[0, 0, Tk - 1]), 'head (0, 0) must tie the first and the last key'
    dk = p.dqkv[:, nq:, 64 * H:128 * H].reshape(B, Tk, H, 64).permute(0, 2, 1, 3)
    dk_nz = (dk != 0).any(-1)
    assert bool((dk_nz <= tied_k).all())
    assert not tied_k.any() or dk_nz[tied_k].double().mean().item() >= 0.9
    dqh = p.dqkv[:, :nq, :64 * H].reshape(B, nq, H, 64).permute(0, 2, 1, 3)
    tied_q = p.mult[:, :, :nq] > 1
    assert not tied_q.any() or (dqh != 0).any(-1)[tied_q].double().mean().item() >= 0.9
    if p.kind == 'mq' and p.shape[4] and tied_q.any():
        assert (dq.reshape(nq, 64) != 0).any(-1)[tied_q[0, 0]].double().mean().item() >= 0.9


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


@pytest.mark.parametrize('Tk', [33, 65, 128, 200, 255, 256])
def test_cross_tie_partners_straddle_the_key_tiles(Tk):
    """Keys of a context / clip: the first and the last key share a class, and classes straddle the 16-key tiles of the
    MFMA kernels, the 32-key grid of the pooler's backward and the 64 keys a wave owns in the decoder's backward."""
    cls, size = _slot_classes(Tk)
    assert int(size[cls[0]]) in (2, 4) and cls[0] == cls[Tk - 1]
    lo = torch.full((size.numel(),), Tk).scatter_reduce(0, cls, torch.arange(Tk), 'amin')
    hi = torch.full((size.numel(),), -1).scatter_reduce(0, cls, torch.arange(Tk), 'amax')
    for tile in (16, 32, 64):
        for b in range(tile, Tk, tile):
            assert int(((lo < b) & (hi >= b)).sum()) >= min(b, Tk - b) // 2


@pytest.mark.parametrize('B,L,H,cap', AP.DECODE)
def test_decode_tie_partners_sit_in_different_key_slots(B, L, H, cap):
    """lvl_decode_self_attn walks the cache with 32 key slots (key j in slot j % 32): the partners of causal_layout are 17
    apart, so (almost) every tie is merged across slots, and past 32 keys a slot holds more than one key."""
    cls, _, size = AP.causal_layout(L)
    assert cap >= L
    split = 0
    for c in range(size.numel()):
        slots = torch.nonzero(cls == c).flatten() % 32
        split += int(slots.unique().numel() == slots.numel())
    assert split == size.numel()


def test_divided_problem_ties_the_cls_key_in_every_group():
    p = AP.divided_problem(1, 16, 9, 4, 'time', seed=1)
    assert int(p.key_tied[0]) == 1
    # the cls key's class has a member in every location group
    assert (p.tok_class[1:] == 0).sum().item() >= 9
