"""GPU (the tests marked gpu): the narrator's attention kernels against the EXACT float64 reference of the tied-softmax problems.

tests/test_gpu_narrator.py, test_gpu_narrator_train.py and test_gpu_boundary.py compare these kernels with random inputs
inside an elementwise band (2e-2) or a max-norm ratio (2^-7 of the largest value of a tensor): a wrong value in a small
entry -- a masked tail key, a query row of the last partial round, the P^T / dS^T image of the wrong wave -- passes both.
Here every query's softmax is {1}, {1/2, 1/2} or {1/4 x4} over different keys (attention_problems.py: 'cross' and 'mq'
problems, and the causal one for the decode step), so out, dq, dk and dv are nonzero dyadic rationals and

  * bf16: every value where the reference is nonzero comes out bit for bit, every other value within 2^-10;
  * float32: the same at a relative 2^-20

(the rule of test_gpu_attention_ties.py, whose _assert_exact is used). Every result buffer is filled with NaN and has a guard
row behind it: the guard must stay NaN and no NaN may remain inside. One shape per dispatch branch and tail of
lvl_cross_attn_rows_fwd (the branch is restated here and asserted before the call), lvl_cross_attn_rows_bwd over
its rounds of 64 rows and tiles of 16 keys, lvl_mq_cross_attn_fwd / _bwd in bf16 AND float32 with shared and per-sample
queries, lvl_decode_self_attn step by step on a NaN-filled cache.

The second part holds the bf16 instantiations to float64 on random inputs at the narrator's own geometry, relative L2 per
tensor <= 1e-2 (the bound of test_gpu_attention_ties.py: same arithmetic -- bf16 P and dS, f32 accumulation).
"""
import functools

import pytest
import torch

import attention_problems as AP
from oracle import oracle as O
from test_gpu_attention_ties import REL_BOUND, _assert_exact, _rel, _report

gpu = pytest.mark.gpu
DEV = 'cuda'
BF, F32 = torch.bfloat16, torch.float32
NAN = float('nan')
assert REL_BOUND == 1e-2


@functools.lru_cache(maxsize=None)
def _problem(kind, shape):
    return AP.make(kind, shape)


def _guarded(shape, dt):
    """A NaN-filled result buffer [prod(shape[:-1]) + 1, shape[-1]]: the last row is the guard."""
    rows = 1
    for s in shape[:-1]:
        rows *= s
    return torch.full((rows + 1, shape[-1]), NAN, dtype=dt, device=DEV)


def _inside(name, buf, shape):
    """The result inside a _guarded buffer, after checking that the guard row is untouched and no NaN is left."""
    assert torch.isnan(buf[-1].float()).all(), f'{name}: the guard row behind the result was written'
    assert not torch.isnan(buf[:-1].float()).any(), f'{name}: an element of the result was never written'
    return buf[:-1].reshape(shape)


def _dev(x, dt):
    return x.to(DEV, dt).contiguous()


# ---- lvl_cross_attn_rows_fwd -----------------------------------------------------------------------------------------
def _cross_fwd_branch(dt, qrep, Tk):
    """The dispatch of lvl_cross_attn_rows_fwd (cls_attn.hip), restated: move a threshold there and the shape lists
    below fail here instead of going blind."""
    if dt == BF and qrep >= 2 and Tk <= 256:
        return 'mfma'
    if qrep >= 2 and Tk * 128 * (4 if dt == F32 else 2) <= 150 * 1024:
        return 'lds'                      # cross_attn_shared_kernel: the context's keys / values staged once in LDS
    return 'row'                          # cls_attn_fwd_kernel, one workgroup per (row, head): context = row / qrep


CROSS_FWD = ([(BF, s, b) for s, b in zip(AP.CROSS_FWD_BF16, ['mfma'] * 5 + ['lds'] * 2 + ['row'] * 2)] +
             [(F32, s, b) for s, b in zip(AP.CROSS_FWD_F32, ['lds', 'lds', 'row', 'row'])])


def test_cross_fwd_shapes_reach_every_branch():
    assert len(CROSS_FWD) == len(AP.CROSS_FWD_BF16) + len(AP.CROSS_FWD_F32)
    for dt, (contexts, qrep, H, Tk), branch in CROSS_FWD:
        assert _cross_fwd_branch(dt, qrep, Tk) == branch, (dt, qrep, Tk)
    # the row kernel with qrep >= 2 (keys past LDS) in both types, and the largest key counts that still fit LDS
    assert {(dt, s[1] >= 2) for dt, s, b in CROSS_FWD if b == 'row'} == {(BF, True), (BF, False), (F32, True), (F32, False)}
    assert _cross_fwd_branch(BF, 2, 600) == 'lds' and _cross_fwd_branch(BF, 2, 601) == 'row'
    assert _cross_fwd_branch(F32, 2, 300) == 'lds' and _cross_fwd_branch(F32, 2, 301) == 'row'


def _cross_fwd(q, kv, out, rows, qrep, Tk, H):
    from lavila_amd import _cabi as C
    C.check(C.lib().lvl_cross_attn_rows_fwd(C.ptr(q), C.ptr(kv), C.ptr(out), rows, qrep, Tk, H, C.dtype_code(q),
                                            C.stream_ptr()), 'lvl_cross_attn_rows_fwd')


def _cross_bwd(q, kv, do, dq, dkv, rows, qrep, Tk, H):
    from lavila_amd import _cabi as C
    C.check(C.lib().lvl_cross_attn_rows_bwd(C.ptr(q), C.ptr(kv), C.ptr(do), C.ptr(dq), C.ptr(dkv), rows, qrep, Tk, H,
                                            C.dtype_code(q), C.stream_ptr()), 'lvl_cross_attn_rows_bwd')


@gpu
@pytest.mark.parametrize('dt,shape,branch', CROSS_FWD, ids=lambda v: str(v).replace(' ', '').replace('torch.', ''))
def test_cross_attn_rows_fwd_ties_exact(dt, shape, branch):
    contexts, qrep, H, Tk = shape
    assert _cross_fwd_branch(dt, qrep, Tk) == branch
    D, rows = 64 * H, contexts * qrep
    q, kv, _, out_ref, _, _ = _problem('cross', shape).as_cross()
    out = _guarded((rows, D), dt)
    _cross_fwd(_dev(q, dt), _dev(kv, dt), out, rows, qrep, Tk, H)
    torch.cuda.synchronize()
    _assert_exact('out', _inside('out', out, (rows, D)), out_ref, dt)


# ---- lvl_cross_attn_rows_bwd -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('shape', AP.CROSS_BWD, ids=lambda v: str(v).replace(' ', ''))
def test_cross_attn_rows_bwd_ties_exact(shape):
    """dq, dk and dv exactly, twice with bit-identical results: one round and one key tile, row and key tails, a second
    round of 64 rows with the last key masked, full key capacity, three rounds whose last holds 2 rows, twelve heads."""
    contexts, qrep, H, Tk = shape
    assert Tk <= 256 and qrep >= 2
    D, rows = 64 * H, contexts * qrep
    q, kv, dout, _, dq_ref, dkv_ref = _problem('cross', shape).as_cross()
    qd, kvd, dod = _dev(q, BF), _dev(kv, BF), _dev(dout, BF)
    runs = []
    for _ in range(2):
        dq, dkv = _guarded((rows, D), BF), _guarded((contexts, Tk, 2 * D), BF)
        _cross_bwd(qd, kvd, dod, dq, dkv, rows, qrep, Tk, H)
        torch.cuda.synchronize()
        runs.append((_inside('dq', dq, (rows, D)), _inside('dkv', dkv, (contexts, Tk, 2 * D))))
    (dq, dkv), (dq2, dkv2) = runs
    assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2), 'two runs differ'
    _assert_exact('dq', dq, dq_ref, BF)
    _assert_exact('dk', dkv[..., :D], dkv_ref[..., :D], BF)
    _assert_exact('dv', dkv[..., D:], dkv_ref[..., D:], BF)


# ---- lvl_mq_cross_attn_fwd / _bwd ------------------------------------------------------------------------------------
def _mq_fwd(q, kv, out, B, NQ, H, Tk, shared):
    from lavila_amd import _cabi as C
    C.check(C.lib().lvl_mq_cross_attn_fwd(C.ptr(q), 0 if shared else NQ * H * 64, C.ptr(kv), C.ptr(out), B, NQ, H, Tk,
                                          C.dtype_code(kv), C.stream_ptr()), 'lvl_mq_cross_attn_fwd')


def _mq_bwd(q, kv, do, dq, dkv, B, NQ, H, Tk, shared):
    """One backward on a NaN-poisoned workspace."""
    from lavila_amd import _cabi as C
    n_ws = C.lib().lvl_mq_cross_attn_bwd_ws(B, NQ, H, int(shared))
    assert n_ws > 0
    ws = torch.full((n_ws,), NAN, dtype=torch.float32, device=DEV)
    C.check(C.lib().lvl_mq_cross_attn_bwd(C.ptr(q), 0 if shared else NQ * H * 64, C.ptr(kv), C.ptr(do), C.ptr(dq),
                                          C.ptr(dkv), C.ptr(ws), B, NQ, H, Tk, C.dtype_code(kv), C.stream_ptr()),
            'lvl_mq_cross_attn_bwd')


@gpu
@pytest.mark.parametrize('shared', [False, True])
@pytest.mark.parametrize('dt', [BF, F32])
@pytest.mark.parametrize('shape', AP.MQ, ids=lambda v: str(v).replace(' ', ''))
def test_mq_cross_attn_ties_exact(shape, dt, shared):
    """The pooler's forward and its three backward kernels, bf16 and float32: fewer rows than a workgroup's 32 with a
    partial block of 8 keys; one key past the 64-key LDS chunk; a row tail with the second workgroup of the backward's
    32-key grid holding one key; full blocks only. Shared queries: dq is the sum over the clips."""
    B, NQ, H, Tk = shape
    D = 64 * H
    q, kv, dout, out_ref, dq_ref, dkv_ref = _problem('mq', shape + (shared,)).as_mq()
    qd, kvd, dod = _dev(q, dt), _dev(kv, dt), _dev(dout, dt)
    out = _guarded((B, NQ, D), dt)
    _mq_fwd(qd, kvd, out, B, NQ, H, Tk, shared)
    dq, dkv = _guarded(tuple(q.shape), dt), _guarded((B, Tk, 128), dt)
    _mq_bwd(qd, kvd, dod, dq, dkv, B, NQ, H, Tk, shared)
    torch.cuda.synchronize()
    _assert_exact('out', _inside('out', out, (B, NQ, D)), out_ref, dt)
    dkv = _inside('dkv', dkv, (B, Tk, 128))
    _assert_exact('dq', _inside('dq', dq, tuple(q.shape)), dq_ref, dt)
    _assert_exact('dk', dkv[..., :64], dkv_ref[..., :64], dt)
    _assert_exact('dv', dkv[..., 64:], dkv_ref[..., 64:], dt)


# ---- lvl_decode_self_attn --------------------------------------------------------------------------------------------
def _decode_steps(qkv_all, cap, H, dt):
    """Feeds qkv_all[:, t] step by step into a NaN-filled cache (the position advances on the device); returns the
    outputs [B, L, D] and the cache."""
    from lavila_amd import _cabi as C
    B, L, _ = qkv_all.shape
    D = 64 * H
    steps = _dev(qkv_all.transpose(0, 1), dt)                                       # [L, B, 3D]
    cache = torch.full((B, cap, 2 * D), NAN, dtype=dt, device=DEV)                  # unwritten rows must never be read
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    outs = _guarded((L, B, D), dt)
    for t in range(L):
        C.check(C.lib().lvl_decode_self_attn(C.ptr(steps[t]), C.ptr(cache), C.ptr(pos), C.ptr(outs[t * B:]), B, cap, H,
                                             C.dtype_code(steps), C.stream_ptr()), 'lvl_decode_self_attn')
        pos.add_(1)
    torch.cuda.synchronize()
    assert int(pos.item()) == L
    return _inside('out', outs, (L, B, D)).transpose(0, 1), cache


@gpu
@pytest.mark.parametrize('dt', [BF, F32])
@pytest.mark.parametrize('shape', AP.DECODE, ids=lambda v: str(v).replace(' ', ''))
def test_decode_self_attn_ties_exact(shape, dt):
    """Step t equals row t of the causal problem, at every step; tie partners sit 17 keys apart, so in different ones of
    the kernel's 32 key slots, and from step 32 on a slot holds more than one key. The cache ends as the k | v thirds,
    rows past the last step untouched."""
    B, L, H, cap = shape
    D = 64 * H
    p = _problem('causal', (B, L, H))
    out, cache = _decode_steps(p.qkv, cap, H, dt)
    for t in range(L):
        _assert_exact(f'out of step {t}', out[:, t], p.out[:, t], dt)
    assert torch.equal(cache[:, :L].double().cpu(), p.qkv[..., D:]), 'the cache is not the k | v rows of the steps'
    assert torch.isnan(cache[:, L:].float()).all(), 'a cache row past the last step was written'


# ----------------------------------------------------------------------------------------------------------------------
# bf16 instantiations vs float64 on random inputs at the narrator's geometry
# ----------------------------------------------------------------------------------------------------------------------
def _rand(shape, g, scale=1.5):
    return (torch.randn(*shape, generator=g) * scale).to(BF).double()


@gpu
@pytest.mark.parametrize('shape', [(3, 12, 12, 256), (1, 76, 12, 256)], ids=lambda v: str(v).replace(' ', ''))
def test_cross_attn_rows_bf16_vs_float64_random(shape):
    """Relative L2 of out, dq, dk, dv against float64 on bf16-rounded N(0, 1.5^2) q / kv and N(0, 1) dout must stay
    <= 1e-2; the bound follows from u = 2^-8 (see test_gpu_attention_ties.py), it is not measured.
    Measured on an MI355X (out / dq / dk / dv):
      (3,12,12,256)  1.9e-3 / 2.4e-3 / 2.4e-3 / 2.4e-3
      (1,76,12,256)  1.9e-3 / 2.4e-3 / 2.4e-3 / 2.3e-3"""
    contexts, qrep, H, Tk = shape
    D, rows = 64 * H, contexts * qrep
    g = torch.Generator().manual_seed(31 + qrep)
    q, kv, dout = _rand((rows, D), g), _rand((contexts, Tk, 2 * D), g), _rand((rows, D), g, 1.0)
    qo, kvo = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    oo = O.gpt2_attention_core(qo.reshape(contexts, qrep, D), kvo[..., :D], kvo[..., D:], H, causal=False)
    oo.backward(dout.reshape(contexts, qrep, D))
    qd, kvd, dod = _dev(q, BF), _dev(kv, BF), _dev(dout, BF)
    out, dq, dkv = _guarded((rows, D), BF), _guarded((rows, D), BF), _guarded((contexts, Tk, 2 * D), BF)
    _cross_fwd(qd, kvd, out, rows, qrep, Tk, H)
    _cross_bwd(qd, kvd, dod, dq, dkv, rows, qrep, Tk, H)
    torch.cuda.synchronize()
    dkv = _inside('dkv', dkv, (contexts, Tk, 2 * D))
    _report(f'cross {shape}', {'out': _rel(_inside('out', out, (rows, D)), oo.reshape(rows, D)),
                               'dq': _rel(_inside('dq', dq, (rows, D)), qo.grad),
                               'dk': _rel(dkv[..., :D], kvo.grad[..., :D]), 'dv': _rel(dkv[..., D:], kvo.grad[..., D:])})


@gpu
@pytest.mark.parametrize('shared', [False, True])
def test_mq_cross_attn_bf16_vs_float64_random(shared):
    """The pooler at the narrator's geometry: 256 queries x 8 heads over 785 tokens, 2 clips.
    Measured on an MI355X (out / dq / dk / dv):
      per-sample  1.7e-3 / 1.7e-3 / 1.7e-3 / 1.7e-3
      shared      1.7e-3 / 1.7e-3 / 1.7e-3 / 1.6e-3"""
    B, NQ, H, Tk = 2, 256, 8, 785
    D = 64 * H
    g = torch.Generator().manual_seed(37)
    q, kv, dout = _rand((NQ, D) if shared else (B, NQ, D), g), _rand((B, Tk, 128), g), _rand((B, NQ, D), g, 1.0)
    qo, kvo = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    oo = O.mq_cross_attention_core(qo[None].expand(B, -1, -1) if shared else qo, kvo, H)
    oo.backward(dout)
    qd, kvd, dod = _dev(q, BF), _dev(kv, BF), _dev(dout, BF)
    out, dq, dkv = _guarded((B, NQ, D), BF), _guarded(tuple(q.shape), BF), _guarded((B, Tk, 128), BF)
    _mq_fwd(qd, kvd, out, B, NQ, H, Tk, shared)
    _mq_bwd(qd, kvd, dod, dq, dkv, B, NQ, H, Tk, shared)
    torch.cuda.synchronize()
    dkv = _inside('dkv', dkv, (B, Tk, 128))
    _report(f'mq {(B, NQ, H, Tk)} shared={shared}',
            {'out': _rel(_inside('out', out, (B, NQ, D)), oo), 'dq': _rel(_inside('dq', dq, tuple(q.shape)), qo.grad),
             'dk': _rel(dkv[..., :64], kvo.grad[..., :64]), 'dv': _rel(dkv[..., 64:], kvo.grad[..., 64:])})


@gpu
def test_decode_self_attn_bf16_vs_float64_random():
    """The last of 77 decode steps, 2 sequences x 12 heads: the last row of the causal attention over the prefix.
    Measured on an MI355X: out 1.7e-3"""
    B, H, L = 2, 12, 77
    D = 64 * H
    qkv = _rand((B, L, 3 * D), torch.Generator().manual_seed(41))
    want = O.gpt2_attention_core(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], H, causal=True)
    out, _ = _decode_steps(qkv, L, H, BF)
    _report(f'decode {(B, H, L)} last step', {'out': _rel(out[:, L - 1], want[:, L - 1])})
