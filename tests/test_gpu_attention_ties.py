"""GPU (-m gpu): every attention kernel family against an EXACT float64 reference that sees dQ and dK.

The one-hot problems of test_gpu_parity_bf16.py have dS = 0, so they assert dq == dk == 0 whatever the kernel does
on that path. The tied-softmax problems of attention_problems.py give every query 1, 2 or 4 equal softmax entries over
different keys: out, dq, dk and dv are nonzero and exactly representable, so

  * bf16: every value where the reference is nonzero must come out bit for bit, every other value within 2^-10
    (float32 P = exp2(-lse log2e) ~ 1/m (1 +- 1e-7) leaves cancellation residue of that size; the builder asserts that
    this slack stays far below the 2^-6 quantum of the reference values);
  * float32: the same at a relative 2^-20;
  * lse = ln m to 1e-6 where a raw entry returns it; d(qkv bias): k third exactly 0, v third exactly sum(dout), q third
    sum(dq) under the same rule.

Every family runs in three bias modes: with a trainable qkv bias (the backward call carries the bias-gradient rider), with
none and with a frozen one (the plain entry, every dq_part pointer null: what a freeze_space or frozen-tower step runs in every
block). The bias-free runs meet the same bars, and their out and dqkv equal the trainable run's bit for bit.

The second part holds the bf16 instantiations to a float64 reference on random inputs at the benched geometries, with a
bound derived from the bf16 unit roundoff instead of the loose elementwise band of the older tests.
"""
import contextlib
import functools

import pytest
import torch

import attention_problems as AP
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF, F32 = torch.bfloat16, torch.float32


@functools.lru_cache(maxsize=None)
def _problem(kind, shape, seed=0):
    return AP.make(kind, shape, seed)


def _lib():
    from lavila_amd import _cabi as C
    return C.lib()


def _generic_calls():
    return _lib().lvl_debug_generic_attention_calls(1)


@contextlib.contextmanager
def _switch(name, on, off):
    """A library test hook set for the duration of the block and reset in a finally."""
    fn = getattr(_lib(), name)
    assert fn(on) == 0
    try:
        yield
    finally:
        fn(off)


@contextlib.contextmanager
def _fp8_qk():
    from lavila_amd import ops
    ops.set_fp8_qk(True)
    try:
        yield
    finally:
        ops.set_fp8_qk(False)


def _assert_exact(name, got, want, dt):
    """bf16: bit for bit where want != 0; float32: within 2^-20 relative. Everywhere else |got| <= 2^-10."""
    got = got.detach().double().cpu().reshape(want.shape)
    nz = want != 0
    if dt == BF:
        bad = nz & (got != want)
    else:
        bad = nz & ((got - want).abs() > 2.0 ** -20 * want.abs())
    bad |= ~nz & (got.abs() > AP.ZERO_SLACK)
    if bool(bad.any()):
        i = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f'{name}: {int(bad.sum())} of {bad.numel()} values wrong, first at {i}: '
                             f'got {got[tuple(i)].item()!r}, want {want[tuple(i)].item()!r}')


def _assert_bias(db, p, D):
    db = db.detach().double().cpu()
    want_q = p.dbias[:D]
    assert torch.count_nonzero(db[D:2 * D]) == 0, 'd(bias) k third must be exactly 0'
    assert torch.equal(db[2 * D:], p.dbias[2 * D:]), 'd(bias) v third must be exactly sum(dout)'
    # sum over rows of dq: every term is exact or within the zero slack of the reference
    rows = p.qkv.shape[0] * p.qkv.shape[1]
    tol = AP.ZERO_SLACK * rows + 2.0 ** -20 * p.dqkv[..., :D].abs().sum((0, 1))
    err = (db[:D] - want_q).abs()
    assert bool((err <= tol).all()), f'd(bias) q third: max error {err.max().item()} vs sum(dq)'


def _assert_lse(lse, p, rows=None):
    want = p.lse if rows is None else p.lse[:, :, rows]
    err = (lse.detach().double().cpu().reshape(want.shape) - want).abs().max().item()
    assert err <= 1e-6, f'lse differs from ln(m) by {err}'


BIAS_MODES = ('trainable', 'none', 'frozen')
NO_BIAS_GRAD = [m for m in BIAS_MODES if m != 'trainable']


def _qkv_bias(D, mode):
    """The qkv bias handed to the attention op: trainable (its gradient is the rider of the backward call), absent, or
    present with requires_grad=False (a frozen qkv Linear)."""
    return None if mode == 'none' else torch.zeros(3 * D, device=DEV, requires_grad=mode == 'trainable')


def _divided_once(kind, shape, dt, generic, bias_mode):
    from lavila_amd import ops
    B, F, N, H = shape
    D = 64 * H
    p = _problem(kind, shape)
    _generic_calls()
    x = p.qkv.to(DEV, dt).requires_grad_(True)
    bias = _qkv_bias(D, bias_mode)
    out = ops.divided_attention(x, F, N, H, kind, bias=bias)
    out.backward(p.dout.to(DEV, dt))
    _, lse = ops.divided_attn_fwd_raw(x.detach(), F, N, H, {'space': 0, 'time': 1}[kind])
    torch.cuda.synchronize()
    calls = _generic_calls()
    assert calls == generic, f'{calls} calls on the generic kernels, {generic} expected (bias {bias_mode})'
    _assert_exact('out', out, p.out, dt)
    _assert_exact('dq', x.grad[..., :D], p.dqkv[..., :D], dt)
    _assert_exact('dk', x.grad[..., D:2 * D], p.dqkv[..., D:2 * D], dt)
    _assert_exact('dv', x.grad[..., 2 * D:], p.dqkv[..., 2 * D:], dt)
    _assert_lse(lse, p)
    if bias_mode == 'trainable':
        _assert_bias(bias.grad, p, D)
    elif bias is not None:
        assert bias.grad is None, 'a frozen qkv bias received a gradient'
    return out.detach(), x.grad


def _run_divided(kind, shape, dt, generic=0, bias='trainable'):
    """Forward + backward through ops.divided_attention with a qkv bias, a second forward for lse, then every check.
    generic: how many of those three calls must land on the shape-generic kernels.
    bias: 'trainable' -- the backward call carries the bias-gradient rider (lvl_divided_attn_bwd_bias); 'none' / 'frozen' --
    no bias, or one with requires_grad=False: the plain entry (lvl_divided_attn_bwd, every dq_part pointer null). Those two
    meet the same exact bars, use the generic kernels as often, and their out and dqkv equal the trainable run's (made
    here, under the same library switches) bit for bit."""
    assert bias in BIAS_MODES
    out, dqkv = _divided_once(kind, shape, dt, generic, bias)
    if bias != 'trainable':
        out_t, dqkv_t = _divided_once(kind, shape, dt, generic, 'trainable')
        assert torch.equal(out, out_t), f'out differs from the run with a trainable bias (bias {bias})'
        assert torch.equal(dqkv, dqkv_t), f'dqkv differs from the run with a trainable bias (bias {bias})'


# ---- space -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', [BF, F32])
@pytest.mark.parametrize('shape', AP.SPACE_RESIDENT)
def test_space_resident_ties_exact(shape, dt):
    """Up to 288 keys: the LDS-resident MFMA forward and the fused space backward (float32: their split-operand
    instantiations, or the streaming kernels above 272 keys)."""
    B, F, N, H = shape
    fp = _lib().lvl_attention_fast_path if dt == BF else _lib().lvl_attention_fast_path_f32
    assert fp(0, F, N, H) == 1
    _run_divided('space', shape, dt)


@pytest.mark.parametrize('shape', AP.SPACE_RESIDENT_273)
def test_space_resident_forward_273_to_288_keys_ties_exact(shape):
    _run_divided('space', shape, BF)


@pytest.mark.parametrize('variant', [0, 1, 4, 5])
@pytest.mark.parametrize('shape', AP.SPACE_STREAM)
def test_space_streaming_ties_exact(shape, variant):
    """More than 288 keys: the key-tiled streaming kernels (default dispatch), every staging variant."""
    with _switch('lvl_debug_stream_variant', variant, 0):
        _run_divided('space', shape, BF)


@pytest.mark.parametrize('shape', AP.SPACE_STREAM)
def test_space_streaming_f32_ties_exact(shape):
    _run_divided('space', shape, F32)


@pytest.mark.parametrize('shape', AP.SPACE_LARGE_RESIDENT)
def test_space_large_group_resident_ties_exact(shape):
    """Large groups on the LDS-resident kernels, lvl_debug_space_stream(-1): the forward takes up to 592 keys, the
    4-wave large-group backward up to 577 (its LDS budget); at 591 keys the backward runs on the generic kernels."""
    B, F, N, H = shape
    with _switch('lvl_debug_space_stream', -1, 0):
        assert _lib().lvl_attention_fast_path(0, F, N, H) == int(N + 1 <= 577)
        _run_divided('space', shape, BF, generic=int(N + 1 > 577))


@pytest.mark.parametrize('shape', AP.SPACE_FP8)
def test_space_fp8_qk_ties_exact(shape):
    """The fp8 QK^T policy: q and k of the problem are e4m3-exact, so the bar is the same."""
    with _fp8_qk():
        _run_divided('space', shape, BF)


# ---- time ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rider', [0, 1, 2])
@pytest.mark.parametrize('dt', [BF, F32])
@pytest.mark.parametrize('shape', AP.TIME_REGISTER)
def test_time_register_ties_exact(shape, dt, rider):
    """The register-tiled time kernels (1-4, 8, 16 frames; heads not a multiple of 4 at 8 / 16 frames), every mode of
    the bias-gradient rider."""
    B, F, N, H = shape
    fp = _lib().lvl_attention_fast_path if dt == BF else _lib().lvl_attention_fast_path_f32
    assert fp(1, F, N, H) == 1
    with _switch('lvl_debug_time_bwd_rider', rider, -1):
        _run_divided('time', shape, dt)


@pytest.mark.parametrize('shape', AP.TIME_MFMA)
def test_time_mfma_ties_exact(shape):
    """The MFMA time kernels (bf16, 5-16 frames, heads % 4 == 0): the 16-frame geometry of BASELINE configs 2 / 3,
    cls dK summed over location chunks."""
    B, F, N, H = shape
    assert _lib().lvl_attention_fast_path(1, F, N, H) == 1
    _run_divided('time', shape, BF)


@pytest.mark.parametrize('shape', AP.TIME_GENERIC)
def test_time_generic_ties_exact(shape):
    B, F, N, H = shape
    assert _lib().lvl_attention_fast_path(1, F, N, H) == 0
    _run_divided('time', shape, BF, generic=3)


@pytest.mark.parametrize('kind,shape', AP.F32_GENERIC)
def test_f32_generic_ties_exact(kind, shape):
    with _switch('lvl_debug_f32_generic', 1, 0):
        B, F, N, H = shape
        assert _lib().lvl_attention_fast_path_f32({'space': 0, 'time': 1}[kind], F, N, H) == 0
        _run_divided(kind, shape, F32, generic=3)


# ---- causal text and cls-only ----------------------------------------------------------------------------------------
def _causal_lse(x, B, L, H):
    from lavila_amd import _cabi as C
    out = torch.empty(B, L, 64 * H, dtype=x.dtype, device=DEV)
    lse = torch.empty(B, H, L, dtype=torch.float32, device=DEV)
    C.check(C.lib().lvl_causal_attn_fwd(C.ptr(x), C.ptr(out), C.ptr(lse), B, L, H, C.dtype_code(x), C.stream_ptr()),
            'lvl_causal_attn_fwd')
    return lse


def _causal_once(shape, dt, bias_mode):
    from lavila_amd import ops
    B, L, H = shape
    D = 64 * H
    p = _problem('causal', shape)
    x = p.qkv.to(DEV, dt).requires_grad_(True)
    bias = _qkv_bias(D, bias_mode)
    _generic_calls()
    out = ops.causal_attention(x, H, bias=bias)
    torch.cuda.synchronize()
    assert _generic_calls() == 0, 'causal forward left the MFMA kernel'
    out.backward(p.dout.to(DEV, dt))
    lse = _causal_lse(x.detach(), B, L, H)
    torch.cuda.synchronize()
    assert _generic_calls() == int(L > 256), 'causal backward: generic kernel above 256 tokens only'
    _assert_exact('out', out, p.out, dt)
    _assert_exact('dq', x.grad[..., :D], p.dqkv[..., :D], dt)
    _assert_exact('dk', x.grad[..., D:2 * D], p.dqkv[..., D:2 * D], dt)
    _assert_exact('dv', x.grad[..., 2 * D:], p.dqkv[..., 2 * D:], dt)
    _assert_lse(lse, p)
    if bias_mode == 'trainable':
        _assert_bias(bias.grad, p, D)
    elif bias is not None:
        assert bias.grad is None, 'a frozen in_proj bias received a gradient'
    return out.detach(), x.grad


@pytest.mark.parametrize('dt', [BF, F32])
@pytest.mark.parametrize('shape', AP.CAUSAL)
def test_causal_ties_exact(shape, dt):
    """Causal text: MFMA kernels up to 256 tokens; at 272 the forward stays on the MFMA kernel and the backward goes to
    the generic one."""
    _causal_once(shape, dt, 'trainable')


@pytest.mark.parametrize('bias', NO_BIAS_GRAD)
@pytest.mark.parametrize('dt', [BF, F32])
@pytest.mark.parametrize('shape', AP.CAUSAL)
def test_causal_ties_exact_without_bias_gradient(shape, dt, bias):
    """No in_proj bias, or a frozen one: no lvl_qkv_bias_grad pass; out and dqkv as with a trainable bias, to the bit."""
    out, dqkv = _causal_once(shape, dt, bias)
    out_t, dqkv_t = _causal_once(shape, dt, 'trainable')
    assert torch.equal(out, out_t) and torch.equal(dqkv, dqkv_t)


def _cls_once(shape, dt, bias_mode):
    from lavila_amd import _cabi as C
    from lavila_amd import ops
    B, T, H = shape
    D = 64 * H
    p = _problem('cls', shape)
    q_ref, kv_ref, out_ref, dq_ref, dkv_ref = p.as_cls()
    q = q_ref.to(DEV, dt).contiguous().requires_grad_(True)
    kv = kv_ref.to(DEV, dt).contiguous().requires_grad_(True)
    bias = _qkv_bias(D, bias_mode)
    out = ops.cls_attention(q, kv, H, bias=bias)
    out.backward(p.dout[:, 0].to(DEV, dt))
    o2 = torch.empty(B, D, dtype=dt, device=DEV)
    lse = torch.empty(B, H, dtype=torch.float32, device=DEV)
    C.check(C.lib().lvl_cls_attn_fwd(C.ptr(q.detach()), C.ptr(kv.detach()), C.ptr(o2), C.ptr(lse), B, T, H,
                                     C.dtype_code(kv), C.stream_ptr()), 'lvl_cls_attn_fwd')
    torch.cuda.synchronize()
    _assert_exact('out', out, out_ref, dt)
    _assert_exact('dq', q.grad, dq_ref, dt)
    _assert_exact('dk', kv.grad[..., :D], dkv_ref[..., :D], dt)
    _assert_exact('dv', kv.grad[..., D:], dkv_ref[..., D:], dt)
    _assert_lse(lse, p, rows=[0])
    if bias_mode == 'trainable':
        db = bias.grad.detach().double().cpu()
        assert torch.count_nonzero(db[D:2 * D]) == 0
        assert torch.equal(db[2 * D:], p.dout[:, 0].sum(0))
        _assert_exact('d(bias) q third', db[:D], dq_ref.sum(0), F32)      # a float32 sum of the float32 dq
    elif bias is not None:
        assert bias.grad is None, 'a frozen qkv bias received a gradient'
    return out.detach(), q.grad, kv.grad


@pytest.mark.parametrize('dt', [BF, F32])
@pytest.mark.parametrize('shape', AP.CLS)
def test_cls_only_ties_exact(shape, dt):
    """The cls-only kernels of the last block (cls query over all T tokens, location-chunk partials combined)."""
    _cls_once(shape, dt, 'trainable')


@pytest.mark.parametrize('bias', NO_BIAS_GRAD)
@pytest.mark.parametrize('dt', [BF, F32])
@pytest.mark.parametrize('shape', AP.CLS)
def test_cls_only_ties_exact_without_bias_gradient(shape, dt, bias):
    got = _cls_once(shape, dt, bias)
    want = _cls_once(shape, dt, 'trainable')
    assert all(torch.equal(a, b) for a, b in zip(got, want))


# ---- the divided entry points without a bias gradient: lvl_divided_attn_bwd, every dq_part pointer null ---------------------
# Every shape list above that ops.divided_attention serves, with no qkv bias and with a frozen one. A trainable bias sends
# the backward to lvl_divided_attn_bwd_bias, whose kernels also leave column sums of dq (the fused space backward below 289
# keys always, the time kernels by lvl_debug_time_bwd_rider); every freeze_space / frozen-tower step runs the other branch.
def _fast(kind, dt, shape):
    B, F, N, H = shape
    fp = _lib().lvl_attention_fast_path if dt == BF else _lib().lvl_attention_fast_path_f32
    return fp({'space': 0, 'time': 1}[kind], F, N, H)


@pytest.mark.parametrize('bias', NO_BIAS_GRAD)
@pytest.mark.parametrize('dt', [BF, F32])
@pytest.mark.parametrize('shape', AP.SPACE_RESIDENT)
def test_space_resident_ties_exact_without_bias_gradient(shape, dt, bias):
    assert _fast('space', dt, shape) == 1
    _run_divided('space', shape, dt, bias=bias)


@pytest.mark.parametrize('bias', NO_BIAS_GRAD)
@pytest.mark.parametrize('shape', AP.SPACE_RESIDENT_273)
def test_space_resident_forward_273_to_288_keys_ties_exact_without_bias_gradient(shape, bias):
    _run_divided('space', shape, BF, bias=bias)


@pytest.mark.parametrize('bias', NO_BIAS_GRAD)
@pytest.mark.parametrize('dt', [BF, F32])
@pytest.mark.parametrize('shape', AP.SPACE_STREAM)
def test_space_streaming_ties_exact_without_bias_gradient(shape, dt, bias):
    _run_divided('space', shape, dt, bias=bias)


@pytest.mark.parametrize('bias', NO_BIAS_GRAD)
@pytest.mark.parametrize('shape', AP.SPACE_LARGE_RESIDENT)
def test_space_large_group_resident_ties_exact_without_bias_gradient(shape, bias):
    B, F, N, H = shape
    with _switch('lvl_debug_space_stream', -1, 0):
        assert _lib().lvl_attention_fast_path(0, F, N, H) == int(N + 1 <= 577)
        _run_divided('space', shape, BF, generic=int(N + 1 > 577), bias=bias)


@pytest.mark.parametrize('bias', NO_BIAS_GRAD)
@pytest.mark.parametrize('dt', [BF, F32])
@pytest.mark.parametrize('shape', AP.TIME_REGISTER)
def test_time_register_ties_exact_without_bias_gradient(shape, dt, bias):
    assert _fast('time', dt, shape) == 1
    _run_divided('time', shape, dt, bias=bias)


@pytest.mark.parametrize('bias', NO_BIAS_GRAD)
@pytest.mark.parametrize('shape', AP.TIME_MFMA)
def test_time_mfma_ties_exact_without_bias_gradient(shape, bias):
    assert _fast('time', BF, shape) == 1
    _run_divided('time', shape, BF, bias=bias)


@pytest.mark.parametrize('bias', NO_BIAS_GRAD)
@pytest.mark.parametrize('shape', AP.TIME_GENERIC)
def test_time_generic_ties_exact_without_bias_gradient(shape, bias):
    assert _fast('time', BF, shape) == 0
    _run_divided('time', shape, BF, generic=3, bias=bias)


@pytest.mark.parametrize('bias', NO_BIAS_GRAD)
@pytest.mark.parametrize('kind,shape', AP.F32_GENERIC)
def test_f32_generic_ties_exact_without_bias_gradient(kind, shape, bias):
    with _switch('lvl_debug_f32_generic', 1, 0):
        assert _fast(kind, F32, shape) == 0
        _run_divided(kind, shape, F32, generic=3, bias=bias)


@pytest.mark.parametrize('bias', NO_BIAS_GRAD)
@pytest.mark.parametrize('dt', [BF, F32])
@pytest.mark.parametrize('shape', [(2, 4, 196, 12), (2, 3, 5, 2)])
def test_space_backward_without_bias_gradient_is_bitwise_reproducible(shape, dt, bias):
    """Ten backward passes of the fused space kernel on its rider-free branch (TSF-B geometry, a tiny group) agree to the bit,
    as test_divided_attention_backward_is_bitwise_reproducible requires of the branch with a bias; random data."""
    from lavila_amd import ops
    B, F, N, H = shape
    D = 64 * H
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(B, 1 + F * N, 3 * D, generator=g) * 1.5).to(DEV, dt).requires_grad_(True)
    go = torch.randn(B, 1 + F * N, D, generator=g).to(DEV, dt)
    b = _qkv_bias(D, bias)
    first = None
    for _ in range(10):
        x.grad = None
        ops.divided_attention(x, F, N, H, 'space', bias=b).backward(go)
        if first is None:
            first = x.grad.clone()
        assert torch.equal(x.grad, first)
    assert b is None or b.grad is None
    assert bool(torch.isfinite(first.float()).all())


# ----------------------------------------------------------------------------------------------------------------------
# bf16 instantiations vs float64 on random inputs at the benched geometries
# ----------------------------------------------------------------------------------------------------------------------
REL_BOUND = 1e-2


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double()
    return ((a.reshape(b.shape) - b).norm() / b.norm()).item()


def _rand_case(shape, width, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(*shape, 3 * width, generator=g) * 1.5).to(BF).double()
    dout = torch.randn(*shape, width, generator=g).to(BF).double()
    return qkv, dout


def _report(name, rels):
    print(f'{name}: ' + ' '.join(f'{k}={v:.2e}' for k, v in rels.items()))
    bad = {k: v for k, v in rels.items() if not v <= REL_BOUND}
    assert not bad, f'{name}: relative L2 above {REL_BOUND}: {bad}'


@pytest.mark.parametrize('mode,shape', [('space', (2, 4, 196, 12)), ('time', (2, 4, 196, 12)),
                                        ('time', (1, 16, 196, 12)), ('space', (1, 2, 576, 2))])
def test_divided_bf16_vs_float64_random(mode, shape):
    """Relative L2 of out and of each third of dqkv, and of the cls row's out / dq / dk / dv on their own scale, must
    stay <= 1e-2. The bound is not measured: it follows from u = 2^-8 (output rounding, bf16 P and dS: about 2-4e-3
    expected). Measured on an MI355X (largest of out / dq / dk / dv, then of the cls row's four):
      space (2,4,196,12) 2.8e-3 / 2.7e-3     time (2,4,196,12) 1.7e-3 / 1.9e-3     time (1,16,196,12) 2.4e-3 / 2.5e-3
      space (1,2,576,2) 2.7e-3 / 3.5e-3      causal (4,77,8) 3.2e-3                cls (2,3137,12) 1.9e-3"""
    from lavila_amd import ops
    B, F, N, H = shape
    D = 64 * H
    qkv, dout = _rand_case((B, 1 + F * N), D, seed=3 + F + N)
    qo = qkv.clone().requires_grad_(True)
    oo = O.divided_attention_core(qo, H, F, N, mode)
    oo.backward(dout)
    x = qkv.to(DEV, BF).requires_grad_(True)
    out = ops.divided_attention(x, F, N, H, mode)
    out.backward(dout.to(DEV, BF))
    gr, wr = x.grad, qo.grad
    rels = {'out': _rel(out, oo), 'dq': _rel(gr[..., :D], wr[..., :D]), 'dk': _rel(gr[..., D:2 * D], wr[..., D:2 * D]),
            'dv': _rel(gr[..., 2 * D:], wr[..., 2 * D:]), 'cls_out': _rel(out[:, 0], oo[:, 0]),
            'cls_dq': _rel(gr[:, 0, :D], wr[:, 0, :D]), 'cls_dk': _rel(gr[:, 0, D:2 * D], wr[:, 0, D:2 * D]),
            'cls_dv': _rel(gr[:, 0, 2 * D:], wr[:, 0, 2 * D:])}
    _report(f'{mode} {shape}', rels)


def test_causal_bf16_vs_float64_random():
    from lavila_amd import ops
    B, L, H = 4, 77, 8
    D = 64 * H
    qkv, dout = _rand_case((B, L), D, seed=5)
    qo = qkv.clone().requires_grad_(True)
    oo = O.causal_attention_core(qo, H)
    oo.backward(dout)
    x = qkv.to(DEV, BF).requires_grad_(True)
    out = ops.causal_attention(x, H)
    out.backward(dout.to(DEV, BF))
    gr, wr = x.grad, qo.grad
    _report(f'causal {(B, L, H)}', {'out': _rel(out, oo), 'dq': _rel(gr[..., :D], wr[..., :D]),
                                    'dk': _rel(gr[..., D:2 * D], wr[..., D:2 * D]),
                                    'dv': _rel(gr[..., 2 * D:], wr[..., 2 * D:])})


def test_cls_bf16_vs_float64_random():
    from lavila_amd import ops
    B, T, H = 2, 3137, 12
    D = 64 * H
    g = torch.Generator().manual_seed(9)
    q = (torch.randn(B, D, generator=g) * 1.5).to(BF).double()
    kv = (torch.randn(B, T, 2 * D, generator=g) * 1.5).to(BF).double()
    dout = torch.randn(B, D, generator=g).to(BF).double()
    qo, kvo = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    oo = O.cls_attention_core(qo, kvo, H)
    oo.backward(dout)
    qg, kvg = q.to(DEV, BF).requires_grad_(True), kv.to(DEV, BF).requires_grad_(True)
    out = ops.cls_attention(qg, kvg, H)
    out.backward(dout.to(DEV, BF))
    _report(f'cls {(B, T, H)}', {'out': _rel(out, oo), 'dq': _rel(qg.grad, qo.grad),
                                 'dk': _rel(kvg.grad[..., :D], kvo.grad[..., :D]),
                                 'dv': _rel(kvg.grad[..., D:], kvo.grad[..., D:])})
