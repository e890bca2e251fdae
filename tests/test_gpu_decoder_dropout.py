"""GPU: the narrator decoder's opt-in dropout, generated inside the fused kernels (lavila_amd/csrc/dropout.h).

  * lvl_dropout_mask against the numpy restatement (tests/dropout_reference.py), bit for bit; every other test reads the
    kernels' masks from it
  * lvl_dropout_apply, the gated add + LayerNorm pair and the rows attention pair with dropout: p = 0 against the entry
    points without dropout (torch.equal), p > 0 against float64 torch with the explicit mask at the bounds of
    tests/test_gpu_narrator_train.py (2^-7 of the largest magnitude), exact cases, run-to-run bit identity
  * the autograd Functions (_GatedAddLnFn, _RowsAttnFn), with and without `drop`, against the raw calls they stand for
    (torch.equal, forward and backward)
  * one training step of the narrator against the unmodified reference under the same masks (tests/golden/narrator_dropout.pt)
  * the switch: nothing changes with it off, with all probabilities 0, in .eval() or under no_grad

Output buffers are NaN-poisoned before each call."""
import numpy as np
import pytest
import torch

import dropout_reference as R
from conftest import load_golden
from oracle import oracle as O
from test_gpu_kernels import _close
from test_gpu_narrator import _golden_model
from test_gpu_narrator_train import _bf, _compare_step, _ratio

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF = torch.bfloat16
NAN = float('nan')
SEED = 0x9E3779B97F4A7C15           # non-zero high word


def _C():
    from lavila_amd import _cabi as C
    return C


def _kernel_mask(seed, site, elem0, n, p):
    """bool [n] on the CPU: the keep mask the fused kernels generate (lvl_dropout_mask)."""
    C = _C()
    out = torch.full((n,), 77, dtype=torch.uint8, device=DEV)
    C.check(C.lib().lvl_dropout_mask(C.ptr(out), n, elem0, seed, site, p, C.stream_ptr()), 'lvl_dropout_mask')
    out = out.cpu()
    assert ((out == 0) | (out == 1)).all()
    return out.bool()


# ----------------------------------------------------------------------------------------------------------------------
# 1. the mask
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [5, SEED])
@pytest.mark.parametrize('site', [0, 7])
@pytest.mark.parametrize('n,elem0', [(8, 0), (4104, 0), (16, (1 << 34) - 8), (13, 3)])
def test_dropout_mask_equals_restatement(n, elem0, site, seed):
    for p in (0.1, 0.5):
        got = _kernel_mask(seed, site, elem0, n, p)
        want = torch.from_numpy(R.keep_mask(seed, site, elem0, n, p))
        assert torch.equal(got, want), (p, (got != want).nonzero().flatten()[:8])
    assert _kernel_mask(seed, site, elem0, n, 0.0).all()


# ----------------------------------------------------------------------------------------------------------------------
# 2. lvl_dropout_apply
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('inplace', [False, True])
@pytest.mark.parametrize('dt', [torch.float32, BF])
def test_dropout_apply(dt, inplace):
    C = _C()
    g = torch.Generator().manual_seed(21)
    n, site, p = 8 * 1031, 0, 0.1
    x = torch.randn(n, generator=g).to(dt).to(DEV)
    dy = torch.randn(n, generator=g).to(dt).to(DEV)
    x_before = x.clone()
    keep = _kernel_mask(SEED, site, 0, n, p).to(DEV)
    scale = torch.tensor(float(R.scale(p)), dtype=torch.float32, device=DEV)

    def apply(t):
        out = t.clone() if inplace else torch.full_like(t, NAN)
        C.check(C.lib().lvl_dropout_apply(C.ptr(out if inplace else t), C.ptr(out), n, SEED, site, p, C.dtype_code(t),
                                          C.stream_ptr()), 'lvl_dropout_apply')
        return out

    for t in (x, dy):                                    # applied to a gradient it is the backward
        out = apply(t)
        want = torch.where(keep, (scale * t.float()).to(dt), torch.zeros_like(t))      # one f32 product, rounded once
        assert torch.equal(out, want)
        assert (out[~keep] == 0).all() and 0 < int((~keep).sum()) < n
        assert torch.equal(out, apply(t))
    assert torch.equal(x, x_before)                      # the caller's tensor is only ever read
    out0 = torch.full_like(x, NAN)
    C.check(C.lib().lvl_dropout_apply(C.ptr(x), C.ptr(out0), n, SEED, site, 0.0, C.dtype_code(x), C.stream_ptr()), 'p=0')
    assert torch.equal(out0, x)


# ----------------------------------------------------------------------------------------------------------------------
# 3. gated add + LayerNorm with dropout
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', [0.0, 0.1, 0.5])
@pytest.mark.parametrize('gated', [True, False])
@pytest.mark.parametrize('rows,D', [(3, 192), (5, 8), (7, 1600), (2, 4096), (300, 256)])
def test_gated_add_layernorm_drop_pair(rows, D, gated, p):
    C = _C()
    lib = C.lib()
    g = torch.Generator().manual_seed(300 + rows + D)
    eps, site = 1e-5, 8
    res, res64 = _bf((rows, D), g)
    y, y64 = _bf((rows, D), g)
    dh, dh64 = _bf((rows, D), g)
    dadd, dadd64 = _bf((rows, D), g)
    gamma = 1.0 + 0.2 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    gate = torch.tanh(torch.tensor([0.7])) if gated else None
    gamma_d, beta_d, gate_d = gamma.to(DEV), beta.to(DEV), None if gate is None else gate.to(DEV)
    code = C.dtype_code(res)
    n_ws = lib.lvl_workspace_floats(b'gated_add_layernorm_bwd', rows, D)

    def fwd():
        s, h = torch.full_like(res, NAN), torch.full_like(res, NAN)
        mean, rstd = torch.full((rows,), NAN, device=DEV), torch.full((rows,), NAN, device=DEV)
        C.check(lib.lvl_gated_add_layernorm_train_drop(C.ptr(res), C.ptr(y), C.ptr(gate_d), C.ptr(gamma_d), C.ptr(beta_d), eps,
                                                       C.ptr(s), C.ptr(h), C.ptr(mean), C.ptr(rstd), rows, D, SEED, site, p,
                                                       code, C.stream_ptr()), 'train_drop')
        return s, h, mean, rstd

    def bwd(s, mean, rstd):
        ds, dy = torch.full_like(res, NAN), torch.full_like(res, NAN)
        dg, db = torch.full((D,), NAN, device=DEV), torch.full((D,), NAN, device=DEV)
        dgate = torch.full((1,), NAN, device=DEV) if gated else None
        ws = torch.full((n_ws,), NAN, device=DEV)
        C.check(lib.lvl_gated_add_layernorm_bwd_drop(C.ptr(dh), C.ptr(s), C.ptr(y), C.ptr(gate_d), C.ptr(gamma_d), C.ptr(mean),
                                                     C.ptr(rstd), C.ptr(dadd), C.ptr(ds), C.ptr(dy), C.ptr(dg), C.ptr(db),
                                                     C.ptr(dgate), C.ptr(ws), rows, D, SEED, site, p, code, C.stream_ptr()),
                'bwd_drop')
        torch.cuda.synchronize()
        return ds, dy, dg, db, dgate

    s, h, mean, rstd = fwd()
    outs = bwd(s, mean, rstd)
    for a, b in zip(fwd() + bwd(s, mean, rstd), (s, h, mean, rstd) + outs):            # two runs, bit for bit
        assert a is None or torch.equal(a, b)
    ds, dy, dg, db, dgate = outs
    for t in (s, h, mean, rstd, ds, dy, dg, db):
        assert not torch.isnan(t).any()

    if p == 0.0:                                         # the bits of the pair without dropout
        s0, h0 = torch.full_like(res, NAN), torch.full_like(res, NAN)
        mean0, rstd0 = torch.full((rows,), NAN, device=DEV), torch.full((rows,), NAN, device=DEV)
        C.check(lib.lvl_gated_add_layernorm_train(C.ptr(res), C.ptr(y), C.ptr(gate_d), C.ptr(gamma_d), C.ptr(beta_d), eps,
                                                  C.ptr(s0), C.ptr(h0), C.ptr(mean0), C.ptr(rstd0), rows, D, code,
                                                  C.stream_ptr()), 'train')
        assert torch.equal(s, s0) and torch.equal(h, h0) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0)
        ds0, dy0 = torch.full_like(res, NAN), torch.full_like(res, NAN) if gated else None
        dg0, db0 = torch.full((D,), NAN, device=DEV), torch.full((D,), NAN, device=DEV)
        dgate0 = torch.full((1,), NAN, device=DEV) if gated else None
        ws = torch.full((n_ws,), NAN, device=DEV)
        C.check(lib.lvl_gated_add_layernorm_bwd(C.ptr(dh), C.ptr(s0), C.ptr(y) if gated else None, C.ptr(gate_d),
                                                C.ptr(gamma_d), C.ptr(mean0), C.ptr(rstd0), C.ptr(dadd), C.ptr(ds0), C.ptr(dy0),
                                                C.ptr(dg0), C.ptr(db0), C.ptr(dgate0), C.ptr(ws), rows, D, code,
                                                C.stream_ptr()), 'bwd')
        assert torch.equal(ds, ds0) and torch.equal(dg, dg0) and torch.equal(db, db0)
        if gated:
            assert torch.equal(dy, dy0) and torch.equal(dgate, dgate0)
        else:
            assert torch.equal(dy, ds)
        return

    keep = _kernel_mask(SEED, site, 0, rows * D, p).reshape(rows, D)
    assert 0 < int((~keep).sum()) < rows * D
    assert torch.equal(s.cpu()[~keep], res.cpu()[~keep])                   # a dropped element leaves the residual, to the bit
    # float64 autograd with the explicit mask; c = gate * scale is formed in float32 by the kernel
    c32 = (gate if gated else torch.ones(1)) * torch.tensor(float(R.scale(p)))
    r64 = res64.clone().requires_grad_(True)
    yy = y64.clone().requires_grad_(True)
    gm, bt = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    s64 = r64 + keep.double() * c32.double() * yy
    tot = (O.layer_norm(s64, gm, bt, eps) * dh64).sum() + (s64 * dadd64).sum()
    tot.backward()
    k64 = s.double().cpu()                               # the stored (rounded) sum is what the LayerNorm sees
    torch.testing.assert_close(mean.cpu().double(), k64.mean(1), rtol=1e-5, atol=1e-5 * k64.abs().max().item())
    torch.testing.assert_close(rstd.cpu().double(), (k64.var(1, unbiased=False) + eps).rsqrt(), rtol=1e-5, atol=0)
    r = {'s': _ratio(s, s64.detach()), 'h': _ratio(h, O.layer_norm(k64, gamma.double(), beta.double(), eps)),
         'ds': _ratio(ds, r64.grad), 'dy': _ratio(dy, yy.grad), 'dgamma': _ratio(dg, gm.grad), 'dbeta': _ratio(db, bt.grad)}
    assert (dy.cpu()[~keep] == 0).all()
    if gated:
        # inputs of the gate gradient: the kernel's own ds (bf16) and scale * y where kept; only the f32 summation order differs
        prod = ds.double().cpu() * keep.double() * float(R.scale(p)) * y64
        err, bound = abs(dgate.item() - prod.sum().item()), 2.0 ** -8 * prod.abs().sum().item()
        print(f'[gated_add_layernorm_bwd_drop {rows, D} p={p}] |dgate - want| {err:.3e} (bound {bound:.3e})')
        assert err <= bound
    print(f'[gated_add_layernorm drop pair {rows, D} gated={gated} p={p}] worst ratios {r} (bound {2.0 ** -7:.2e})')
    assert max(r.values()) <= 2.0 ** -7, r


# ----------------------------------------------------------------------------------------------------------------------
# 4. rows attention with dropout (cross-attention layout and the causal self-attention on qkv)
# ----------------------------------------------------------------------------------------------------------------------
def _attn64(q, k, v, H, causal, keep, scale):
    """float64: softmax(q k^T / 8 [causal]) -> keep ? scale * P : 0 -> . v; q [ctx, Lq, D], k / v [ctx, Lk, D],
    keep bool [ctx, H, Lq, Lk]."""
    ctx, Lq, D = q.shape
    Lk = k.shape[1]
    qh, kh, vh = (t.reshape(ctx, -1, H, 64).permute(0, 2, 1, 3) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / 8.0
    if causal:
        s = s.masked_fill(~torch.ones(Lq, Lk, dtype=torch.bool).tril_(), float('-inf'))
    pd = torch.softmax(s, -1) * keep.double() * scale
    return (pd @ vh).permute(0, 2, 1, 3).reshape(ctx, Lq, D)


def _attn_keep(site, ctx, H, qrep, Tk, p):
    return _kernel_mask(SEED, site, 0, ctx * H * qrep * 256, p).reshape(ctx, H, qrep, 256)[..., :Tk]


def _run_attn(q, k, v, do, dq, dk, dv, ctx, qrep, Tk, H, qs, kvs, kvc, causal, site, p, out_shape):
    """One forward + backward through the raw entry points; k / v / dk / dv are ctypes pointers."""
    C = _C()
    out = torch.full(out_shape, NAN, dtype=BF, device=DEV)
    C.check(C.lib().lvl_attn_rows_drop_fwd(C.ptr(q), k, v, C.ptr(out), ctx, qrep, Tk, H, qs, kvs, kvc, causal, SEED, site, p,
                                           C.dtype_code(q), C.stream_ptr()), 'lvl_attn_rows_drop_fwd')
    C.check(C.lib().lvl_attn_rows_drop_bwd(C.ptr(q), k, v, C.ptr(do), C.ptr(dq), dk, dv, ctx, qrep, Tk, H, qs, kvs, kvc, causal,
                                           SEED, site, p, C.dtype_code(q), C.stream_ptr()), 'lvl_attn_rows_drop_bwd')
    torch.cuda.synchronize()
    return out


def _off(t, elements):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + elements * t.element_size())


@pytest.mark.parametrize('p', [0.0, 0.1, 0.5])
@pytest.mark.parametrize('contexts,qrep,H,Tk', [(2, 1, 3, 24), (2, 5, 2, 37), (1, 3, 1, 1), (2, 70, 2, 37), (2, 20, 3, 200),
                                                (3, 12, 12, 256)])
def test_attn_rows_drop_cross(contexts, qrep, H, Tk, p):
    C = _C()
    g = torch.Generator().manual_seed(100 + qrep + Tk)
    D, rows, site = H * 64, contexts * qrep, 13
    q, q64 = _bf((rows, D), g)
    kv, kv64 = _bf((contexts, Tk, 2 * D), g)
    do, do64 = _bf((rows, D), g)
    runs = []
    for _ in range(2):
        dq = torch.full((rows, D), NAN, dtype=BF, device=DEV)
        dkv = torch.full((contexts, Tk, 2 * D), NAN, dtype=BF, device=DEV)
        out = _run_attn(q, C.ptr(kv), _off(kv, D), do, dq, C.ptr(dkv), _off(dkv, D), contexts, qrep, Tk, H, D, 2 * D,
                        Tk * 2 * D, 0, site, p, (rows, D))
        runs.append((out, dq, dkv))
    for a, b in zip(*runs):
        assert torch.equal(a, b) and not torch.isnan(a).any()
    out, dq, dkv = runs[0]
    if p == 0.0:                                         # the bits of the pair without dropout
        out0 = torch.full((rows, D), NAN, dtype=BF, device=DEV)
        dq0, dkv0 = torch.full_like(dq, NAN), torch.full_like(dkv, NAN)
        C.check(C.lib().lvl_cross_attn_rows_fwd(C.ptr(q), C.ptr(kv), C.ptr(out0), rows, qrep, Tk, H, C.dtype_code(q),
                                                C.stream_ptr()), 'lvl_cross_attn_rows_fwd')
        C.check(C.lib().lvl_cross_attn_rows_bwd(C.ptr(q), C.ptr(kv), C.ptr(do), C.ptr(dq0), C.ptr(dkv0), rows, qrep, Tk, H,
                                                C.dtype_code(q), C.stream_ptr()), 'lvl_cross_attn_rows_bwd')
        assert torch.equal(out, out0) and torch.equal(dq, dq0) and torch.equal(dkv, dkv0)
        return
    keep = _attn_keep(site, contexts, H, qrep, Tk, p)
    assert torch.equal(keep, torch.from_numpy(np.ascontiguousarray(R.attn_mask(SEED, site, contexts, H, qrep, Tk, p))))
    q64.requires_grad_(True)
    kv64.requires_grad_(True)
    want = _attn64(q64.reshape(contexts, qrep, D), kv64[..., :D], kv64[..., D:], H, False, keep, float(R.scale(p)))
    want.backward(do64.reshape(contexts, qrep, D))
    r = (_ratio(out, want.detach().reshape(rows, D)), _ratio(dq, q64.grad), _ratio(dkv[..., :D], kv64.grad[..., :D]),
         _ratio(dkv[..., D:], kv64.grad[..., D:]))
    print(f'[attn_rows_drop cross {contexts, qrep, H, Tk} p={p}] worst ratios out {r[0]:.2e} dq {r[1]:.2e} dk {r[2]:.2e} '
          f'dv {r[3]:.2e} (bound {2.0 ** -7:.2e})')
    if Tk == 1:                                          # the softmax is 1: no gradient reaches the scores
        assert (dq == 0).all() and (dkv[..., :D] == 0).all()
    assert max(r) <= 2.0 ** -7, r


@pytest.mark.parametrize('p', [0.0, 0.1, 0.5])
@pytest.mark.parametrize('B,L,H', [(2, 1, 1), (2, 5, 2), (3, 17, 3), (2, 64, 2), (2, 65, 2), (1, 77, 12), (1, 256, 1)])
def test_attn_rows_drop_causal(B, L, H, p):
    from lavila_amd import ops
    g = torch.Generator().manual_seed(500 + L + H)
    D, rows, site = H * 64, B * L, 4
    qkv, qkv64 = _bf((rows, 3 * D), g, 1.5)
    do, do64 = _bf((rows, D), g)
    runs = []
    for _ in range(2):
        dqkv = torch.full((rows, 3 * D), NAN, dtype=BF, device=DEV)
        out = _run_attn(qkv, _off(qkv, D), _off(qkv, 2 * D), do, dqkv, _off(dqkv, D), _off(dqkv, 2 * D), B, L, L, H, 3 * D,
                        3 * D, L * 3 * D, 1, site, p, (rows, D))
        runs.append((out, dqkv))
    for a, b in zip(*runs):
        assert torch.equal(a, b) and not torch.isnan(a).any()
    out, dqkv = runs[0]
    keep = _attn_keep(site, B, H, L, L, p)
    qkv64.requires_grad_(True)
    x = qkv64.reshape(B, L, 3 * D)
    want = _attn64(x[..., :D], x[..., D:2 * D], x[..., 2 * D:], H, True, keep, float(R.scale(p)))
    want.backward(do64.reshape(B, L, D))
    wg = qkv64.grad
    r = (_ratio(out, want.detach().reshape(rows, D)), _ratio(dqkv[:, :D], wg[:, :D]), _ratio(dqkv[:, D:2 * D], wg[:, D:2 * D]),
         _ratio(dqkv[:, 2 * D:], wg[:, 2 * D:]))
    print(f'[attn_rows_drop causal {B, L, H} p={p}] worst ratios out {r[0]:.2e} dq {r[1]:.2e} dk {r[2]:.2e} dv {r[3]:.2e} '
          f'(bound {2.0 ** -7:.2e})')
    if L == 1:
        assert (dqkv[:, :2 * D] == 0).all()
    assert max(r) <= 2.0 ** -7, r
    if p == 0.0:                                         # the text tower's causal kernels, at test_causal_attention_core's tolerance
        xg = qkv.reshape(B, L, 3 * D).clone().requires_grad_(True)
        o = ops.causal_attention(xg, H)
        o.backward(do.reshape(B, L, D))
        _close(out.reshape(B, L, D), o.detach().float().cpu(), BF, 2, 'out vs ops.causal_attention')
        _close(dqkv.reshape(B, L, 3 * D), xg.grad.float().cpu(), BF, 6, 'dqkv vs ops.causal_attention')


def test_attn_rows_drop_single_key_is_exact():
    """Causal L = 1, p = 0.5: the one probability is 1, so a row is exactly 2 v or exactly 0; no gradient reaches q or k."""
    B, H, p, site = 64, 2, 0.5, 9
    D = H * 64
    g = torch.Generator().manual_seed(77)
    qkv, _ = _bf((B, 3 * D), g)
    do, _ = _bf((B, D), g)
    dqkv = torch.full((B, 3 * D), NAN, dtype=BF, device=DEV)
    out = _run_attn(qkv, _off(qkv, D), _off(qkv, 2 * D), do, dqkv, _off(dqkv, D), _off(dqkv, 2 * D), B, 1, 1, H, 3 * D, 3 * D,
                    3 * D, 1, site, p, (B, D))
    keep = _attn_keep(site, B, H, 1, 1, p).reshape(B, H, 1).to(DEV)
    assert 0 < int(keep.sum()) < B * H
    v = qkv[:, 2 * D:].reshape(B, H, 64)
    zero = torch.zeros((), dtype=BF, device=DEV)
    assert torch.equal(out.reshape(B, H, 64), torch.where(keep, 2 * v, zero))
    assert (dqkv[:, :2 * D] == 0).all()                  # all keys dropped or not: dS = P (dP - delta) = 0
    assert torch.equal(dqkv[:, 2 * D:].reshape(B, H, 64), torch.where(keep, 2 * do.reshape(B, H, 64), zero))


# ----------------------------------------------------------------------------------------------------------------------
# 4b. the autograd Functions make the raw calls: one Function per family, with and without `drop`
# ----------------------------------------------------------------------------------------------------------------------
DROP = (SEED, 8, 0.5)


@pytest.mark.parametrize('form,drop', [('gated', None), ('gated', DROP), ('ungated', None), ('ungated', DROP), ('no_y', None)])
def test_gated_add_ln_function_makes_the_raw_calls(form, drop):
    """_GatedAddLnFn, forward and backward, gives the bits of lvl_gated_add_layernorm_train / _bwd without `drop` and of
    _train_drop / _bwd_drop with it, on the same operands; no_y is the first norm of the stack (h alone, no sum kept)."""
    from lavila_amd import gpt2_gated as G
    C = _C()
    lib = C.lib()
    rows, D, eps = 5, 192, 1e-5
    g = torch.Generator().manual_seed(4100)
    res, y, dh, dadd = (_bf((rows, D), g)[0] for _ in range(4))
    y = None if form == 'no_y' else y
    gamma = (1.0 + 0.2 * torch.randn(D, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(D, generator=g)).to(DEV)
    alpha = torch.tensor(0.7, device=DEV) if form == 'gated' else None
    gate = None if alpha is None else torch.tanh(alpha).reshape(1)
    code, tail = C.dtype_code(res), () if drop is None else drop
    s, h = torch.full_like(res, NAN) if y is not None else None, torch.full_like(res, NAN)
    mean, rstd = torch.full((rows,), NAN, device=DEV), torch.full((rows,), NAN, device=DEV)
    fwd = lib.lvl_gated_add_layernorm_train if drop is None else lib.lvl_gated_add_layernorm_train_drop
    C.check(fwd(C.ptr(res), C.ptr(y), C.ptr(gate), C.ptr(gamma), C.ptr(beta), eps, C.ptr(s), C.ptr(h), C.ptr(mean), C.ptr(rstd),
                rows, D, *tail, code, C.stream_ptr()), 'forward')
    kept = res if s is None else s
    ds = torch.full_like(res, NAN)
    dy = torch.full_like(res, NAN) if (gate is not None or drop is not None) else None
    dg, db = torch.full((D,), NAN, device=DEV), torch.full((D,), NAN, device=DEV)
    dgate = torch.full((1,), NAN, device=DEV) if gate is not None else None
    ws = torch.full((lib.lvl_workspace_floats(b'gated_add_layernorm_bwd', rows, D),), NAN, device=DEV)
    bwd = lib.lvl_gated_add_layernorm_bwd if drop is None else lib.lvl_gated_add_layernorm_bwd_drop
    C.check(bwd(C.ptr(dh), C.ptr(kept), C.ptr(y if gate is not None else None), C.ptr(gate), C.ptr(gamma), C.ptr(mean),
                C.ptr(rstd), C.ptr(dadd if y is not None else None), C.ptr(ds), C.ptr(dy), C.ptr(dg), C.ptr(db), C.ptr(dgate),
                C.ptr(ws), rows, D, *tail, code, C.stream_ptr()), 'backward')
    torch.cuda.synchronize()

    ins = [t.clone().requires_grad_(True) if t is not None else None for t in (res, y, alpha, gamma, beta)]
    out = G._GatedAddLnFn.apply(*ins, eps) if drop is None else G._GatedAddLnFn.apply(*ins, eps, drop)
    if y is None:
        assert torch.equal(out, h)
        out.backward(dh)
    else:
        assert torch.equal(out[0], s) and torch.equal(out[1], h)
        torch.autograd.backward(out, (dadd, dh))
    assert not torch.isnan(h).any() and not torch.isnan(ds).any()
    assert torch.equal(ins[0].grad, ds)
    if y is not None:
        assert torch.equal(ins[1].grad, ds if dy is None else dy)       # an ungated add without dropout: dy is ds
    if alpha is not None:
        assert torch.equal(ins[2].grad, (dgate * (1.0 - gate * gate)).reshape(()))
    assert torch.equal(ins[3].grad, dg) and torch.equal(ins[4].grad, db)


@pytest.mark.parametrize('drop', [None, (SEED, 13, 0.5)], ids=['plain', 'p0.5'])
def test_rows_attn_function_makes_the_raw_calls_cross(drop):
    """_RowsAttnFn on the image layout: lvl_cross_attn_rows_fwd / _bwd without `drop`, lvl_attn_rows_drop_fwd / _bwd with it."""
    from lavila_amd import gpt2_gated as G
    C = _C()
    contexts, qrep, H, Tk = 2, 5, 2, 37
    D, rows = H * 64, contexts * qrep
    g = torch.Generator().manual_seed(4200)
    q, kv, do = _bf((rows, D), g)[0], _bf((contexts, Tk, 2 * D), g)[0], _bf((rows, D), g)[0]
    dq, dkv = torch.full_like(q, NAN), torch.full_like(kv, NAN)
    if drop is None:
        out = torch.full((rows, D), NAN, dtype=BF, device=DEV)
        C.check(C.lib().lvl_cross_attn_rows_fwd(C.ptr(q), C.ptr(kv), C.ptr(out), rows, qrep, Tk, H, C.dtype_code(q),
                                                C.stream_ptr()), 'lvl_cross_attn_rows_fwd')
        C.check(C.lib().lvl_cross_attn_rows_bwd(C.ptr(q), C.ptr(kv), C.ptr(do), C.ptr(dq), C.ptr(dkv), rows, qrep, Tk, H,
                                                C.dtype_code(q), C.stream_ptr()), 'lvl_cross_attn_rows_bwd')
        torch.cuda.synchronize()
    else:
        out = _run_attn(q, C.ptr(kv), _off(kv, D), do, dq, C.ptr(dkv), _off(dkv, D), contexts, qrep, Tk, H, D, 2 * D,
                        Tk * 2 * D, 0, drop[1], drop[2], (rows, D))
    qa, kva = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    got = G._RowsAttnFn.apply(qa, kva, qrep, H) if drop is None else G._RowsAttnFn.apply(qa, kva, qrep, H, drop)
    got.backward(do)
    assert not torch.isnan(out).any() and not torch.isnan(dq).any() and not torch.isnan(dkv).any()
    assert torch.equal(got, out) and torch.equal(qa.grad, dq) and torch.equal(kva.grad, dkv)


def test_rows_attn_function_makes_the_raw_calls_causal():
    """_RowsAttnFn without kv: the causal self-attention on qkv through lvl_attn_rows_drop_fwd / _bwd; it needs `drop`."""
    from lavila_amd import gpt2_gated as G
    C = _C()
    B, L, H, site, p = 2, 5, 2, 4, 0.5
    D, rows = H * 64, B * L
    g = torch.Generator().manual_seed(4300)
    qkv, do = _bf((rows, 3 * D), g, 1.5)[0], _bf((rows, D), g)[0]
    dqkv = torch.full_like(qkv, NAN)
    out = _run_attn(qkv, _off(qkv, D), _off(qkv, 2 * D), do, dqkv, _off(dqkv, D), _off(dqkv, 2 * D), B, L, L, H, 3 * D, 3 * D,
                    L * 3 * D, 1, site, p, (rows, D))
    xa = qkv.clone().requires_grad_(True)
    got = G._RowsAttnFn.apply(xa, None, L, H, (SEED, site, p))
    got.backward(do)
    assert not torch.isnan(out).any() and not torch.isnan(dqkv).any()
    assert torch.equal(got, out) and torch.equal(xa.grad, dqkv)
    with pytest.raises(C.HipExtensionError, match='dropout'):
        G._RowsAttnFn.apply(xa, None, L, H)


def test_attn_rows_drop_refuses_more_than_256_keys():
    from lavila_amd import gpt2_gated as G
    C = _C()
    qkv = torch.zeros(257, 192, dtype=BF, device=DEV, requires_grad=True)
    with pytest.raises(C.HipExtensionError, match='256'):
        G._RowsAttnFn.apply(qkv, None, 257, 1, (SEED, 4, 0.1))
    out = torch.zeros(257, 64, dtype=BF, device=DEV)
    with pytest.raises(C.HipExtensionError, match='256'):
        C.check(C.lib().lvl_attn_rows_drop_fwd(C.ptr(qkv), _off(qkv, 64), _off(qkv, 128), C.ptr(out), 1, 257, 257, 1, 192, 192,
                                               257 * 192, 1, SEED, 4, 0.1, C.dtype_code(qkv), C.stream_ptr()), 'fwd')
    with pytest.raises(C.HipExtensionError, match='bf16'):
        qf = torch.zeros(4, 192, device=DEV)
        C.check(C.lib().lvl_attn_rows_drop_fwd(C.ptr(qf), _off(qf, 64), _off(qf, 128), C.ptr(out), 1, 4, 4, 1, 192, 192,
                                               4 * 192, 1, SEED, 4, 0.1, C.dtype_code(qf), C.stream_ptr()), 'fwd')


# ----------------------------------------------------------------------------------------------------------------------
# 5. the training plan
# ----------------------------------------------------------------------------------------------------------------------
def _step_fn(m, video, text, tok):
    from lavila.models.loss import CaptionLoss
    crit = CaptionLoss(tokenizer=tok)

    def step():
        m.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=BF):
            out = m(video, text)
            res = crit(out)
        res['loss'].backward()
        torch.cuda.synchronize()
        return res['loss'].item(), out['text_tokens_logits'].detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}
    return step


def _set_pdrop(m, pdrop):
    for k, v in pdrop.items():
        setattr(m.text_decoder.config, k, v)


@pytest.mark.parametrize('variant', ['freq1_gated', 'freq2_plain'])
def test_narrator_dropout_step_vs_reference(variant, monkeypatch):
    """One bf16 step in .train() under the golden's seed against the unmodified reference's float32 step under the same
    masks, through _compare_step's criterion as test_narrator_end_to_end_training_step applies it."""
    from lavila_amd import gpt2_gated as G
    gold = load_golden('narrator_dropout.pt')
    gv = gold['variants'][variant]
    m, c, d, v, video, tok = _golden_model(variant)
    monkeypatch.setattr(G, 'DECODER_DROPOUT', True)
    _set_pdrop(m, gold['pdrop'])
    m.train()
    assert m.text_decoder.applies_dropout()
    step = _step_fn(m, video, v['text'].to(DEV), tok)

    def picked(got):
        sl = {k: got[k].reshape(got[k].shape[0], -1)[rows] for k, (rows, _) in gv['grad_slices'].items()}
        return {**{k: got[k] for k in gv['grads']}, **sl}

    want = {**{k: t.double() for k, t in gv['grads'].items()}, **{k: t.double() for k, (_, t) in gv['grad_slices'].items()}}
    with G.fixed_dropout_seed(gold['seed']):
        loss, logits, got = step()
        assert set(got) == set(gv['grad_norms'])
        _compare_step(f'narrator dropout step {variant}', picked(got), want, loss, gv['loss'])
        _, logits2, got2 = step()
    assert torch.equal(logits, logits2)
    for k in got:
        assert torch.equal(got[k], got2[k]), k
    with G.fixed_dropout_seed(gold['seed'] ^ 1):          # another mask: the criterion sees it
        loss_o, logits_o, got_o = step()
    assert not torch.equal(logits_o, logits)
    with pytest.raises(AssertionError):
        _compare_step(f'narrator dropout step {variant}, wrong seed', picked(got_o), want, loss_o, gv['loss'])
    # no pinned seed: every forward draws a fresh one from torch's generator, which torch.manual_seed repeats
    torch.manual_seed(1234)
    _, la, _ = step()
    _, lb, _ = step()
    torch.manual_seed(1234)
    _, lc, _ = step()
    assert not torch.equal(la, lb) and torch.equal(la, lc)


def test_switch_hygiene(monkeypatch):
    from lavila_amd import gpt2_gated as G
    gold = load_golden('narrator_dropout.pt')
    m, c, d, v, video, tok = _golden_model('freq1_gated')
    text = v['text'].to(DEV)
    step = _step_fn(m, video, text, tok)
    m.train()
    monkeypatch.setattr(G, 'DECODER_DROPOUT', False)
    off = step()
    monkeypatch.setattr(G, 'DECODER_DROPOUT', True)       # all probabilities 0: exactly the plan without dropout
    on = step()
    assert off[0] == on[0] and torch.equal(off[1], on[1])
    for k in off[2]:
        assert torch.equal(off[2][k], on[2][k]), k
    _set_pdrop(m, gold['pdrop'])
    assert not torch.equal(step()[1], off[1])             # ... and with probabilities it drops

    def infer(eval_mode):
        m.train(not eval_mode)
        with torch.autocast('cuda', dtype=BF):
            if eval_mode:                                  # gradients enabled: the training primitives, not dropping
                return m(video, text)['text_tokens_logits'].detach().clone()
            with torch.no_grad():                          # train mode under no_grad: the inference image
                return m(video, text)['text_tokens_logits'].clone()

    for eval_mode in (True, False):
        monkeypatch.setattr(G, 'DECODER_DROPOUT', True)
        a = infer(eval_mode)
        monkeypatch.setattr(G, 'DECODER_DROPOUT', False)
        assert torch.equal(a, infer(eval_mode))


def test_graphed_train_step_refuses_decoder_dropout(monkeypatch):
    from lavila.models.loss import CaptionLoss
    from lavila_amd import gpt2_gated as G
    from lavila_amd.graph_step import GraphedTrainStep
    m, c, d, v, video, tok = _golden_model('freq1_gated')
    _set_pdrop(m, load_golden('narrator_dropout.pt')['pdrop'])
    m.train()
    monkeypatch.setattr(G, 'DECODER_DROPOUT', True)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, capturable=True)
    with pytest.raises(NotImplementedError, match='decoder dropout'):
        GraphedTrainStep(m, CaptionLoss(tokenizer=tok), opt, tuple(video.shape), tuple(v['text'].shape), DEV)
