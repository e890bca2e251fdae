"""The Linear-layer autograd Functions against the raw calls they stand for, bit for bit.

_LinearFn, _LinearTokenFn, _Conv1DFn, _LmHeadFn, _ClassifierHeadFn, _MlpFn and _MlpResidualLayerNormFn share one routing
rule, one GEMM helper and one backward core (ops._route, _gemm, _linear_backward, _mlp_forward, _mlp_backward). Here every
one of them is run on the shapes of freeze_cases.py (40 rows: one partial tile; 1024 x 256, 320 x 320, 512 x 320, 97 classes)
and its output and every gradient must be torch.equal to the same arithmetic spelled out with linear_tn_raw,
linear_tn_ragged_raw, linear_wgrad_raw, split3, layernorm_apply_raw and a float32 column sum -- the bodies these Functions
had before they shared code. test_gpu_freeze_ops.py pins the launches and the equality between freeze patterns; this file
pins what is launched on what.
"""
import pytest
import torch
import torch.nn.functional as F

import freeze_cases as FC

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROWS = FC.ROWS
BF16, F32 = torch.bfloat16, torch.float32


def _rnd(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *shape, scale=1.0, shift=0.0, dtype=F32: (shift + scale * torch.randn(*shape, generator=g)).to(DEV, dtype)


def _leaf(t):
    return t.requires_grad_(True)


def _copies(w):
    """the bf16 copy [out, in] and its transpose, as ops.weight_copies casts them"""
    wb = w.detach().to(BF16).contiguous()
    return wb, wb.t().contiguous()


def _copies3(w):
    from lavila_amd import ops
    src = w.detach().float().contiguous()
    return ops.split3(src, 1), ops.split3(src.t().contiguous(), 1)


def _wgrad(dy2, x2):
    from lavila_amd import ops
    if dy2.dtype == F32:
        return ops.linear_wgrad_raw(ops.split3(dy2, 0, stack=True), ops.split3(x2, 1, stack=True), False)[0]
    return ops.linear_wgrad_raw(dy2, x2, False)[0]


def _tn(x2, w, bias=None, epilogue=None, aux_in=None):
    """linear_tn_raw, in the f32-class mode for float32 rows (w: the term images)"""
    from lavila_amd import ops
    epilogue = ops.C.EPI_BIAS if epilogue is None else epilogue
    if x2.dtype == F32:
        return ops.linear_tn_raw(ops.split3(x2, 0), w, bias, epilogue, aux_in=aux_in, f32=True)
    return ops.linear_tn_raw(x2, w, bias, epilogue, aux_in=aux_in)


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (what, i, (a.float() - b.float()).abs().max().item())


# ---- _LinearFn --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('recipe', [False, True], ids=['plain', 'recipe'])
@pytest.mark.parametrize('dt', [BF16, F32], ids=['bf16', 'f32'])
def test_linear_fn(dt, recipe):
    from lavila_amd import ops
    r = _rnd(11)
    n_out, n_in = 1024, 256
    x, weight, bias = _leaf(r(ROWS, n_in, dtype=dt)), _leaf(r(n_out, n_in, scale=n_in ** -0.5)), _leaf(r(n_out, scale=0.1))
    gam, bet, dy = r(n_in, scale=0.2, shift=1.0), r(n_in, scale=0.3), r(ROWS, n_out, dtype=dt)
    h, rec = ops.layer_norm(x, gam, bet, 1e-6, recipe=True) if recipe else (x, None)
    y = ops.linear(h, weight, bias, ln=rec)
    got = (y.detach(), *torch.autograd.grad(y, (h, weight, bias), dy))
    with torch.no_grad():
        w, wt = _copies3(weight) if dt == F32 else _copies(weight)
        h2 = h.detach()
        rows = ops.layernorm_apply_raw(*rec.saved()) if recipe else h2
        want = (_tn(h2, w, bias.detach()), _tn(dy, wt), _wgrad(dy, rows), dy.sum(0, dtype=F32))
    _same(got, want, 'linear')


# ---- _LinearTokenFn ---------------------------------------------------------------------------------------------------------
def test_linear_token_fn():
    from lavila_amd import ops
    r = _rnd(12)
    x, weight, xtoken = _leaf(r(ROWS, 256, dtype=BF16)), _leaf(r(1024, 256, scale=1 / 16)), _leaf(r(256))
    dy, dtok = r(ROWS, 1024, dtype=BF16), r(1024)
    y, tok = ops.linear_with_token(x, weight, xtoken)
    assert tok is not None
    got = (y.detach(), *torch.autograd.grad((y, tok), (x, weight, xtoken), (dy, dtok)))
    with torch.no_grad():
        w, wt = _copies(weight)
        want = (_tn(x.detach(), w), _tn(dy, wt), _wgrad(dy, x.detach()), ops.vec_mat(dtok, weight))
    _same(got, want, 'linear_token')


# ---- _Conv1DFn --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_in,n_out', [(256, 1024), (320, 320)], ids=['256', 'ragged320'])
def test_conv1d_fn(n_in, n_out):
    from lavila_amd import gpt2_gated, ops
    r = _rnd(13)
    x, weight, bias = _leaf(r(ROWS, n_in, dtype=BF16)), _leaf(r(n_in, n_out, scale=n_in ** -0.5)), _leaf(r(n_out, scale=0.1))
    dy = r(ROWS, n_out, dtype=BF16)
    y = gpt2_gated._Conv1DFn.apply(x, weight, bias)
    got = (y.detach(), *torch.autograd.grad(y, (x, weight, bias), dy))
    tn = ops.linear_tn_raw if n_out % 256 == 0 else ops.linear_tn_ragged_raw
    with torch.no_grad():
        w_in_out, w_out_in = _copies(weight)
        want = (tn(x.detach(), w_out_in, bias.detach()), tn(dy, w_in_out), _wgrad(x.detach(), dy), dy.sum(0, dtype=F32))
    _same(got, want, 'conv1d')


# ---- _LmHeadFn --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('padded', [False, True], ids=['sliced', 'padded'])
@pytest.mark.parametrize('D', [256, 320], ids=['256', 'ragged320'])
def test_lm_head_fn(D, padded):
    from lavila_amd import gpt2_gated, ops
    r = _rnd(14)
    V, Vp = 300, 512
    h, weight = _leaf(r(ROWS, D, dtype=BF16)), _leaf(r(V, D, scale=D ** -0.5))
    dlogits = r(ROWS, Vp if padded else V, dtype=BF16)
    y = gpt2_gated._LmHeadFn.apply(h, weight, padded)
    got = (y.detach(), *torch.autograd.grad(y, (h, weight), dlogits))
    with torch.no_grad():
        w = torch.cat([weight.detach().to(BF16), torch.zeros(Vp - V, D, dtype=BF16, device=DEV)])
        full = ops.linear_tn_raw(h.detach(), w)
        dl = torch.zeros(ROWS, Vp, dtype=BF16, device=DEV)
        dl[:, :dlogits.shape[1]] = dlogits
        dh = (ops.linear_tn_raw if D % 256 == 0 else ops.linear_tn_ragged_raw)(dl, w.t().contiguous())
        want = (full if padded else full[:, :V], dh, _wgrad(dl, h.detach())[:V])
    _same(got, want, 'lm_head')


# ---- _ClassifierHeadFn ------------------------------------------------------------------------------------------------------
def test_classifier_head_fn():
    from lavila_amd import models, ops
    r = _rnd(15)
    n, D = 97, 256
    x, weight, bias = _leaf(r(ROWS, D, dtype=BF16)), _leaf(r(n, D, scale=1 / 16)), _leaf(r(n, scale=0.1))
    dlogits = r(ROWS, n, dtype=BF16)
    y = models._ClassifierHeadFn.apply(x, weight, bias)
    got = (y.detach(), *torch.autograd.grad(y, (x, weight, bias), dlogits))
    with torch.no_grad():
        w = F.pad(weight.detach().to(BF16), (0, 0, 0, 256 - n))
        dl = F.pad(dlogits, (0, 256 - n))
        want = (ops.linear_tn_raw(x.detach(), w, F.pad(bias.detach(), (0, 256 - n)))[:, :n],
                ops.linear_tn_raw(dl, w.t().contiguous())[:, :D], _wgrad(dl, x.detach())[:n], dlogits.sum(0, dtype=F32))
    _same(got, want, 'classifier_head')


# ---- _MlpFn, _MlpResidualLayerNormFn ----------------------------------------------------------------------------------------
def _mlp_reference(ops, act, h2, rec, w1, b1, w2, b2=None, res2=None):
    """The two GEMMs and the backward of fc2(act(fc1(h2) + b1)) from raw calls: bf16 keeps act'(u) unless selective (rec),
    float32 keeps u. Returns y and backward(dy2) -> (dx, dw1, db1, dw2) for the gradient dy2 of fc2's output."""
    C = ops.C
    keep_u, keep_deriv, bwd_on_u = {'quickgelu': (C.EPI_BIAS_QUICKGELU, C.EPI_BIAS_QUICKGELU_DERIV, C.EPI_QUICKGELU_BWD),
                                    'gelu': (C.EPI_BIAS_GELU, C.EPI_BIAS_GELU_DERIV, C.EPI_GELU_BWD)}[act]
    on_u = h2.dtype == F32 or rec is not None
    (w1b, w1t), (w2b, w2t) = (_copies3(w) if h2.dtype == F32 else _copies(w) for w in (w1, w2))
    a, u = _tn(h2, w1b, b1.detach(), keep_u if on_u else keep_deriv)
    y = _tn(a, w2b) if res2 is None else _tn(a, w2b, b2.detach(), C.EPI_BIAS_RESIDUAL, aux_in=res2)

    def backward(dy2):
        du, db1 = _tn(dy2, w2t, None, bwd_on_u if on_u else C.EPI_MUL_AUX_COLSUM, aux_in=u)
        act_rows = a if rec is None else (ops.quickgelu_apply_raw(u) if act == 'quickgelu' else ops.gelu_apply_raw(u))
        dw2 = _wgrad(dy2, act_rows)
        dx = _tn(du, w1t)
        dw1 = _wgrad(du, h2 if rec is None else ops.layernorm_apply_raw(*rec.saved()))
        return dx, dw1, db1, dw2
    return y, backward


MLP_CASES = [(BF16, False), (BF16, True), (F32, False)]
MLP_IDS = ['bf16', 'bf16-selective', 'f32']


def _mlp_leaves(r, dt):
    D, Hd = 256, 1024
    return (_leaf(r(ROWS, D, dtype=dt)), _leaf(r(Hd, D, scale=D ** -0.5)), _leaf(r(Hd, scale=0.5)), _leaf(r(D, Hd, scale=Hd ** -0.5)),
            r(D, scale=0.2, shift=1.0), r(D, scale=0.3))


@pytest.mark.parametrize('dt,sel', MLP_CASES, ids=MLP_IDS)
@pytest.mark.parametrize('act', ['quickgelu', 'gelu'])
def test_mlp_fn(act, dt, sel):
    from lavila_amd import ops
    r = _rnd(16)
    x, w1, b1, w2, gam, bet = _mlp_leaves(r, dt)
    dy = r(ROWS, 256, dtype=dt)
    h, rec = ops.layer_norm(x, gam, bet, 1e-6, recipe=True) if sel else (x, None)
    y = ops.mlp(h, w1, b1, w2, act, ln=rec)
    got = (y.detach(), *torch.autograd.grad(y, (h, w1, b1, w2), dy))
    with torch.no_grad():
        y_ref, backward = _mlp_reference(ops, act, h.detach(), rec, w1, b1, w2)
        want = (y_ref, *backward(dy))
    _same(got, want, 'mlp')


@pytest.mark.parametrize('sel', [False, True], ids=['plain', 'selective'])
@pytest.mark.parametrize('act', ['quickgelu', 'gelu'])
def test_mlp_residual_layer_norm_fn(act, sel):
    from lavila_amd import ops
    r = _rnd(17)
    x, w1, b1, w2, gam, bet = _mlp_leaves(r, BF16)
    b2, res = _leaf(r(256, scale=0.5)), _leaf(r(ROWS, 256, dtype=BF16))
    gamma, beta = _leaf(r(256, scale=0.2, shift=1.0)), _leaf(r(256, scale=0.3))
    ds, dh = r(ROWS, 256, dtype=BF16), r(ROWS, 256, dtype=BF16)
    h, rec = ops.layer_norm(x, gam, bet, 1e-6, recipe=True) if sel else (x, None)
    out = ops.mlp_residual_layer_norm(h, w1, b1, w2, b2, res, gamma, beta, 1e-6, ln=rec, act=act)
    assert out is not None
    got = (out[0].detach(), out[1].detach(),
           *torch.autograd.grad(out, (h, w1, b1, w2, b2, res, gamma, beta), (ds, dh)))
    with torch.no_grad():
        s, backward = _mlp_reference(ops, act, h.detach(), rec, w1, b1, w2, b2, res.detach())
        hn, _, mean, rstd = ops.layernorm_fwd_raw(s, None, None, gamma.detach(), beta.detach(), 1e-6, False)
        dsum, dg, dbeta, dcol = ops.layernorm_bwd_raw(dh, s, None, None, gamma.detach(), mean, rstd, ds, True)
        dx, dw1, db1, dw2 = backward(dsum)
        want = (s, hn, dx, dw1, db1, dw2, dcol, dsum, dg, dbeta)
    _same(got, want, 'mlp_residual_layer_norm')
