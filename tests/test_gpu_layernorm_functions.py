"""The LayerNorm autograd Functions against the raw calls they stand for, bit for bit, and against their recorded C calls.

_LayerNormFn, _AddLayerNormFn, _AddLayerNormPassFn, _LinearResidualLayerNormFn and _MlpResidualLayerNormFn share one forward
core and one backward core (ops._ln_forward, ops._ln_backward). Here every public form that reaches them runs on every case
of layernorm_function_cases.py, and

  * every output and every gradient must be torch.equal to the same arithmetic spelled out with layernorm_fwd_raw,
    layernorm_fwd_mixed_raw, layernorm_bwd_raw, layernorm_bwd_mixed_raw (the GEMM forms: with linear_tn_raw, linear_wgrad_raw
    and vec_mat too) -- the bodies these Functions had before they shared code; with recipe=True the rows rebuilt by
    layernorm_apply_raw from the recipe must equal the form's own output;
  * the C-ABI calls of the forward and of the backward must equal tests/golden/layernorm_call_plans.json
    (tools/gen_layernorm_call_plans.py, recorded before the Functions shared code): same kernels, same order, same operands.

A first output nothing consumes still hands its Function a gradient: autograd materialises zeros. The spelled-out arithmetic
passes those zeros where the Function does.
"""
import os

import pytest
import torch

import layernorm_function_cases as LC
from cabi_recorder import Recorder, load_plans
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
EPS = LC.EPS


def _p32(p):
    return None if p is None else p.float().contiguous()


def _same(got, want, what):
    assert list(got) == list(want), (what, list(got), list(want))
    for k in got:
        a, b = got[k], want[k]
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), \
            (what, k, a.dtype, b.dtype, (a.float() - b.float()).abs().max().item())


def _plain_forms(ops, r):
    """layer_norm, add_layer_norm, add_layer_norm_pass from the four raw launchers: ({output or gradient: tensor}, the
    operands the recipe must hold)."""
    c, t, (dfirst, dh) = r['case'], r['leaves'], r['cot']
    mixed = c['dt'] == 'mixed'
    fwd = ops.layernorm_fwd_mixed_raw if mixed else ops.layernorm_fwd_raw
    g, b = _p32(t['weight']), _p32(t['bias'])
    if c['form'] == 'layer_norm':
        x = t['x']
        h, _, mean, rstd = fwd(x, None, None, g, b, EPS, False)
        bwd = ops.layernorm_bwd_mixed_raw if mixed else ops.layernorm_bwd_raw
        dx, dg, db = bwd(dh, x, None, None, g, mean, rstd, None, False)[:3]
        return dict(h=h, x=dx, weight=dg.to(t['weight'].dtype), bias=db.to(t['bias'].dtype)), (x, None, None)
    res, y, yb = t['res'], t['y'], _p32(t.get('ybias'))
    if c['form'] == 'add_layer_norm':
        h, s, mean, rstd = fwd(res, y, yb, g, b, EPS, c['keep_sum'])
        operands = (s, None, None) if c['keep_sum'] else (res, y, yb)
        dadd = (dfirst if c['dstream'] else torch.zeros_like(s)) if c['keep_sum'] else None
        if mixed:
            dx, dg, db, colsum, dy = ops.layernorm_bwd_mixed_raw(dh, *operands, g, mean, rstd, dadd, c['ybias'], want_dx2=True)
        else:
            dx, dg, db, colsum = ops.layernorm_bwd_raw(dh, *operands, g, mean, rstd, dadd, c['ybias'])
            dy = dx
        want = dict(s=s, h=h) if c['keep_sum'] else dict(h=h)
    else:
        h, _, mean, rstd = fwd(res, y, yb, g, b, EPS, False)
        operands = (res, y, yb)
        dadd = dfirst if c['dstream'] else torch.zeros_like(res)
        want_sum = c['ybias'] or c['token']
        if mixed:
            dx, dg, db, colsum, dy = ops.layernorm_bwd_mixed_raw(dh, *operands, g, mean, rstd, dadd, want_sum, want_dx2=True,
                                                                 plain=True)
        else:
            dx, dg, db, colsum, dy = ops.layernorm_bwd_raw(dh, *operands, g, mean, rstd, dadd, want_sum, want_plain=True)
        want = dict(s=res, h=h)
    want.update(res=dx, y=dy)
    if c['ybias']:
        want['ybias'] = colsum.to(t['ybias'].dtype)
    want.update(weight=dg.to(t['weight'].dtype), bias=db.to(t['bias'].dtype))
    if c['token']:
        want['ytoken'] = colsum
    return want, operands


def _gemm_forms(ops, r):
    """linear_residual_layer_norm and mlp_residual_layer_norm (QuickGELU; bf16 keeps act'(u), selective keeps u) from
    linear_tn_raw, linear_wgrad_raw, vec_mat and the plain LayerNorm launchers."""
    C = ops.C
    c, t, (dfirst, dh) = r['case'], r['leaves'], r['cot']
    copies = lambda w: (w.to(BF16).contiguous(), w.to(BF16).t().contiguous())
    wgrad = lambda dy2, x2: ops.linear_wgrad_raw(dy2, x2, False)[0]
    res, g, b = t['res'], t['gamma'], t['beta']
    mlp = c['form'] == 'mlp_residual_layer_norm'
    x2 = r['wrt']['x']
    if mlp:
        on_u = c['selective']
        (w1b, w1t), (w2b, w2t) = copies(t['w1']), copies(t['w2'])
        a, u = ops.linear_tn_raw(x2, w1b, t['b1'], C.EPI_BIAS_QUICKGELU if on_u else C.EPI_BIAS_QUICKGELU_DERIV)
        s = ops.linear_tn_raw(a, w2b, t.get('b2'), C.EPI_BIAS_RESIDUAL, aux_in=res)
    else:
        w, wt = copies(t['weight'])
        s = ops.linear_tn_raw(x2, w, t.get('lbias'), C.EPI_BIAS_RESIDUAL, aux_in=res)
    h, _, mean, rstd = ops.layernorm_fwd_raw(s, None, None, g, b, EPS, False)
    dadd = dfirst if c['dstream'] else torch.zeros_like(s)
    ds, dg, dbeta, colsum = ops.layernorm_bwd_raw(dh, s, None, None, g, mean, rstd, dadd, c['ybias'] or c['token'])
    if mlp:
        du, db1 = ops.linear_tn_raw(ds, w2t, None, C.EPI_QUICKGELU_BWD if on_u else C.EPI_MUL_AUX_COLSUM, aux_in=u)
        dw2 = wgrad(ds, ops.quickgelu_apply_raw(u) if on_u else a)
        rows = x2
        if on_u:        # x2 is the LayerNorm output of the leaf: fc1's weight gradient reads the rows rebuilt from its recipe
            x0, gam, bet = t['x'], r['consts']['gam'], r['consts']['bet']
            rows = ops.layernorm_apply_raw(x0, None, None, gam, bet, *ops.layernorm_fwd_raw(x0, None, None, gam, bet, EPS, False)[2:])
        want = dict(s=s, h=h, x=ops.linear_tn_raw(du, w1t), w1=wgrad(du, rows), b1=db1, w2=dw2)
        if c['ybias']:
            want['b2'] = colsum
        want.update(res=ds, gamma=dg, beta=dbeta)
    else:
        want = dict(s=s, h=h, x=ops.linear_tn_raw(ds, wt), weight=wgrad(ds, x2))
        if c['ybias']:
            want['lbias'] = colsum
        want.update(res=ds, gamma=dg, beta=dbeta)
        if c['token']:
            want['xtoken'] = ops.vec_mat(colsum, t['weight'])
    return want, (s, None, None)


@pytest.fixture(scope='module')
def plans():
    return load_plans(os.path.join(GOLDEN, 'layernorm_call_plans.json'))


def test_the_recorded_file_holds_exactly_the_matrix(plans):
    assert list(plans) == list(LC.CASES)


def test_the_matrix_crosses_what_the_functions_branch_on():
    cases = list(LC.CASES.values())
    forms = {c['form'] for c in cases}
    assert forms == {'layer_norm', 'add_layer_norm', 'add_layer_norm_pass', 'linear_residual_layer_norm', 'mlp_residual_layer_norm'}
    for form in ('layer_norm', 'add_layer_norm', 'add_layer_norm_pass'):
        assert {(c['dt'], c['cols']) for c in cases if c['form'] == form} == {(d, n) for d in ('bf16', 'f32', 'mixed') for n in (768, 320)}
    for form in forms - {'layer_norm'}:
        for flag in ('ybias', 'dstream', 'recipe'):
            assert {c[flag] for c in cases if c['form'] == form} == {False, True}, (form, flag)
    assert {c['keep_sum'] for c in cases if c['form'] == 'add_layer_norm'} == {False, True}
    for form in ('add_layer_norm_pass', 'linear_residual_layer_norm'):
        assert {c['token'] for c in cases if c['form'] == form} == {False, True}
    assert LC.ROWS == 37 and LC.GEMM_ROWS == 40


@pytest.mark.parametrize('name', list(LC.CASES))
def test_form_equals_its_raw_calls(name):
    from lavila_amd import ops
    r = LC.run(name)
    c = r['case']
    with torch.no_grad():
        plain = c['form'] in ('layer_norm', 'add_layer_norm', 'add_layer_norm_pass')
        want, operands = (_plain_forms if plain else _gemm_forms)(ops, r)
        got = dict(zip(('s', 'h') if len(r['outs']) == 2 else ('h',), r['outs']))
        got.update(r['grads'])
        _same(got, want, name)
        if c['recipe']:
            x, x2, xbias, gamma, beta, mean, rstd = r['rec'].saved()
            for kept, operand in zip((x, x2, xbias), operands):
                assert (kept is None) == (operand is None) and (kept is None or torch.equal(kept, operand)), name
            if x2 is not None and x2.dtype != x.dtype:      # the mixed pair: the float32 kernel between a widening and one rounding
                x2 = x2.float()
            rebuilt = ops.layernorm_apply_raw(x, x2, xbias, gamma, beta, mean, rstd)
            assert torch.equal(rebuilt.to(want['h'].dtype).reshape(want['h'].shape), want['h']), name
        else:
            assert r['rec'] is None


@pytest.mark.parametrize('name', list(LC.CASES))
def test_form_makes_the_recorded_calls(name, plans, monkeypatch):
    rec = Recorder(monkeypatch)
    LC.run(name, rec)
    for phase, got in (('forward', rec.forward), ('backward', rec.backward)):
        want = plans[name][phase]
        assert any(call[0].startswith('lvl_layernorm_') for call in got), f'{name}: no LayerNorm kernel in the {phase}'
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, f'{name}: {phase} call {i} is {g}, recorded {w}'
        assert len(got) == len(want), f'{name}: {len(got)} {phase} calls, recorded {len(want)}: {[call[0] for call in got]}'
