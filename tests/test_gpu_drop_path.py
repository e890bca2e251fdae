"""GPU (-m gpu): the stochastic-depth kernel pair lvl_droppath_add_layernorm_fwd / _bwd through the C ABI.

  s = res + c_b * (y + ybias), h = LayerNorm(s); one c_b per sample, row r belongs to sample r // rows_per_sample.

What is exact is asserted exactly: scale = 1 reproduces lvl_layernorm_fwd(res, y, ybias) to the bit, scale = 0 leaves s = res
and the plain LayerNorm of res, ds / dgamma / dbeta equal lvl_layernorm_bwd on the same operands, dy equals ds where c = 1 and
is 0 where c = 0, every backward is deterministic. The rest is compared with float64:
  * s without a bias is one fma and one rounding to the stored type: |s - s64| <= 2^-8 |s64| (bf16), 2^-23 |s64| (f32);
  * s with a bias is two fmas (v = fma(c, y, res); v = fma(c, bias, v)): each rounds to f32 at the magnitude of its own result,
    which the cancellation of the second add can leave far above |s64|, so the bound there is the stored type's half ulp of
    s64 plus 2 * 2^-24 * (|res| + |c y| + |c bias|);
  * h within the error model of rowops_reference.ln_fwd_bounds for the stored (rounded) sum, as test_gpu_rowops_at_scale.py;
  * dy against c * (the stored ds in float64): 2^-7 relative in bf16 (two roundings: a fused backward would round c * ds
    from the unrounded ds), one f32 ulp in f32;
  * dysum against the float64 column sums of the stored dy within rows * 2^-24 * sum |dy|.
Widths: 768 (exact-width instantiation, W = 4), 1024 (the wider one), 128 (narrow: idle lanes), 520 (general). In bf16 the
backward of 768 and 1024 columns is the fused LayerNorm-backward instantiation; float32 and the other widths run the composed
form (lvl_layernorm_bwd, then the dy pass): the same assertions hold for both. Rows: several
samples of 33 rows, one row per sample, 785 rows, one sample of 4099 rows (past the 3072-row sweep of the backward grids), and
4 x 3137 rows of 768 (past the 12288-row sweep of the forward grid)."""
import pytest
import torch

import rowops_reference as R
from test_gpu_rowops_at_scale import _p, _within
from test_gpu_selective_recompute import _poison

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = (torch.bfloat16, torch.float32)
COLS = (768, 1024, 128, 520)
SHAPES = ((5, 33), (5, 1), (3, 785), (2, 4099))
CASES = [(cols, smp, rps) for cols in COLS for smp, rps in SHAPES] + [(768, 4, 3137)]
EPS = 1e-6
U_STORE = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -23}


def _C():
    from lavila_amd import _cabi as C
    return C


def _mixed(samples):
    """Scale vectors with a dropped sample, a kept one at 1 / keep, a plain 1 and a factor outside {0, 1 / keep}."""
    full = [0.0, 1 / 0.9, 2.0, 0.0, 1.0]
    if samples >= 5:
        return [full[:samples] if samples == 5 else (full * samples)[:samples]]
    if samples == 2:
        return [[0.0, 1 / 0.9], [2.0, 1.0]]
    return [(full[:samples - 1] + [1.0])]


def _inputs(cols, samples, rps, dt, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rows = samples * rps
    res = (2 * torch.randn(rows, cols, generator=g, device=DEV) + 0.5).to(dt)
    y = torch.randn(rows, cols, generator=g, device=DEV).to(dt)
    bias = 0.1 * torch.randn(cols, generator=g, device=DEV)
    gamma = 1 + 0.2 * torch.randn(cols, generator=g, device=DEV)
    beta = 0.1 * torch.randn(cols, generator=g, device=DEV)
    return res, y, bias, gamma, beta


def _dp_fwd(res, y, bias, scale, gamma, beta, rps):
    C = _C()
    rows, cols = res.shape
    s, h = torch.full_like(res, float('nan')), torch.full_like(res, float('nan'))
    mean = torch.full((rows,), float('nan'), device=DEV)
    rstd = torch.full((rows,), float('nan'), device=DEV)
    C.check(C.lib().lvl_droppath_add_layernorm_fwd(_p(res), _p(y), _p(bias), _p(scale), _p(gamma), _p(beta), _p(s), _p(h),
                                                   _p(mean), _p(rstd), rows, rps, cols, EPS, C.dtype_code(res),
                                                   C.stream_ptr()), 'lvl_droppath_add_layernorm_fwd')
    return s, h, mean, rstd


def _ln_fwd(x, x2, bias, gamma, beta, keep):
    C = _C()
    rows, cols = x.shape
    s = torch.full_like(x, float('nan')) if keep else None
    h = torch.full_like(x, float('nan'))
    mean = torch.full((rows,), float('nan'), device=DEV)
    rstd = torch.full((rows,), float('nan'), device=DEV)
    C.check(C.lib().lvl_layernorm_fwd(_p(x), _p(x2), _p(bias), _p(gamma), _p(beta), _p(s), _p(h), _p(mean), _p(rstd), rows,
                                      cols, EPS, C.dtype_code(x), C.stream_ptr()), 'lvl_layernorm_fwd')
    return s, h, mean, rstd


def _dp_bwd(dh, s, gamma, mean, rstd, scale, dadd, rps, want_sum=True):
    C = _C()
    rows, cols = s.shape
    ds, dy = torch.full_like(s, float('nan')), torch.full_like(s, float('nan'))
    dgamma, dbeta = (torch.full((cols,), float('nan'), device=DEV) for _ in range(2))
    dysum = torch.full((cols,), float('nan'), device=DEV) if want_sum else None
    n = int(C.lib().lvl_workspace_floats(b'droppath_add_layernorm_bwd', rows, cols))
    assert n > int(C.lib().lvl_workspace_floats(b'layernorm_bwd', rows, cols))
    ws = torch.full((n,), float('nan'), device=DEV)
    C.check(C.lib().lvl_droppath_add_layernorm_bwd(_p(dh), _p(s), _p(gamma), _p(mean), _p(rstd), _p(scale), _p(dadd), _p(ds),
                                                   _p(dy), _p(dgamma), _p(dbeta), _p(dysum), _p(ws), rows, rps, cols,
                                                   C.dtype_code(s), C.stream_ptr()), 'lvl_droppath_add_layernorm_bwd')
    return ds, dy, dgamma, dbeta, dysum


def _ln_bwd(dh, s, gamma, mean, rstd, dadd):
    C = _C()
    rows, cols = s.shape
    dx = torch.full_like(s, float('nan'))
    dgamma, dbeta = (torch.full((cols,), float('nan'), device=DEV) for _ in range(2))
    ws = torch.full((int(C.lib().lvl_workspace_floats(b'layernorm_bwd', rows, cols)),), float('nan'), device=DEV)
    C.check(C.lib().lvl_layernorm_bwd(_p(dh), _p(s), None, None, _p(gamma), _p(mean), _p(rstd), _p(dadd), _p(dx), None,
                                      _p(dgamma), _p(dbeta), None, _p(ws), rows, cols, C.dtype_code(s), C.stream_ptr()),
            'lvl_layernorm_bwd')
    return dx, dgamma, dbeta


def _ids(v):
    return str(v)[6:] if isinstance(v, torch.dtype) else None


@pytest.mark.parametrize('dt', DTYPES, ids=_ids)
@pytest.mark.parametrize('cols,samples,rps', CASES)
def test_forward_unit_and_zero_scale_are_exact(cols, samples, rps, dt):
    res, y, bias, gamma, beta = _inputs(cols, samples, rps, dt, seed=cols + rps)
    for b in (bias, None):
        ones = torch.ones(samples, device=DEV)
        got = _dp_fwd(res, y, b, ones, gamma, beta, rps)
        want = _ln_fwd(res, y, b, gamma, beta, keep=True)
        for name, a, w in zip(('s', 'h', 'mean', 'rstd'), got, want):
            assert torch.equal(a, w), f'scale 1, {name}: not lvl_layernorm_fwd(res, y, ybias) to the bit'
        s, h, _, _ = _dp_fwd(res, y, b, torch.zeros(samples, device=DEV), gamma, beta, rps)
        assert torch.equal(s, res), 'scale 0: s is not res'
        assert torch.equal(h, _ln_fwd(res, None, None, gamma, beta, keep=False)[1]), 'scale 0: h is not LayerNorm(res)'


@pytest.mark.parametrize('dt', DTYPES, ids=_ids)
@pytest.mark.parametrize('cols,samples,rps', CASES)
def test_forward_mixed_scale_against_float64(cols, samples, rps, dt):
    res, y, bias, gamma, beta = _inputs(cols, samples, rps, dt, seed=3 * cols + rps)
    tag = f' [{str(dt)[6:]} cols={cols} samples={samples} x {rps}]'
    for vec in _mixed(samples):
        scale = torch.tensor(vec, dtype=torch.float32, device=DEV)
        c = scale.double().repeat_interleave(rps)[:, None]
        for b in (None, bias):
            s, h, mean, rstd = _dp_fwd(res, y, b, scale, gamma, beta, rps)
            cy = c * y.double()
            s64 = res.double() + cy if b is None else res.double() + c * (y.double() + b.double())
            err = (s.double() - s64).abs()
            if b is None:
                bound = U_STORE[dt] * s64.abs()
            else:
                bound = R.U_OUT[dt] * s64.abs() + 2 * R.U * (res.double().abs() + cy.abs() + (c * b.double()).abs())
            worst = (err / bound.clamp_min(1e-300)).max().item()
            print(f'[droppath fwd{tag} bias={b is not None} scale={vec}] worst |s - s64| / bound {worst:.3g}')
            assert bool((err <= bound).all()), f's beyond its bound{tag}: worst ratio {worst:.3g}'
            dropped = (c[:, 0] == 0)
            assert torch.equal(s[dropped], res[dropped]), f'rows of a zero-scale sample differ from res{tag}'
            st = s.double()                  # the kernel normalises the rounded sum it stored
            h64, mu64, rs64 = R.ln_fwd_ref(st, gamma, beta, EPS)
            eh, emu, ers = R.ln_fwd_bounds(st, st.abs(), 0, gamma, beta, EPS, cols, dt)
            _within(f'droppath h {str(dt)[6:]}', h, h64, eh, tag)
            _within('droppath mean', mean, mu64, emu, tag)
            _within('droppath rstd', rstd, rs64, ers, tag)


def _bwd_operands(cols, samples, rps, dt, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rows = samples * rps
    s = (2 * torch.randn(rows, cols, generator=g, device=DEV) + 0.5).to(dt)
    dh = torch.randn(rows, cols, generator=g, device=DEV).to(dt)
    dadd = torch.randn(rows, cols, generator=g, device=DEV).to(dt)
    gamma = 1 + 0.2 * torch.randn(cols, generator=g, device=DEV)
    beta = torch.zeros(cols, device=DEV)
    _, _, mean, rstd = _ln_fwd(s, None, None, gamma, beta, keep=False)
    return s, dh, dadd, gamma, mean, rstd


@pytest.mark.parametrize('with_dadd', [False, True], ids=['plain', 'dadd'])
@pytest.mark.parametrize('dt', DTYPES, ids=_ids)
@pytest.mark.parametrize('cols,samples,rps', CASES)
def test_backward(cols, samples, rps, dt, with_dadd):
    s, dh, dadd, gamma, mean, rstd = _bwd_operands(cols, samples, rps, dt, seed=5 * cols + rps)
    dadd = dadd if with_dadd else None
    rows = samples * rps
    tag = f' [{str(dt)[6:]} cols={cols} samples={samples} x {rps} dadd={with_dadd}]'
    want_dx, want_dg, want_db = _ln_bwd(dh, s, gamma, mean, rstd, dadd)
    for vec in _mixed(samples):
        scale = torch.tensor(vec, dtype=torch.float32, device=DEV)
        runs = []
        for rep in range(3):
            if rep:
                _poison()
            runs.append(_dp_bwd(dh, s, gamma, mean, rstd, scale, dadd, rps))
            torch.cuda.synchronize()
        for other in runs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(runs[0], other)), f'backward is not deterministic{tag}'
        ds, dy, dgamma, dbeta, dysum = runs[0]
        assert torch.equal(ds, want_dx) and torch.equal(dgamma, want_dg) and torch.equal(dbeta, want_db), \
            f'ds / dgamma / dbeta are not lvl_layernorm_bwd\'s{tag}'
        c = scale.repeat_interleave(rps)
        assert torch.equal(dy[c == 1], ds[c == 1]), f'dy != ds where c = 1{tag}'
        assert bool((dy[c == 0] == 0).all()), f'dy != 0 where c = 0{tag}'
        want = c.double()[:, None] * ds.double()
        err = (dy.double() - want).abs()
        if dt == torch.bfloat16:
            bound = 2.0 ** -7 * want.abs()
        else:                       # one f32 ulp of the result
            bound = torch.maximum(2.0 ** -23 * want.abs(), torch.full_like(want, 2.0 ** -149))
        worst = (err / bound.clamp_min(1e-300)).max().item()
        assert bool((err <= bound).all()), f'dy beyond its bound{tag}: worst ratio {worst:.3g}'
        sum64 = dy.double().sum(0)
        sbound = rows * 2.0 ** -24 * dy.double().abs().sum(0)
        serr = (dysum.double() - sum64).abs()
        print(f'[droppath bwd{tag} scale={vec}] dy worst ratio {worst:.3g}; dysum worst '
              f'{(serr / sbound.clamp_min(1e-300)).max().item():.3g} of its bound')
        assert bool((serr <= sbound).all()), f'dysum beyond the f32 accumulation bound{tag}'
        # the sums are optional: without them the other outputs do not change
        again = _dp_bwd(dh, s, gamma, mean, rstd, scale, dadd, rps, want_sum=False)
        assert again[4] is None and all(torch.equal(a, b) for a, b in zip(again[:4], runs[0][:4]))


@pytest.mark.parametrize('dt', DTYPES, ids=_ids)
def test_zero_rows(dt):
    cols = 768
    C = _C()
    empty = torch.empty(0, cols, dtype=dt, device=DEV)
    gamma, beta = torch.ones(cols, device=DEV), torch.zeros(cols, device=DEV)
    none = torch.empty(0, device=DEV)
    C.check(C.lib().lvl_droppath_add_layernorm_fwd(_p(empty), _p(empty), None, _p(none), _p(gamma), _p(beta), _p(empty),
                                                   _p(empty), _p(none), _p(none), 0, 7, cols, EPS, C.dtype_code(empty),
                                                   C.stream_ptr()), 'lvl_droppath_add_layernorm_fwd')
    ds, dy, dgamma, dbeta, dysum = _dp_bwd(empty, empty, gamma, none, none, none, None, 7)
    torch.cuda.synchronize()
    for t in (dgamma, dbeta, dysum):
        assert bool((t == 0).all())


def test_refuses_rows_that_do_not_divide():
    C = _C()
    x = torch.zeros(10, 768, dtype=torch.bfloat16, device=DEV)
    v = torch.zeros(768, device=DEV)
    st = torch.zeros(10, device=DEV)
    with pytest.raises(C.HipExtensionError, match='rows_per_sample'):
        C.check(C.lib().lvl_droppath_add_layernorm_fwd(_p(x), _p(x), None, _p(st), _p(v), _p(v), _p(x.clone()), _p(x.clone()),
                                                       _p(st.clone()), _p(st.clone()), 10, 3, 768, EPS, C.dtype_code(x),
                                                       C.stream_ptr()), 'lvl_droppath_add_layernorm_fwd')


@pytest.mark.parametrize('dt', DTYPES, ids=_ids)
def test_graph_capture_and_replay_equal_eager(dt):
    cols, samples, rps = 768, 5, 33
    res, y, bias, gamma, beta = _inputs(cols, samples, rps, dt, seed=77)
    scale = torch.tensor(_mixed(samples)[0], dtype=torch.float32, device=DEV)
    dh = torch.randn(samples * rps, cols, device=DEV).to(dt)
    dadd = torch.randn(samples * rps, cols, device=DEV).to(dt)

    def both():
        s, h, mean, rstd = _dp_fwd(res, y, bias, scale, gamma, beta, rps)
        return (s, h, mean, rstd) + _dp_bwd(dh, s, gamma, mean, rstd, scale, dadd, rps)
    eager = both()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = both()
    for t in static:
        t.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, static):
        assert torch.equal(a, b)


def test_ops_function_gradients():
    """ops.scaled_add_layer_norm: both outputs used, d scale is None, d ybias = column sums of dy, the token slot returns
    them too."""
    from lavila_amd import ops
    g = torch.Generator(device=DEV).manual_seed(9)
    B, T, D = 5, 33, 256
    res = torch.randn(B, T, D, generator=g, device=DEV).bfloat16().requires_grad_(True)
    y = torch.randn(B, T, D, generator=g, device=DEV).bfloat16().requires_grad_(True)
    yb = (0.1 * torch.randn(D, generator=g, device=DEV)).requires_grad_(True)
    w = (1 + 0.1 * torch.randn(D, generator=g, device=DEV)).requires_grad_(True)
    b = torch.zeros(D, device=DEV, requires_grad=True)
    tok = torch.zeros(D, device=DEV, requires_grad=True)
    scale = torch.tensor([0.0, 2.0, 2.0, 0.0, 2.0], device=DEV, requires_grad=True)
    s, h = ops.scaled_add_layer_norm(res, y, yb, scale, T, w, b, 1e-6, ytoken=tok)
    up_s = torch.randn(B, T, D, generator=g, device=DEV).bfloat16()
    up_h = torch.randn(B, T, D, generator=g, device=DEV).bfloat16()
    (s.float() * up_s.float()).sum().add((h.float() * up_h.float()).sum()).backward()
    assert scale.grad is None
    r64, y64, yb64, w64, b64 = (t.detach().double().requires_grad_(True) for t in (res, y, yb, w, b))
    c = scale.detach().double()[:, None, None]
    s64 = r64 + c * (y64 + yb64)
    mu = s64.mean(-1, keepdim=True)
    h64 = (s64 - mu) * torch.rsqrt(((s64 - mu) ** 2).mean(-1, keepdim=True) + 1e-6) * w64 + b64
    ((s64 * up_s.double()).sum() + (h64 * up_h.double()).sum()).backward()
    for name, got, want in (('res', res.grad, r64.grad), ('y', y.grad, y64.grad), ('ybias', yb.grad, yb64.grad),
                            ('weight', w.grad, w64.grad), ('bias', b.grad, b64.grad), ('token', tok.grad, y64.grad.sum((0, 1)))):
        rel = ((got.double() - want).norm() / want.norm()).item()
        print(f'[scaled_add_layer_norm] d {name}: relative L2 {rel:.2e}')
        assert rel <= 2.0 ** -7, (name, rel)
    assert bool((y.grad[0] == 0).all()) and bool((y.grad[3] == 0).all())
