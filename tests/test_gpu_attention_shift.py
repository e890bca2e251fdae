"""GPU (-m gpu): every attention kernel family on softmax rows far from zero (attention_shift_cases.py).

The rows of every case are shifted by 0, +-8, +-24, +-48, +-96 and +-120 and their keys climb or descend a staircase of 4
per 16 keys, so lse runs from below -89 to above +89 (up to +280 at 641 keys), the online-softmax rescale multiplies
accumulators that matter, the partial-record merges weigh records of very different maxima, and a padded or hidden key
that is not masked BEFORE its exp2 overflows. For every case:

  * every result is finite;
  * |got - ref| <= bound element by element for out, lse, dq, dk, dv, with the float64 reference and the derived bound of
    attention_shift_cases.py (constants from the documented arithmetic, not fitted to a run);
  * d(qkv bias): the k third is exactly 0, the v third is the column sum of dout (float32 summation: n 2^-24 sum |dout|);
  * the case ran on the intended family (fast-path queries, generic-call counter, debug hooks), as the tie tests assert.

The runners' helpers are those of test_gpu_attention_ties.py, test_gpu_narrator_ties.py and test_gpu_keymask_attention.py.
Every test prints its worst err / bound per tensor.

Measured on an MI355X, worst err / bound per family over its shapes, types, stairs and hook settings (no family is above
0.5; `-`: the entry point does not return that tensor):
  family                  out   lse    dq    dk    dv
  space_resident         0.38  0.30  0.13  0.15  0.41
  space_resident_273     0.34  0.31  0.08  0.06  0.32
  space_large_resident   0.36  0.38  0.10  0.08  0.35
  space_stream (0,1,4,5) 0.39  0.46  0.14  0.10  0.35
  space_stream_f32       0.16  0.39  0.02  0.01  0.16
  time_register (riders) 0.25  0.44  0.09  0.12  0.25
  time_mfma              0.41  0.31  0.13  0.17  0.43
  time_generic           0.25  0.23  0.08  0.15  0.44
  f32_generic            0.04  0.23  0.01  0.02  0.06
  causal                 0.41  0.38  0.17  0.17  0.44
  cls                    0.21  0.22  0.04  0.12  0.25
  rows_fwd_mfma          0.32     -     -     -     -
  rows_fwd_lds           0.23     -     -     -     -
  rows_fwd_row           0.23     -     -     -     -
  rows_bwd                  -     -  0.10  0.16  0.45
  pooler                 0.24     -  0.06  0.11  0.23
  decode                 0.25     -     -     -     -
  keymask_mfma           0.38     -  0.12  0.12  0.39
  keymask_generic        0.25     -  0.07  0.07  0.22
"""
import math

import pytest
import torch

import attention_shift_cases as SC
from test_gpu_attention_ties import _causal_lse, _generic_calls, _lib, _qkv_bias, _switch
from test_gpu_keymask_attention import _Problem as _KeymaskCall
from test_gpu_narrator_ties import (_cross_bwd, _cross_fwd, _cross_fwd_branch, _decode_steps, _dev, _guarded, _inside,
                                    _mq_bwd, _mq_fwd)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF, F32 = torch.bfloat16, torch.float32
_id = lambda v: str(v).replace(' ', '').replace('torch.', '')          # noqa: E731
stairs = pytest.mark.parametrize('stair', SC.STAIRS)
both = pytest.mark.parametrize('dt', [BF, F32], ids=['bf16', 'f32'])


def _check(tag, pairs):
    """pairs: name -> (got, reference, bound). Finite, inside the bound element by element; prints the worst ratios."""
    worst, bad = {}, []
    for name, (got, ref, bound) in pairs.items():
        got = got.detach().double().cpu().reshape(ref.shape)
        if not bool(torch.isfinite(got).all()):
            worst[name] = math.inf
            bad.append(f'{name}: {int((~torch.isfinite(got)).sum())} of {got.numel()} values are not finite')
            continue
        ratio = (got - ref).abs() / bound
        worst[name] = ratio.max().item()
        if worst[name] > 1:
            i = tuple(torch.nonzero(ratio == ratio.max())[0].tolist())
            bad.append(f'{name}: {int((ratio > 1).sum())} of {ratio.numel()} values past their bound, worst at {i}: got '
                       f'{got[i].item()!r}, want {ref[i].item()!r}, bound {bound[i].item():.3e}')
    print(f'SHIFT {tag} ' + ' '.join(f'{n}={r:.3f}' for n, r in worst.items()))
    assert not bad, f'{tag}: ' + '; '.join(bad)


def _check_bias(db, dout_rows, D):
    """dout_rows [rows, D] float64: every row that is a query. k third exactly 0, v third the column sum of dout within the
    round-off of a float32 sum of that many terms."""
    db = db.detach().double().cpu()
    assert torch.count_nonzero(db[D:2 * D]) == 0, 'd(bias) k third must be exactly 0'
    tol = dout_rows.shape[0] * 2.0 ** -24 * dout_rows.abs().sum(0) + 2.0 ** -20
    err = (db[2 * D:] - dout_rows.sum(0)).abs()
    assert bool((err <= tol).all()), f'd(bias) v third: {(err / tol).max().item():.2f} x the float32 summation bound'
    assert bool(torch.isfinite(db[:D]).all())


def _thirds(case, out, lse, dqkv):
    D = case.heads * 64
    pairs = {'out': (out,) + case.packed('out'), 'lse': (lse,) + case.packed('lse')}
    for i, n in enumerate(('dq', 'dk', 'dv')):
        pairs[n] = (dqkv[..., i * D:(i + 1) * D],) + case.packed(n)
    return pairs


# ---- divided attention -----------------------------------------------------------------------------------------------
def _run_divided(family, kind, shape, dt, stair, generic=0):
    from lavila_amd import ops
    B, F, N, H = shape
    D = 64 * H
    case = SC.make(kind, shape, dt, stair)
    _generic_calls()
    x = case.qkv.to(DEV, dt).requires_grad_(True)
    bias = _qkv_bias(D, 'trainable')
    out = ops.divided_attention(x, F, N, H, kind, bias=bias)
    out.backward(case.dout.to(DEV, dt))
    _, lse = ops.divided_attn_fwd_raw(x.detach(), F, N, H, {'space': 0, 'time': 1}[kind])
    torch.cuda.synchronize()
    calls = _generic_calls()
    assert calls == generic, f'{calls} calls on the generic kernels, {generic} expected'
    _check(f'{family} {kind}{_id(shape)} {_id(dt)} stair={stair:+.0f}', _thirds(case, out, lse, x.grad))
    _check_bias(bias.grad, case.dout.reshape(-1, D), D)


def _fast(kind, dt, shape):
    B, F, N, H = shape
    fp = _lib().lvl_attention_fast_path if dt == BF else _lib().lvl_attention_fast_path_f32
    return fp({'space': 0, 'time': 1}[kind], F, N, H)


@stairs
@both
@pytest.mark.parametrize('shape', SC.SPACE_RESIDENT, ids=_id)
def test_space_resident_shifted(shape, dt, stair):
    assert _fast('space', dt, shape) == 1
    _run_divided('space_resident', 'space', shape, dt, stair)


@stairs
@pytest.mark.parametrize('shape', SC.SPACE_RESIDENT_273, ids=_id)
def test_space_resident_forward_273_to_288_keys_shifted(shape, stair):
    _run_divided('space_resident_273', 'space', shape, BF, stair)


@stairs
@pytest.mark.parametrize('shape', SC.SPACE_LARGE_RESIDENT, ids=_id)
def test_space_large_group_resident_shifted(shape, stair):
    B, F, N, H = shape
    with _switch('lvl_debug_space_stream', -1, 0):
        assert _lib().lvl_attention_fast_path(0, F, N, H) == 1
        _run_divided('space_large_resident', 'space', shape, BF, stair)


@stairs
@pytest.mark.parametrize('shape', SC.SPACE_STREAM, ids=_id)
def test_space_streaming_shifted(shape, stair):
    _run_divided('space_stream', 'space', shape, BF, stair)


@stairs
@pytest.mark.parametrize('variant', [1, 4, 5])
def test_space_streaming_variants_shifted(variant, stair):
    """Variant 0 is the default dispatch of test_space_streaming_shifted."""
    with _switch('lvl_debug_stream_variant', variant, 0):
        _run_divided(f'space_stream_v{variant}', 'space', SC.SPACE_STREAM_VARIANTS, BF, stair)


@stairs
@pytest.mark.parametrize('shape', SC.SPACE_STREAM_F32, ids=_id)
def test_space_streaming_f32_shifted(shape, stair):
    _run_divided('space_stream_f32', 'space', shape, F32, stair)


@stairs
@both
@pytest.mark.parametrize('shape', SC.TIME_REGISTER, ids=_id)
def test_time_register_shifted(shape, dt, stair):
    assert _fast('time', dt, shape) == 1
    _run_divided('time_register', 'time', shape, dt, stair)


@stairs
@both
@pytest.mark.parametrize('rider', [0, 1, 2])
def test_time_register_riders_shifted(rider, dt, stair):
    assert _fast('time', dt, SC.TIME_RIDERS) == 1
    with _switch('lvl_debug_time_bwd_rider', rider, -1):
        _run_divided(f'time_register_rider{rider}', 'time', SC.TIME_RIDERS, dt, stair)


@stairs
@pytest.mark.parametrize('shape', SC.TIME_MFMA, ids=_id)
def test_time_mfma_shifted(shape, stair):
    assert _fast('time', BF, shape) == 1
    _run_divided('time_mfma', 'time', shape, BF, stair)


@stairs
@pytest.mark.parametrize('shape', SC.TIME_GENERIC, ids=_id)
def test_time_generic_shifted(shape, stair):
    assert _fast('time', BF, shape) == 0
    _run_divided('time_generic', 'time', shape, BF, stair, generic=3)


@stairs
@pytest.mark.parametrize('kind,shape', SC.F32_GENERIC, ids=_id)
def test_f32_generic_shifted(kind, shape, stair):
    with _switch('lvl_debug_f32_generic', 1, 0):
        assert _fast(kind, F32, shape) == 0
        _run_divided('f32_generic', kind, shape, F32, stair, generic=3)


# ---- causal text and cls-only ----------------------------------------------------------------------------------------
@stairs
@both
@pytest.mark.parametrize('shape', SC.CAUSAL, ids=_id)
def test_causal_shifted(shape, dt, stair):
    from lavila_amd import ops
    B, L, H = shape
    D = 64 * H
    case = SC.make('causal', shape, dt, stair)
    x = case.qkv.to(DEV, dt).requires_grad_(True)
    bias = _qkv_bias(D, 'trainable')
    _generic_calls()
    out = ops.causal_attention(x, H, bias=bias)
    torch.cuda.synchronize()
    assert _generic_calls() == 0, 'causal forward left the MFMA kernel'
    out.backward(case.dout.to(DEV, dt))
    lse = _causal_lse(x.detach(), B, L, H)
    torch.cuda.synchronize()
    assert _generic_calls() == int(L > 256), 'causal backward: generic kernel above 256 tokens only'
    _check(f'causal causal{_id(shape)} {_id(dt)} stair={stair:+.0f}', _thirds(case, out, lse, x.grad))
    _check_bias(bias.grad, case.dout.reshape(-1, D), D)


@stairs
@both
@pytest.mark.parametrize('shape', SC.CLS, ids=_id)
def test_cls_only_shifted(shape, dt, stair):
    from lavila_amd import _cabi as C
    from lavila_amd import ops
    B, T, H = shape
    D = 64 * H
    case = SC.make('cls', shape, dt, stair)
    q = case.qkv[:, 0, :D].to(DEV, dt).contiguous().requires_grad_(True)
    kv = case.qkv[:, :, D:].to(DEV, dt).contiguous().requires_grad_(True)
    bias = _qkv_bias(D, 'trainable')
    out = ops.cls_attention(q, kv, H, bias=bias)
    out.backward(case.dout[:, 0].to(DEV, dt))
    o2 = torch.empty(B, D, dtype=dt, device=DEV)
    lse = torch.empty(B, H, dtype=torch.float32, device=DEV)
    C.check(C.lib().lvl_cls_attn_fwd(C.ptr(q.detach()), C.ptr(kv.detach()), C.ptr(o2), C.ptr(lse), B, T, H,
                                     C.dtype_code(kv), C.stream_ptr()), 'lvl_cls_attn_fwd')
    torch.cuda.synchronize()
    first = lambda n: tuple(x[:, 0] for x in case.packed(n))              # noqa: E731
    lse_ref, lse_bound = case.packed('lse')
    _check(f'cls cls{_id(shape)} {_id(dt)} stair={stair:+.0f}',
           {'out': (out,) + first('out'), 'lse': (lse, lse_ref[:, :, 0], lse_bound[:, :, 0]),
            'dq': (q.grad,) + first('dq'), 'dk': (kv.grad[..., :D],) + case.packed('dk'),
            'dv': (kv.grad[..., D:],) + case.packed('dv')})
    _check_bias(bias.grad, case.dout[:, 0], D)


# ---- the narrator's kernels: rows attention, pooler, decode ------------------------------------------------------------
CROSS_FWD = ([(BF, s, b) for s, b in zip(SC.CROSS_FWD_BF16, ['mfma'] * 3 + ['lds'] + ['row'] * 2)] +
             [(F32, s, b) for s, b in zip(SC.CROSS_FWD_F32, ['lds', 'row'])])


@stairs
@pytest.mark.parametrize('dt,shape,branch', CROSS_FWD, ids=_id)
def test_cross_attn_rows_fwd_shifted(dt, shape, branch, stair):
    contexts, qrep, H, Tk = shape
    assert _cross_fwd_branch(dt, qrep, Tk) == branch
    D, rows = 64 * H, contexts * qrep
    q, kv, _, res = SC.make('cross', shape, dt, stair).as_cross()
    out = _guarded((rows, D), dt)
    _cross_fwd(_dev(q, dt), _dev(kv, dt), out, rows, qrep, Tk, H)
    torch.cuda.synchronize()
    _check(f'rows_fwd_{branch} cross{_id(shape)} {_id(dt)} stair={stair:+.0f}',
           {'out': (_inside('out', out, (rows, D)),) + res['out']})


@stairs
@pytest.mark.parametrize('shape', SC.CROSS_BWD, ids=_id)
def test_cross_attn_rows_bwd_shifted(shape, stair):
    contexts, qrep, H, Tk = shape
    assert Tk <= 256 and qrep >= 2
    D, rows = 64 * H, contexts * qrep
    q, kv, dout, res = SC.make('cross', shape, BF, stair).as_cross()
    dq, dkv = _guarded((rows, D), BF), _guarded((contexts, Tk, 2 * D), BF)
    _cross_bwd(_dev(q, BF), _dev(kv, BF), _dev(dout, BF), dq, dkv, rows, qrep, Tk, H)
    torch.cuda.synchronize()
    dkv = _inside('dkv', dkv, (contexts, Tk, 2 * D))
    _check(f'rows_bwd cross{_id(shape)} bfloat16 stair={stair:+.0f}',
           {'dq': (_inside('dq', dq, (rows, D)),) + res['dq'], 'dk': (dkv[..., :D],) + res['dk'],
            'dv': (dkv[..., D:],) + res['dv']})


@stairs
@pytest.mark.parametrize('shared', [False, True])
@both
@pytest.mark.parametrize('shape', SC.MQ, ids=_id)
def test_mq_cross_attn_shifted(shape, dt, shared, stair):
    B, NQ, H, Tk = shape
    D = 64 * H
    q, kv, dout, res = SC.make('mq', shape + (shared,), dt, stair).as_mq()
    qd, kvd, dod = _dev(q, dt), _dev(kv, dt), _dev(dout, dt)
    out = _guarded((B, NQ, D), dt)
    _mq_fwd(qd, kvd, out, B, NQ, H, Tk, shared)
    dq, dkv = _guarded(tuple(q.shape), dt), _guarded((B, Tk, 128), dt)
    _mq_bwd(qd, kvd, dod, dq, dkv, B, NQ, H, Tk, shared)
    torch.cuda.synchronize()
    dkv = _inside('dkv', dkv, (B, Tk, 128))
    _check(f'pooler mq{_id(shape)}{"shared" if shared else ""} {_id(dt)} stair={stair:+.0f}',
           {'out': (_inside('out', out, (B, NQ, D)),) + res['out'], 'dq': (_inside('dq', dq, tuple(q.shape)),) + res['dq'],
            'dk': (dkv[..., :64],) + res['dk'], 'dv': (dkv[..., 64:],) + res['dv']})


@stairs
@both
@pytest.mark.parametrize('shape', SC.DECODE, ids=_id)
def test_decode_self_attn_shifted(shape, dt, stair):
    """Step t equals row t of the causal case; the cache ends as the k | v thirds, rows past the last step untouched."""
    B, L, H, cap = shape
    D = 64 * H
    case = SC.make('causal', (B, L, H), dt, stair)
    out, cache = _decode_steps(case.qkv, cap, H, dt)
    _check(f'decode decode{_id(shape)} {_id(dt)} stair={stair:+.0f}', {'out': (out,) + case.packed('out')})
    assert torch.equal(cache[:, :L].double().cpu(), case.qkv[..., D:]), 'the cache is not the k | v rows of the steps'
    assert torch.isnan(cache[:, L:].float()).all(), 'a cache row past the last step was written'


# ---- key-masked attention --------------------------------------------------------------------------------------------
def _keymask_branch(dt, Tk):
    """The dispatch of lvl_keymask_attn_fwd / _bwd (keymask_attn.hip), restated."""
    return 'mfma' if dt == BF and Tk <= 256 else 'generic'


KEYMASK = [(dt, s, b) for (dt, s), b in zip(SC.KEYMASK, ['mfma', 'mfma', 'generic', 'generic'])]


@stairs
@pytest.mark.parametrize('which', SC.MASKS)
@pytest.mark.parametrize('dt,shape,branch', KEYMASK, ids=_id)
def test_keymask_attention_shifted(dt, shape, branch, which, stair):
    """A ragged prefix; one context without a visible key (uniform, dq = dk = 0 there); hidden keys that hold the largest
    scores of their context: the reference is computed without them and their dk / dv rows are exact zeros."""
    contexts, Tk, H = shape
    assert _keymask_branch(dt, Tk) == branch
    D = 64 * H
    case = SC.make('keymask', shape + (which,), dt, stair)
    call = _KeymaskCall(contexts, Tk, Tk, H, dt, 'separate', seed=0)
    for t, x in ((call.q, case.pack(case.q)), (call.k, case.pack(case.k)), (call.v, case.pack(case.v)),
                 (call.do, case.dout)):
        t.copy_(x.reshape(t.shape).to(DEV, dt))
    got = call.run(case.vis.to(torch.uint8))
    _check(f'keymask_{branch}_{which} keymask{_id(shape)} {_id(dt)} stair={stair:+.0f}',
           {n: (g,) + case.packed(n) for n, g in zip(SC.NAMES, got)})
    hidden = ~case.vis & case.vis.any(-1, keepdim=True)               # a context without a visible key is uniform: dv != 0
    assert not got[2][hidden].any() and not got[3][hidden].any(), 'dk / dv rows of hidden keys must be exact zeros'
    if which == SC.EMPTY:
        assert not got[1][1].any() and not got[2][1].any(), 'no gradient reaches the scores of a uniform row'
