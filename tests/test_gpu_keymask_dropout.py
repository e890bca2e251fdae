"""GPU: the raw entry points of the text tower's dropout -- lvl_keymask_attn_drop_fwd / _bwd (both kernel families) and
lvl_dropout_add_layernorm_fwd / _bwd -- against float64 autograd under the restated mask
(tests/distilbert_dropout_reference.py) and in exact checks: p = 0 is today's call bit for bit, the keep bits read back out
of the forward equal the numpy restatement for every (b, h, i, j), one visible key, the row-0 form, hidden keys, the
bits of the decoder's gated pair, the error codes.

Every output buffer and the workspace are NaN-poisoned before each call; every call runs twice and must give equal bits."""
import ctypes

import numpy as np
import pytest
import torch

import distilbert_dropout_reference as DD
import dropout_reference as DR
from test_gpu_keymask_attention import BF, DEV, NAN, _check, _mask, _off, _Problem, _rand

pytestmark = pytest.mark.gpu
SEED = 0x5EEDC0DE0B5E55ED
BOUND = 2.0 ** -7


def _C():
    from lavila_amd import _cabi as C
    return C


def _ratio(got, want):
    """tests/test_gpu_narrator_train.py::_ratio: max|got - want| / max|want|."""
    return ((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()


def _run_drop(pb, mask, p, site=3, idx_qrep=None, seed=SEED, backward=True):
    """_Problem.run through lvl_keymask_attn_drop_fwd / _bwd, twice into NaN-prefilled buffers: (out, dq, dk, dv)."""
    C = _C()
    contexts, qrep, Tk, H = pb.dims
    D, dt = pb.D, pb.dt
    qs, kvs, kvc = pb.strides
    iq = qrep if idx_qrep is None else idx_qrep
    qp, kp, vp = (ctypes.c_void_p(x) if isinstance(x, int) else x for x in pb.pointers())
    m = None if mask is None else mask.to(DEV).contiguous()
    code = C.LVL_BF16 if dt == BF else C.LVL_F32
    n_ws = C.lib().lvl_workspace_floats(b'keymask_attn_bwd', contexts * qrep * H, Tk)
    runs = []
    for _ in range(2):
        out = torch.full((contexts * qrep, D), NAN, dtype=dt, device=DEV)
        C.check(C.lib().lvl_keymask_attn_drop_fwd(qp, kp, vp, C.ptr(m), C.ptr(out), contexts, qrep, Tk, H, qs, kvs, kvc, Tk, iq,
                                                  seed, site, p, code, C.stream_ptr()), 'lvl_keymask_attn_drop_fwd')
        if not backward:
            runs.append((out.cpu().reshape(contexts, qrep, D),))
            continue
        if pb.layout == 'packed':
            dqkv = torch.full((contexts * Tk, 3 * D), NAN, dtype=dt, device=DEV)
            dqp, dkp, dvp = C.ptr(dqkv), _off(dqkv, D), _off(dqkv, 2 * D)
        else:
            dq = torch.full((contexts, Tk, D) if pb.layout == 'row0' else (contexts * qrep, D), NAN, dtype=dt, device=DEV)
            dk = torch.full((contexts, Tk, D), NAN, dtype=dt, device=DEV)
            dv = torch.full((contexts, Tk, D), NAN, dtype=dt, device=DEV)
            dqp, dkp, dvp = C.ptr(dq), C.ptr(dk), C.ptr(dv)
        ws = torch.full((n_ws + 64,), NAN, device=DEV)
        C.check(C.lib().lvl_keymask_attn_drop_bwd(qp, kp, vp, C.ptr(m), C.ptr(pb.do), dqp, dkp, dvp, C.ptr(ws), contexts, qrep,
                                                  Tk, H, qs, kvs, kvc, Tk, iq, seed, site, p, code, C.stream_ptr()),
                'lvl_keymask_attn_drop_bwd')
        torch.cuda.synchronize()
        assert torch.isnan(ws[n_ws:]).all(), 'the backward wrote behind its declared workspace'
        if pb.layout == 'packed':
            x = dqkv.cpu().reshape(contexts, Tk, 3 * D)
            got = (x[..., :D], x[..., D:2 * D], x[..., 2 * D:])
        elif pb.layout == 'row0':
            assert torch.isnan(dq[:, 1:]).all(), 'rows of dq that the call does not address were written'
            got = (dq[:, :1].cpu(), dk.cpu(), dv.cpu())
        else:
            got = (dq.cpu().reshape(contexts, qrep, D), dk.cpu(), dv.cpu())
        runs.append((out.cpu().reshape(contexts, qrep, D),) + tuple(t.contiguous() for t in got))
    for a, b in zip(*runs):
        assert not torch.isnan(a).any(), 'an addressed element was not written'
        assert torch.equal(a, b), 'two runs differ'
    return runs[0]


def _reference_drop(pb, mask, p, site=3, idx_qrep=None, seed=SEED):
    contexts, qrep, Tk, H = pb.dims
    keep = DD.attn_keep(seed, site, contexts, H, qrep, Tk, p, idx_qrep)
    q, k, v = (t.clone().requires_grad_(True) for t in (pb.q64, pb.k64, pb.v64))
    out = DD.keymask_attention_drop(q, k, v, mask, H, keep, float(DR.scale(p)))
    out.backward(pb.do64)
    return out.detach(), q.grad, k.grad, v.grad


def _masks(contexts, Tk, g):
    """prefix, holes, NULL, and a prefix mask with one context that has no visible key"""
    empty = _mask(contexts, Tk, 'prefix', g)
    empty[min(1, contexts - 1)] = 0
    return {'prefix': _mask(contexts, Tk, 'prefix', g), 'holes': _mask(contexts, Tk, 'holes', g), 'null': None, 'empty': empty}


MFMA_SHAPES = [(2, 1, 2, 24, 5), (3, 21, 2, 21, None), (2, 17, 1, 1, None), (2, 37, 3, 200, None), (2, 12, 12, 256, None)]


@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('contexts,qrep,H,Tk,idx_qrep', MFMA_SHAPES)
def test_mfma_kernels_against_float64(contexts, qrep, H, Tk, idx_qrep, p):
    """bf16, Tk <= 256: the <DROP, KEYMASK> MFMA instantiations at the 2^-7 bar of tests/test_gpu_decoder_dropout.py. The
    undropped kernels' ratios on the same inputs are printed beside them."""
    pb = _Problem(contexts, qrep, Tk, H, BF, 'separate', seed=2000 + 7 * Tk + H)
    for kind, mask in _masks(contexts, Tk, pb.g).items():
        got, want = _run_drop(pb, mask, p, idx_qrep=idx_qrep), _reference_drop(pb, mask, p, idx_qrep=idx_qrep)
        r = [_ratio(a, b) for a, b in zip(got, want)]
        r0 = [_ratio(a, b) for a, b in zip(pb.run(mask), pb.reference(mask))]
        print(f'[keymask_drop mfma {contexts, qrep, H, Tk} {kind} p={p}] worst ratios out/dq/dk/dv '
              + ' '.join(f'{x:.2e}' for x in r) + ' | undropped ' + ' '.join(f'{x:.2e}' for x in r0) + f' (bound {BOUND:.2e})')
        assert max(r) <= BOUND, (kind, r, r0)
        if mask is not None:
            hidden = (mask == 0) & (mask.sum(1, keepdim=True) > 0)
            assert not got[2][hidden].any() and not got[3][hidden].any(), 'dk / dv rows of hidden keys must be exact zeros'


GENERIC_SHAPES = [(torch.float32, 2, 1, 2, 1), (torch.float32, 2, 63, 2, 63), (torch.float32, 2, 64, 1, 64),
                  (torch.float32, 3, 65, 2, 65), (torch.float32, 2, 130, 2, 130), (torch.float32, 2, 5, 2, 130),
                  (BF, 1, 257, 1, 257), (BF, 2, 300, 2, 300), (BF, 2, 70, 1, 300)]


@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('dt,contexts,qrep,H,Tk', GENERIC_SHAPES, ids=lambda x: str(x).replace('torch.', ''))
def test_generic_kernels_against_float64(dt, contexts, qrep, H, Tk, p):
    """float32, and bf16 beyond 256 keys: the shape-generic kernels at the bars tests/test_gpu_keymask_attention.py sets for
    them (F32_TOL with its out / gradient multipliers; 2^-7 for bf16)."""
    layout = 'packed' if qrep == Tk else 'separate'
    pb = _Problem(contexts, qrep, Tk, H, dt, layout, seed=3000 + 7 * Tk + H)
    idx_qrep = None if qrep == Tk else qrep + 4
    for kind, mask in _masks(contexts, Tk, pb.g).items():
        got, want = _run_drop(pb, mask, p, idx_qrep=idx_qrep), _reference_drop(pb, mask, p, idx_qrep=idx_qrep)
        r = [_ratio(a, b) for a, b in zip(got, want)]
        r0 = [_ratio(a, b) for a, b in zip(pb.run(mask), pb.reference(mask))]
        print(f'[keymask_drop generic {dt} {contexts, qrep, H, Tk} {kind} p={p}] worst ratios out/dq/dk/dv '
              + ' '.join(f'{x:.2e}' for x in r) + ' | undropped ' + ' '.join(f'{x:.2e}' for x in r0))
        _check(got, want, dt, f'drop {contexts, qrep, H, Tk} {kind} p={p}')
        if mask is not None:
            hidden = (mask == 0) & (mask.sum(1, keepdim=True) > 0)
            assert not got[2][hidden].any() and not got[3][hidden].any(), 'dk / dv rows of hidden keys must be exact zeros'


@pytest.mark.parametrize('layout', ['packed', 'separate'])
@pytest.mark.parametrize('dt,contexts,Tk,H', [(BF, 2, 77, 2), (BF, 1, 256, 1), (BF, 1, 300, 1), (torch.float32, 2, 70, 2)],
                         ids=lambda x: str(x).replace('torch.', ''))
def test_p0_is_todays_call_bit_for_bit(dt, contexts, Tk, H, layout):
    pb = _Problem(contexts, Tk, Tk, H, dt, layout, seed=41 + Tk)
    for mask in (_mask(contexts, Tk, 'holes', pb.g), None):
        for a, b in zip(_run_drop(pb, mask, 0.0), pb.run(mask)):
            assert torch.equal(a, b)


@pytest.mark.parametrize('dt,Tk', [(BF, 256), (BF, 300), (torch.float32, 130)], ids=['mfma256', 'generic300', 'f32_130'])
def test_keep_bits_read_back_equal_the_restatement(dt, Tk):
    """q = 0, p = 0.5, a window of exactly 32 visible keys with v_j = one_hot(j - window start): every visible key has
    P = 2^-5, so out[i, c] is exactly 2^-4 where key start + c is kept and 0 where it is dropped. The window slides over all
    keys; the recovered bits must equal the numpy restatement for every (b, h, i, j). Queries are a subset (idx_qrep)."""
    C = _C()
    contexts, qrep, H, idx_qrep, site, p = 2, 19, 2, 23, 5, 0.5
    D = H * 64
    q = torch.zeros(contexts * qrep, D, dtype=dt, device=DEV)
    k = torch.zeros(contexts, Tk, D, dtype=dt, device=DEV)
    code = C.LVL_BF16 if dt == BF else C.LVL_F32
    got = torch.zeros(contexts, H, qrep, Tk, dtype=torch.bool)
    seen = torch.zeros(Tk, dtype=torch.bool)
    starts = sorted(set(list(range(0, Tk - 31, 32)) + [Tk - 32]))
    for start in starts:
        mask = torch.zeros(contexts, Tk, dtype=torch.uint8)
        mask[:, start:start + 32] = 1
        v = torch.zeros(contexts, Tk, H, 64)
        v[:, torch.arange(start, start + 32), :, torch.arange(32)] = 1.0
        v = v.reshape(contexts, Tk, D).to(dt).to(DEV)
        m = mask.to(DEV)
        outs = []
        for _ in range(2):
            out = torch.full((contexts * qrep, D), NAN, dtype=dt, device=DEV)
            C.check(C.lib().lvl_keymask_attn_drop_fwd(C.ptr(q), C.ptr(k), C.ptr(v), C.ptr(m), C.ptr(out), contexts, qrep, Tk, H,
                                                      D, D, Tk * D, Tk, idx_qrep, SEED, site, p, code, C.stream_ptr()), 'fwd')
            outs.append(out.float().cpu())
        assert torch.equal(outs[0], outs[1])
        o = outs[0].reshape(contexts, qrep, H, 64).permute(0, 2, 1, 3)               # [b, h, i, c]
        assert ((o == 0.0625) | (o == 0)).all(), f'window {start}: out must be exactly 2^-4 or 0'
        assert not o[..., 32:].any()
        got[..., start:start + 32] = o[..., :32] != 0
        seen[start:start + 32] = True
    assert seen.all()
    want = torch.from_numpy(DD.attn_keep(SEED, site, contexts, H, qrep, Tk, p, idx_qrep))
    assert torch.equal(got, want)
    assert 0.4 < want.float().mean() < 0.6


@pytest.mark.parametrize('dt,Tk', [(BF, 24), (BF, 300), (torch.float32, 70)], ids=['mfma', 'generic_bf16', 'f32'])
def test_one_visible_key(dt, Tk):
    """One visible key per context, p = 0.5, one query per context: P = 1, so out is exactly 2 v or 0, dq = dk = 0 and dv of
    the visible key is exactly 2 dout or 0."""
    contexts, H, p, idx_qrep = 4, 3, 0.5, 4
    pb = _Problem(contexts, 1, Tk, H, dt, 'separate', seed=17 + Tk, scale=1.0)
    mask = torch.zeros(contexts, Tk, dtype=torch.uint8)
    pos = [0, Tk - 1, Tk // 2, 1 % Tk]
    for b in range(contexts):
        mask[b, pos[b]] = 1
    out, dq, dk, dv = _run_drop(pb, mask, p, idx_qrep=idx_qrep)
    keep = torch.from_numpy(DD.attn_keep(SEED, 3, contexts, H, 1, Tk, p, idx_qrep))      # [b, h, 1, Tk]
    assert not dq.any() and not dk.any()
    kept = 0
    for b in range(contexts):
        for h in range(H):
            kb = bool(keep[b, h, 0, pos[b]])
            kept += kb
            sl = slice(h * 64, (h + 1) * 64)
            v_row, do_row = pb.v.cpu()[b, pos[b], sl].float(), pb.do.cpu()[b, sl].float()
            assert torch.equal(out[b, 0, sl].float(), 2 * v_row if kb else torch.zeros(64)), (b, h)
            assert torch.equal(dv[b, pos[b], sl].float(), 2 * do_row if kb else torch.zeros(64)), (b, h)
    assert 0 < kept < contexts * H
    assert not dv[mask == 0].any()


@pytest.mark.parametrize('kind', ['prefix', 'holes', None])
@pytest.mark.parametrize('dt', [BF, torch.float32], ids=['bf16', 'f32'])
def test_row0_form_is_row_0_of_the_full_call(dt, kind):
    """qrep = 1, q_stride = L D, idx_qrep = L (the last layer under CLIP_HF), compared as
    tests/test_gpu_keymask_attention.py::test_keymask_attention_row0_form compares: against float64 under the mask elements
    of row 0 of the full call. The forward of the full call on the same tensors gives the same row 0."""
    C = _C()
    contexts, Tk, H, p = 3, 77, 4, 0.1
    pb = _Problem(contexts, 1, Tk, H, dt, 'row0', seed=77)
    mask = None if kind is None else _mask(contexts, Tk, kind, pb.g)
    got = _run_drop(pb, mask, p, idx_qrep=Tk)
    _check(got, _reference_drop(pb, mask, p, idx_qrep=Tk), dt, f'row0 drop {kind}')
    D = pb.D
    full = torch.full((contexts * Tk, D), NAN, dtype=dt, device=DEV)
    m = None if mask is None else mask.to(DEV)
    C.check(C.lib().lvl_keymask_attn_drop_fwd(C.ptr(pb.qfull), C.ptr(pb.k), C.ptr(pb.v), C.ptr(m), C.ptr(full), contexts, Tk, Tk,
                                              H, D, D, Tk * D, Tk, Tk, SEED, 3, p, C.LVL_BF16 if dt == BF else C.LVL_F32,
                                              C.stream_ptr()), 'fwd')
    row0 = full.cpu().reshape(contexts, Tk, D)[:, :1]
    if dt == torch.float32:                       # one wave per row, the same arithmetic: equal bits
        assert torch.equal(row0, got[0])
    else:
        assert (row0.double() - got[0].double()).abs().max() <= BOUND * got[0].double().abs().max()


@pytest.mark.parametrize('dt,Tk', [(torch.float32, 37), (torch.float32, 130), (BF, 300)], ids=['f32_37', 'f32_130', 'bf16_300'])
def test_generic_kernels_never_read_hidden_rows(dt, Tk):
    """NaN-poisoned k / v rows at hidden keys: every result is NaN-free and equals the run with those rows as they were, bit
    for bit; dk / dv rows of hidden keys are exact zeros under dropout."""
    contexts, H, p = 2, 2, 0.5
    results = []
    for poison in (False, True):
        pb = _Problem(contexts, Tk, Tk, H, dt, 'separate', seed=31 + Tk)
        mask = _mask(contexts, Tk, 'holes', pb.g)
        if poison:
            hidden = (mask == 0).to(DEV)[..., None]
            for t in (pb.k, pb.v):
                t.copy_(torch.where(hidden, torch.full_like(t, NAN), t))
        results.append(_run_drop(pb, mask, p))
    for name, a, b in zip(('out', 'dq', 'dk', 'dv'), *results):
        assert torch.equal(a, b), f'{name} depends on the rows of hidden keys'
    assert not results[1][2][mask == 0].any() and not results[1][3][mask == 0].any()
    assert results[1][3][mask != 0].any()


# ----------------------------------------------------------------------------------------------------------------------
# lvl_dropout_add_layernorm_fwd / _bwd
# ----------------------------------------------------------------------------------------------------------------------
def _ln_inputs(rows, D, dt, seed):
    g = torch.Generator().manual_seed(seed)
    res, y, dh = (_rand((rows, D), g, dt)[0] for _ in range(3))
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(D, generator=g)).to(DEV)
    return res, y, dh, gamma, beta


def _ln_drop(res, y, dh, gamma, beta, stride, p, site=4, entry='own'):
    """(s, h, mean, rstd, ds, dy, dgamma, dbeta) of the new pair ('own') or of the decoder's gated pair with gate NULL."""
    C = _C()
    L = C.lib()
    rows, D = res.shape
    code, eps = C.dtype_code(res), 1e-12
    runs = []
    for _ in range(2):
        s, h, ds, dy = (torch.full_like(res, NAN) for _ in range(4))
        mean, rstd = (torch.full((rows,), NAN, device=DEV) for _ in range(2))
        dg, db = (torch.full((D,), NAN, device=DEV) for _ in range(2))
        ws = C.workspace('gated_add_layernorm_bwd', rows, D, DEV)
        if entry == 'own':
            C.check(L.lvl_dropout_add_layernorm_fwd(C.ptr(res), C.ptr(y), C.ptr(gamma), C.ptr(beta), eps, C.ptr(s), C.ptr(h),
                                                    C.ptr(mean), C.ptr(rstd), rows, D, stride, SEED, site, p, code,
                                                    C.stream_ptr()), 'lvl_dropout_add_layernorm_fwd')
            C.check(L.lvl_dropout_add_layernorm_bwd(C.ptr(dh), C.ptr(s), C.ptr(gamma), C.ptr(mean), C.ptr(rstd), None, C.ptr(ds),
                                                    C.ptr(dy), C.ptr(dg), C.ptr(db), C.ptr(ws), rows, D, stride, SEED, site, p,
                                                    code, C.stream_ptr()), 'lvl_dropout_add_layernorm_bwd')
        else:
            assert stride == D
            C.check(L.lvl_gated_add_layernorm_train_drop(C.ptr(res), C.ptr(y), None, C.ptr(gamma), C.ptr(beta), eps, C.ptr(s),
                                                         C.ptr(h), C.ptr(mean), C.ptr(rstd), rows, D, SEED, site, p, code,
                                                         C.stream_ptr()), 'lvl_gated_add_layernorm_train_drop')
            C.check(L.lvl_gated_add_layernorm_bwd_drop(C.ptr(dh), C.ptr(s), None, None, C.ptr(gamma), C.ptr(mean), C.ptr(rstd),
                                                       None, C.ptr(ds), C.ptr(dy), C.ptr(dg), C.ptr(db), None, C.ptr(ws), rows, D,
                                                       SEED, site, p, code, C.stream_ptr()), 'lvl_gated_add_layernorm_bwd_drop')
        torch.cuda.synchronize()
        runs.append(tuple(t.cpu() for t in (s, h, mean, rstd, ds, dy, dg, db)))
    for a, b in zip(*runs):
        assert torch.equal(a, b) and not torch.isnan(a).any()
    return runs[0]


@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('dt', [BF, torch.float32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('rows,D', [(1, 256), (3, 768), (65, 256)])
def test_dropout_add_layernorm_is_the_gated_pair_without_a_gate(rows, D, dt, p):
    """row_index_stride = D: the bits of lvl_gated_add_layernorm_train_drop / _bwd_drop with gate NULL; the kept sum shows
    the restated mask (a dropped element leaves the residual as it is) and dy = (keep ? scale : 0) ds."""
    args = _ln_inputs(rows, D, dt, 50 + rows)
    own, gated = _ln_drop(*args, D, p), _ln_drop(*args, D, p, entry='gated')
    for name, a, b in zip(('s', 'h', 'mean', 'rstd', 'ds', 'dy', 'dgamma', 'dbeta'), own, gated):
        assert torch.equal(a, b), name
    keep = torch.from_numpy(DD.row_keep(SEED, 4, rows, D, p))
    res, y = args[0].cpu(), args[1].cpu()
    s, ds, dy = own[0], own[4], own[5]
    assert torch.equal(s[~keep], res[~keep]) and not dy[~keep].any()
    scale = float(DR.scale(p))
    want_s = (res.double() + scale * y.double())[keep]
    assert (s.double()[keep] - want_s).abs().max() <= 2.0 ** (-8 if dt == BF else -22) * want_s.abs().max()
    want_dy = (scale * ds.double())[keep]
    assert (dy.double()[keep] - want_dy).abs().max() <= 2.0 ** (-8 if dt == BF else -22) * want_dy.abs().max().clamp_min(1e-30)


@pytest.mark.parametrize('dt', [BF, torch.float32], ids=['bf16', 'f32'])
def test_dropout_add_layernorm_row0_stride(dt):
    """B rows with row_index_stride = L D: the bits of rows b L of the call on all B L rows (per-row results: s, h, mean,
    rstd, ds, dy; dgamma / dbeta are sums over the rows of a call)."""
    B, L, D, p = 5, 7, 256, 0.5
    res, y, dh, gamma, beta = _ln_inputs(B * L, D, dt, 9)
    full = _ln_drop(res, y, dh, gamma, beta, D, p)
    sub = _ln_drop(res[::L].contiguous(), y[::L].contiguous(), dh[::L].contiguous(), gamma, beta, L * D, p)
    for name, a, b in list(zip(('s', 'h', 'mean', 'rstd', 'ds', 'dy'), full, sub)):
        assert torch.equal(a[::L], b), name
    wrong = _ln_drop(res[::L].contiguous(), y[::L].contiguous(), dh[::L].contiguous(), gamma, beta, D, p)
    assert not torch.equal(wrong[0][1:], sub[0][1:])


@pytest.mark.parametrize('dt', [BF, torch.float32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('rows,D', [(3, 768), (65, 256)])
def test_dropout_add_layernorm_p0_is_the_undropped_train_pair(rows, D, dt):
    C = _C()
    L = C.lib()
    res, y, dh, gamma, beta = _ln_inputs(rows, D, dt, 70 + rows)
    own = _ln_drop(res, y, dh, gamma, beta, D, 0.0)
    s, h, ds = (torch.full_like(res, NAN) for _ in range(3))
    mean, rstd = (torch.full((rows,), NAN, device=DEV) for _ in range(2))
    dg, db = (torch.full((D,), NAN, device=DEV) for _ in range(2))
    ws = C.workspace('gated_add_layernorm_bwd', rows, D, DEV)
    code = C.dtype_code(res)
    C.check(L.lvl_gated_add_layernorm_train(C.ptr(res), C.ptr(y), None, C.ptr(gamma), C.ptr(beta), 1e-12, C.ptr(s), C.ptr(h),
                                            C.ptr(mean), C.ptr(rstd), rows, D, code, C.stream_ptr()), 'train')
    C.check(L.lvl_gated_add_layernorm_bwd(C.ptr(dh), C.ptr(s), None, None, C.ptr(gamma), C.ptr(mean), C.ptr(rstd), None, C.ptr(ds),
                                          None, C.ptr(dg), C.ptr(db), None, C.ptr(ws), rows, D, code, C.stream_ptr()), 'bwd')
    torch.cuda.synchronize()
    for name, a, b in zip(('s', 'h', 'mean', 'rstd', 'ds', 'dy', 'dgamma', 'dbeta'), own, (s, h, mean, rstd, ds, ds, dg, db)):
        assert torch.equal(a, b.cpu()), name


@pytest.mark.parametrize('p', [None, 0.5], ids=['plain', 'p0.5'])
@pytest.mark.parametrize('form', ['full', 'row0'])
@pytest.mark.parametrize('dt', [BF, torch.float32], ids=['bf16', 'f32'])
def test_keymask_function_makes_the_raw_calls(dt, form, p):
    """ops._KeymaskAttnFn, forward and backward, gives the bits of lvl_keymask_attn_fwd / _bwd without `drop` and of
    lvl_keymask_attn_drop_fwd / _bwd with it, on the same operands: the full form and the row-0 form (Lq = 1, idx_qrep = L),
    the last two keys of sample 1 hidden."""
    from lavila_amd import ops
    C = _C()
    L = C.lib()
    B, Lk, H, site = 2, 5, 2, 3
    D, Lq = H * 64, (1 if form == 'row0' else 5)
    g = torch.Generator().manual_seed(5100)
    q, k, v, do = (torch.randn(*s, generator=g).to(dt).to(DEV) for s in ((B, Lq, D), (B, Lk, D), (B, Lk, D), (B, Lq, D)))
    mask = torch.ones(B, Lk, dtype=torch.uint8)
    mask[1, -2:] = 0
    mask = mask.to(DEV)
    drop = None if p is None else (Lk, SEED, site, p)
    tail = () if drop is None else drop
    code = C.LVL_BF16 if dt == BF else C.LVL_F32
    out, dq, dk, dv = (torch.full_like(t, NAN) for t in (q, q, k, v))
    ws = torch.full((L.lvl_workspace_floats(b'keymask_attn_bwd', B * Lq * H, Lk) + 64,), NAN, device=DEV)
    fwd, bwd = (L.lvl_keymask_attn_fwd, L.lvl_keymask_attn_bwd) if drop is None else (L.lvl_keymask_attn_drop_fwd,
                                                                                     L.lvl_keymask_attn_drop_bwd)
    C.check(fwd(C.ptr(q), C.ptr(k), C.ptr(v), C.ptr(mask), C.ptr(out), B, Lq, Lk, H, D, D, Lk * D, Lk, *tail, code,
                C.stream_ptr()), 'forward')
    C.check(bwd(C.ptr(q), C.ptr(k), C.ptr(v), C.ptr(mask), C.ptr(do), C.ptr(dq), C.ptr(dk), C.ptr(dv), C.ptr(ws), B, Lq, Lk, H,
                D, D, Lk * D, Lk, *tail, code, C.stream_ptr()), 'backward')
    torch.cuda.synchronize()
    for t in (out, dq, dk, dv):
        assert not torch.isnan(t).any(), 'an addressed element was not written'
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    got = ops._KeymaskAttnFn.apply(qa, ka, va, mask, H) if drop is None else ops._KeymaskAttnFn.apply(qa, ka, va, mask, H, drop)
    got.backward(do)
    assert torch.equal(got, out) and torch.equal(qa.grad, dq) and torch.equal(ka.grad, dk) and torch.equal(va.grad, dv)
    assert not dk[1, -2:].any() and not dv[1, -2:].any(), 'dk / dv rows of hidden keys must be exact zeros'
    # the one public function is that Function
    assert torch.equal(ops.keymask_attention(q, k, v, mask, H, drop), out)


def test_error_codes():
    """p outside [0, 1), misaligned pointers, idx_qrep < qrep and a bad row index stride return LVL_EINVAL without a launch."""
    C = _C()
    L = C.lib()
    H, Tk = 1, 8
    x = torch.full((Tk, 192), NAN, dtype=BF, device=DEV)
    out = torch.full((Tk, 64), 7.0, dtype=BF, device=DEV)
    ws = torch.zeros(64, device=DEV)
    q, k, v = C.ptr(x), _off(x, 64), _off(x, 128)

    def fwd(q=q, out=C.ptr(out), p=0.5, iq=Tk, dtype=C.LVL_BF16):
        return L.lvl_keymask_attn_drop_fwd(q, k, v, None, out, 1, Tk, Tk, H, 192, 192, Tk * 192, Tk, iq, SEED, 1, p, dtype,
                                           C.stream_ptr())

    def bwd(dq=C.ptr(x), p=0.5, iq=Tk, ws=C.ptr(ws), dtype=C.LVL_F32):
        return L.lvl_keymask_attn_drop_bwd(q, k, v, None, C.ptr(out), dq, k, v, ws, 1, Tk, Tk, H, 192, 192, Tk * 192, Tk, iq, SEED,
                                           1, p, dtype, C.stream_ptr())
    EINVAL = -22
    for f in (fwd, bwd):
        assert f(p=1.0) == EINVAL and b'[0, 1)' in L.lvl_last_error()
        assert f(p=-0.25) == EINVAL and f(p=float('nan')) == EINVAL
        assert f(iq=Tk - 1) == EINVAL and b'idx_qrep' in L.lvl_last_error()
        assert f(dtype=7) == EINVAL
    assert fwd(q=_off(x, 1)) == EINVAL and b'aligned' in L.lvl_last_error()
    assert fwd(out=_off(out, 3)) == EINVAL and bwd(dq=_off(x, 2)) == EINVAL and bwd(ws=None) == EINVAL
    # the row pair
    r = torch.full((2, 64), 3.0, dtype=BF, device=DEV)
    f32 = torch.zeros(64, device=DEV)
    st = torch.zeros(2, device=DEV)

    def ln(res=C.ptr(r), p=0.5, stride=64, D=64):
        return L.lvl_dropout_add_layernorm_fwd(res, C.ptr(r), C.ptr(f32), C.ptr(f32), 1e-12, C.ptr(out), C.ptr(out), C.ptr(st),
                                               C.ptr(st), 2, D, stride, SEED, 2, p, C.LVL_BF16, C.stream_ptr())

    def ln_bwd(dy=C.ptr(x), p=0.5, stride=64):
        return L.lvl_dropout_add_layernorm_bwd(C.ptr(r), C.ptr(r), C.ptr(f32), C.ptr(st), C.ptr(st), None, C.ptr(x), dy, C.ptr(ws),
                                               C.ptr(ws), C.ptr(ws), 2, 64, stride, SEED, 2, p, C.LVL_BF16, C.stream_ptr())
    assert ln(p=1.0) == EINVAL and ln(p=-1.0) == EINVAL and ln(stride=32) == EINVAL and ln(stride=68) == EINVAL
    assert ln(res=_off(r, 1)) == EINVAL and ln(D=60) == EINVAL
    assert ln_bwd(p=1.0) == EINVAL and ln_bwd(stride=32) == EINVAL and ln_bwd(dy=_off(x, 1)) == EINVAL
    torch.cuda.synchronize()
    assert (out == 7.0).all() and torch.isnan(x).all() and (r == 3.0).all(), 'a refused call launched something'
