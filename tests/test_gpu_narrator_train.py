"""GPU (-m gpu): bf16 training of the narrator -- the backward kernels of the gated decoder and the pooler against float64
autograd of the oracle, then the decoder step, the pooler module and `VCLM_HF.forward` -> CaptionLoss -> backward against the
float64 oracle (which tests/test_narrator_train_cpu.py pins to the reference's own gradients).

Kernel bound: 2^-7 * max|want| per output tensor (bf16 operands, f32 accumulation), as
test_linear_tn_quickgelu_derivative_epilogues. Step bound: the criterion of test_tsfb_bf16_training_step_vs_oracle_f32."""
import math
import types

import pytest
import torch

from caption_loss_reference import rows_forward
from oracle import oracle as O
from lavila_amd.guards import forbid_library_gemm
from test_gpu_narrator import _golden_model, _mid_model
from test_gpu_selective_recompute import _poison

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF = torch.bfloat16
NAN = float('nan')


def _bf(shape, g, scale=1.0):
    """A bf16-rounded random tensor: (device bf16, the same values in float64 on the CPU)."""
    t = (scale * torch.randn(*shape, generator=g)).to(BF)
    return t.to(DEV), t.double()


def _ratio(got, want):
    """max|got - want| / max|want|; the bound is 2^-7."""
    return ((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()


# ----------------------------------------------------------------------------------------------------------------------
# 1. decoder cross-attention
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('contexts,qrep,H,Tk', [(2, 1, 3, 24), (3, 12, 12, 256), (2, 5, 2, 37), (2, 20, 3, 200),
                                                (1, 76, 2, 256), (2, 16, 1, 16), (2, 65, 2, 255), (1, 3, 1, 1)])
def test_cross_attn_rows_bwd(contexts, qrep, H, Tk):
    from lavila_amd import _cabi as C
    g = torch.Generator().manual_seed(100 + qrep + Tk)
    D, rows = H * 64, contexts * qrep
    q, q64 = _bf((rows, D), g)
    kv, kv64 = _bf((contexts, Tk, 2 * D), g)
    do, do64 = _bf((rows, D), g)
    q64.requires_grad_(True)
    kv64.requires_grad_(True)
    out = O.gpt2_attention_core(q64.reshape(contexts, qrep, D), kv64[..., :D], kv64[..., D:], H, causal=False)
    out.backward(do64.reshape(contexts, qrep, D))
    runs = []
    for _ in range(2):
        dq = torch.full((rows, D), NAN, dtype=BF, device=DEV)
        dkv = torch.full((contexts, Tk, 2 * D), NAN, dtype=BF, device=DEV)
        C.check(C.lib().lvl_cross_attn_rows_bwd(C.ptr(q), C.ptr(kv), C.ptr(do), C.ptr(dq), C.ptr(dkv), rows, qrep, Tk, H,
                                                C.dtype_code(q), C.stream_ptr()), 'lvl_cross_attn_rows_bwd')
        torch.cuda.synchronize()
        runs.append((dq, dkv))
    (dq, dkv), (dq2, dkv2) = runs
    assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2)
    assert not torch.isnan(dq).any() and not torch.isnan(dkv).any()
    wq, wk, wv = q64.grad, kv64.grad[..., :D], kv64.grad[..., D:]
    if Tk == 1:                             # the softmax is 1: no gradient reaches the scores
        assert (dq == 0).all() and (dkv[..., :D] == 0).all()
        want = do64.reshape(contexts, qrep, D).sum(1, keepdim=True)
        assert ((dkv[..., D:].double().cpu() - want).abs() <= 2.0 ** -8 * want.abs() + 1e-30).all()
        print(f'[cross_attn_rows_bwd {contexts, qrep, H, Tk}] dq, dk exactly zero; dv within one rounding')
        return
    r = (_ratio(dq, wq), _ratio(dkv[..., :D], wk), _ratio(dkv[..., D:], wv))
    print(f'[cross_attn_rows_bwd {contexts, qrep, H, Tk}] worst ratios dq {r[0]:.2e} dk {r[1]:.2e} dv {r[2]:.2e} (bound {2.0 ** -7:.2e})')
    assert max(r) <= 2.0 ** -7, r


def test_cross_attn_rows_bwd_refuses_what_it_does_not_serve():
    from lavila_amd import _cabi as C
    q = torch.zeros(4, 64, dtype=BF, device=DEV)
    kv = torch.zeros(1, 300, 128, dtype=BF, device=DEV)
    with pytest.raises(C.HipExtensionError, match='256'):
        C.check(C.lib().lvl_cross_attn_rows_bwd(C.ptr(q), C.ptr(kv), C.ptr(q), C.ptr(q.clone()), C.ptr(kv.clone()), 4, 4, 300,
                                                1, C.dtype_code(q), C.stream_ptr()), 'lvl_cross_attn_rows_bwd')
    qf, kvf = q.float(), kv[:, :8].float().contiguous()
    with pytest.raises(C.HipExtensionError, match='bf16'):
        C.check(C.lib().lvl_cross_attn_rows_bwd(C.ptr(qf), C.ptr(kvf), C.ptr(qf), C.ptr(qf.clone()), C.ptr(kvf.clone()), 4, 4, 8,
                                                1, C.dtype_code(qf), C.stream_ptr()), 'lvl_cross_attn_rows_bwd')


# ----------------------------------------------------------------------------------------------------------------------
# 2. pooler core
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shared', [False, True])
@pytest.mark.parametrize('B,NQ,H,Tk', [(2, 24, 4, 65), (1, 5, 3, 9), (2, 7, 1, 1), (2, 256, 8, 785)])
def test_mq_cross_attn_bwd(B, NQ, H, Tk, shared):
    from lavila_amd import _cabi as C
    g = torch.Generator().manual_seed(200 + NQ + Tk)
    D = H * 64
    q, q64 = _bf((NQ, D) if shared else (B, NQ, D), g)
    kv, kv64 = _bf((B, Tk, 128), g)
    do, do64 = _bf((B, NQ, D), g)
    q64.requires_grad_(True)
    kv64.requires_grad_(True)
    O.mq_cross_attention_core(q64[None].expand(B, -1, -1) if shared else q64, kv64, H).backward(do64)
    qb = 0 if shared else NQ * D
    n_ws = C.lib().lvl_mq_cross_attn_bwd_ws(B, NQ, H, int(shared))
    assert n_ws > 0 and C.lib().lvl_mq_cross_attn_bwd_ws(B, 0, H, int(shared)) == -1
    runs = []
    for _ in range(2):
        dq = torch.full_like(q, NAN)
        dkv = torch.full_like(kv, NAN)
        ws = torch.full((n_ws,), NAN, dtype=torch.float32, device=DEV)
        C.check(C.lib().lvl_mq_cross_attn_bwd(C.ptr(q), qb, C.ptr(kv), C.ptr(do), C.ptr(dq), C.ptr(dkv), C.ptr(ws), B, NQ, H,
                                              Tk, C.dtype_code(kv), C.stream_ptr()), 'lvl_mq_cross_attn_bwd')
        torch.cuda.synchronize()
        runs.append((dq, dkv))
    (dq, dkv), (dq2, dkv2) = runs
    assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2)
    assert not torch.isnan(dq).any() and not torch.isnan(dkv).any()
    if Tk == 1:
        assert (dq == 0).all() and (dkv[..., :64] == 0).all()
        r = (0.0, 0.0, _ratio(dkv[..., 64:], kv64.grad[..., 64:]))
    else:
        r = (_ratio(dq, q64.grad), _ratio(dkv[..., :64], kv64.grad[..., :64]), _ratio(dkv[..., 64:], kv64.grad[..., 64:]))
    print(f'[mq_cross_attn_bwd {B, NQ, H, Tk} shared={shared}] worst ratios dq {r[0]:.2e} dk {r[1]:.2e} dv {r[2]:.2e} '
          f'(bound {2.0 ** -7:.2e})')
    assert max(r) <= 2.0 ** -7, r


# ----------------------------------------------------------------------------------------------------------------------
# 3. gated add + LayerNorm, training pair
# ----------------------------------------------------------------------------------------------------------------------
# grid caps: lvl_layernorm_bwd runs at most 768 workgroups of 4 rows (3072 rows per sweep), the dy / dgate pass at most 256
# workgroups of 256 x 8 elements (524288 per sweep): (3100, 192) is past both
@pytest.mark.parametrize('mode', ['gate', 'nogate', 'noy'])
@pytest.mark.parametrize('with_dadd', [True, False])
@pytest.mark.parametrize('rows,D', [(3, 192), (64, 768), (7, 1600), (2, 4096), (5, 8), (300, 256), (3100, 192)])
def test_gated_add_layernorm_pair(rows, D, with_dadd, mode):
    from lavila_amd import _cabi as C
    g = torch.Generator().manual_seed(300 + rows + D)
    eps = 1e-5
    res, res64 = _bf((rows, D), g)
    y, y64 = _bf((rows, D), g) if mode != 'noy' else (None, None)
    dh, dh64 = _bf((rows, D), g)
    dadd, dadd64 = _bf((rows, D), g) if with_dadd else (None, None)
    gamma = 1.0 + 0.2 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    gate = torch.tanh(torch.tensor([0.7])) if mode == 'gate' else None
    gamma_d, beta_d, gate_d = gamma.to(DEV), beta.to(DEV), None if gate is None else gate.to(DEV)

    # forward: the inference kernel, then the training entry
    s0 = torch.empty_like(res) if y is not None else None
    h0 = torch.empty_like(res)
    C.check(C.lib().lvl_gated_add_layernorm(C.ptr(res), C.ptr(y), C.ptr(gate_d), C.ptr(gamma_d), C.ptr(beta_d), eps,
                                            C.ptr(s0), C.ptr(h0), rows, D, C.dtype_code(res), C.stream_ptr()), 'fwd')
    s = torch.full_like(res, NAN) if y is not None else None
    h = torch.full_like(res, NAN)
    mean = torch.full((rows,), NAN, device=DEV)
    rstd = torch.full((rows,), NAN, device=DEV)
    C.check(C.lib().lvl_gated_add_layernorm_train(C.ptr(res), C.ptr(y), C.ptr(gate_d), C.ptr(gamma_d), C.ptr(beta_d), eps,
                                                  C.ptr(s), C.ptr(h), C.ptr(mean), C.ptr(rstd), rows, D,
                                                  C.dtype_code(res), C.stream_ptr()), 'train fwd')
    assert torch.equal(h, h0) and (y is None or torch.equal(s, s0))
    kept = (res if s is None else s)
    k64 = kept.double().cpu()                          # the stored (rounded) sum is what the LayerNorm sees
    # 1e-5 relative: of the row's magnitude for the mean (a mean near zero has no relative scale of its own)
    torch.testing.assert_close(mean.cpu().double(), k64.mean(1), rtol=1e-5, atol=1e-5 * k64.abs().max().item())
    torch.testing.assert_close(rstd.cpu().double(), (k64.var(1, unbiased=False) + eps).rsqrt(), rtol=1e-5, atol=0)

    # float64 autograd of O.layer_norm(res + g * y); dadd is a gradient that arrives at the sum
    r64 = res64.clone().requires_grad_(True)
    yy = None if y64 is None else y64.clone().requires_grad_(True)
    gm, bt = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    s64 = r64 if yy is None else (r64 + (gate.double() * yy if gate is not None else yy))
    tot = (O.layer_norm(s64, gm, bt, eps) * dh64).sum() + ((s64 * dadd64).sum() if with_dadd else 0.0)
    tot.backward()
    ds_want = r64.grad

    runs = []
    for _ in range(2):
        ds = torch.full_like(res, NAN)
        dy = torch.full_like(res, NAN) if mode == 'gate' else None
        dg = torch.full((D,), NAN, device=DEV)
        db = torch.full((D,), NAN, device=DEV)
        dgate = torch.full((1,), NAN, device=DEV) if mode == 'gate' else None
        n_ws = C.lib().lvl_workspace_floats(b'gated_add_layernorm_bwd', rows, D)
        ws = torch.full((n_ws,), NAN, device=DEV)
        C.check(C.lib().lvl_gated_add_layernorm_bwd(C.ptr(dh), C.ptr(kept), C.ptr(y), C.ptr(gate_d), C.ptr(gamma_d),
                                                    C.ptr(mean), C.ptr(rstd), C.ptr(dadd), C.ptr(ds), C.ptr(dy), C.ptr(dg),
                                                    C.ptr(db), C.ptr(dgate), C.ptr(ws), rows, D, C.dtype_code(res),
                                                    C.stream_ptr()), 'bwd')
        torch.cuda.synchronize()
        runs.append((ds, dy, dg, db, dgate))
    for a, b in zip(*runs):
        assert a is None or torch.equal(a, b)
    ds, dy, dg, db, dgate = runs[0]
    r = {'ds': _ratio(ds, ds_want), 'dgamma': _ratio(dg, gm.grad), 'dbeta': _ratio(db, bt.grad)}
    if mode == 'gate':
        r['dy'] = _ratio(dy, yy.grad)
        # the gate gradient's inputs are the kernel's own ds (bf16) and y: exact products, only the f32 summation order differs
        prod = ds.double().cpu() * y64
        err = abs(dgate.item() - prod.sum().item())
        bound = 2.0 ** -8 * prod.abs().sum().item()
        print(f'[gated_add_layernorm_bwd {rows, D}] |dgate - want| {err:.3e} (bound {bound:.3e})')
        assert err <= bound
    print(f'[gated_add_layernorm pair {rows, D} {mode} dadd={with_dadd}] worst ratios {r} (bound {2.0 ** -7:.2e})')
    assert max(r.values()) <= 2.0 ** -7, r


# ----------------------------------------------------------------------------------------------------------------------
# 4. activation derivatives
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', ['gelu_new', 'sq_relu'])
def test_activation_derivatives(act):
    from lavila_amd import _cabi as C
    g = torch.Generator().manual_seed(400)
    u, u64 = _bf((40, 3072), g, 3.0)
    da, da64 = _bf((40, 3072), g)
    which = C.ACT_GELU_NEW if act == 'gelu_new' else C.ACT_SQRELU
    u64.requires_grad_(True)
    a64 = (O.gelu_new if act == 'gelu_new' else O.sq_relu)(u64)
    a64.backward(da64)
    a = torch.full_like(u, NAN)
    du = torch.full_like(u, NAN)
    C.check(C.lib().lvl_act_fwd(C.ptr(u), C.ptr(a), u.numel(), which, C.dtype_code(u), C.stream_ptr()), 'lvl_act_fwd')
    C.check(C.lib().lvl_act_bwd(C.ptr(u), C.ptr(da), C.ptr(du), u.numel(), which, C.dtype_code(u), C.stream_ptr()), 'lvl_act_bwd')
    inplace = u.clone()
    C.check(C.lib().lvl_act_inplace(C.ptr(inplace), u.numel(), which, C.dtype_code(u), C.stream_ptr()), 'lvl_act_inplace')
    assert torch.equal(a, inplace)                       # the out-of-place forward is the inference kernel
    r = (_ratio(a, a64.detach()), _ratio(du, u64.grad))
    print(f'[act {act}] worst ratios forward {r[0]:.2e} derivative {r[1]:.2e} (bound {2.0 ** -7:.2e})')
    assert max(r) <= 2.0 ** -7, r
    if act == 'sq_relu':
        assert (du[u <= 0] == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# 5 - 8. the training plan
# ----------------------------------------------------------------------------------------------------------------------
def _caption_loss64(logits_bvt, labels, pad):
    """The float64 restatement of CaptionLoss (tests/caption_loss_reference.py) with autograd through the logits."""
    B, V, T = logits_bvt.shape
    _, nll, _, _, _ = rows_forward(logits_bvt.permute(0, 2, 1).reshape(B * T, V), labels.reshape(-1), pad)
    return nll.sum() / (B * T)


def _compare_step(tag, got, want, loss, loss_want, extra=()):
    """The criterion of test_tsfb_bf16_training_step_vs_oracle_f32: per tensor ||d|| <= max(1e-1 ||want||, 1e-3 scale),
    aggregate relative L2 <= 5e-2, |loss - oracle| <= 2e-2. got / want: name -> gradient."""
    worst, num, den = [], 0.0, 0.0
    for k, w in want.items():
        assert got[k] is not None and torch.isfinite(got[k]).all(), k
        d = (got[k].double().cpu() - w).norm().item()
        num += d * d
        den += w.norm().item() ** 2
        worst.append((d / max(w.norm().item(), 1e-300), d, w.norm().item(), k))
    agg, scale = math.sqrt(num / den), math.sqrt(den / len(worst))
    bad = [t for t in worst if t[0] > 1e-1 and t[1] > 1e-3 * scale]
    ranked = sorted((t for t in worst if t[2] >= 1e-2 * scale), reverse=True)
    print(f'[{tag}] |d loss| {abs(loss - loss_want):.2e}; gradients: aggregate {agg:.2e}, worst tensor above 1e-2 scale '
          f'{ranked[0][0]:.2e} ({ranked[0][3]}), over {len(worst)} tensors, scale {scale:.3g}' +
          ''.join(f'; {n} {v:.2e}' for n, v in extra))
    assert abs(loss - loss_want) <= 2e-2
    assert agg <= 5e-2, agg
    assert not bad, bad[:5]
    return scale


def _decoder_inputs(d, width, queries, gen_seed=5):
    g = torch.Generator().manual_seed(gen_seed)
    B, L = 3, 12
    ids = torch.randint(1, d['vocab'], (B, L), generator=g)
    labels = torch.randint(1, d['vocab'], (B, L), generator=g)
    labels[0, 9:] = 0
    labels[2, 5:] = 0                                   # pad labels
    enc = torch.randn(B, queries, width, generator=g)
    return ids, labels, enc


def _decoder_oracle(w, ids, labels, enc, heads):
    wo = {k: v.double().requires_grad_(True) for k, v in w.items() if k.startswith('text_decoder.')}
    wo['text_decoder.lm_head.weight'] = wo['text_decoder.transformer.wte.weight']
    eo = enc.double().requires_grad_(True)
    logits, _ = O.gpt2_lm_logits(ids, eo, wo, heads, prefix='text_decoder.')
    loss = _caption_loss64(logits.permute(0, 2, 1), labels, 0)
    loss.backward()
    grads = {k[len('text_decoder.'):]: v.grad for k, v in wo.items() if k != 'text_decoder.lm_head.weight'}
    return loss.item(), grads, eo.grad


def _decoder_step(dec, ids, labels, enc):
    from lavila.models.loss import CaptionLoss
    dec.zero_grad(set_to_none=True)
    e = enc.to(DEV).requires_grad_(True)
    crit = CaptionLoss(tokenizer=types.SimpleNamespace(pad_token_id=0))
    with torch.autocast('cuda', dtype=BF), forbid_library_gemm():
        logits = dec(ids.to(DEV), encoder_hidden_states=e).logits
        out = crit({'text_tokens_logits': logits.permute(0, 2, 1), 'labels': labels.to(DEV)})
        out['loss'].backward()
    torch.cuda.synchronize()
    return out['loss'].item(), {k: p.grad for k, p in dec.named_parameters()}, e.grad


@pytest.mark.parametrize('freq,gated', [(1, True), (2, False)])
def test_decoder_training_step_vs_oracle(freq, gated, monkeypatch):
    from lavila_amd import ops
    m, c, d, w = _mid_model('autocast', freq=freq)
    dec = m.text_decoder
    if not gated:                                       # the plain variant: no tanh gates
        for blk in dec.transformer.h:
            if hasattr(blk, 'alpha_cattn'):
                del blk.alpha_cattn, blk.alpha_dense
        w = {k: v for k, v in w.items() if 'alpha_' not in k}
    H = c['pool_heads']
    ids, labels, enc = _decoder_inputs(d, c['text_width'], c['queries'])
    loss_want, want, denc_want = _decoder_oracle(w, ids, labels, enc, H)
    # the inputs must not hide the new kernels
    scale = math.sqrt(sum(v.norm().item() ** 2 for v in want.values()) / len(want))
    small = [k for k, v in want.items() if v.norm().item() < 1e-2 * scale]
    assert len(small) <= 0.1 * len(want), small
    assert not [k for k in small if k.endswith('crossattention.q_attn.weight') or k.endswith('crossattention.c_attn.weight')]

    calls = []
    real = ops._wgrad
    monkeypatch.setattr(ops, '_wgrad', lambda dy, x, wdt: (calls.append((dy.shape[1], x.shape[1])), real(dy, x, wdt))[1])
    loss, got, denc = _decoder_step(dec, ids, labels, enc)
    n_full = len(calls)
    e_enc = ((denc.double().cpu() - denc_want).norm() / denc_want.norm()).item()
    _compare_step(f'decoder step freq={freq} gated={gated}', got, want, loss, loss_want, [('d enc rel L2', e_enc)])
    assert e_enc <= 1e-1
    n_cross = sum(1 for blk in dec.transformer.h if blk.has_cross)
    assert n_full == 4 * d['layers'] + 5 * n_cross + 1                       # every Conv1D and the tied lm_head

    # freeze_lm_weights(): only the cross-attention side trains, bit for bit as before, on fewer weight-gradient GEMMs
    dec.freeze_lm_weights()
    calls.clear()
    _, frozen, denc_f = _decoder_step(dec, ids, labels, enc)
    assert len(calls) == 5 * n_cross, calls
    for k, p in dec.named_parameters():
        if p.requires_grad:
            assert ('crossattention' in k or 'cross_attn' in k or 'alpha_' in k) and torch.equal(frozen[k], got[k]), k
        else:
            assert frozen[k] is None, k
    assert torch.equal(denc_f, denc)


def test_pooler_module_vs_oracle():
    from lavila_amd.narrator import CrossAttention, LayerNorm
    m, c, d, w = _mid_model('autocast')
    H, width = c['pool_heads'], c['text_width']
    pool, norm, queries = m.img_attn_pool, m.img_attn_pool_norm, m.img_queries
    assert isinstance(pool, CrossAttention) and isinstance(norm, LayerNorm)
    factor = 400.0                                      # the procedural weights give an almost uniform softmax otherwise
    with torch.no_grad():
        pool.to_q.weight.mul_(factor)
    names = ['img_queries'] + [f'img_attn_pool.{k}' for k, _ in pool.named_parameters()] + ['img_attn_pool_norm.gamma']
    wo = {k: w[k].double() for k in names}
    wo['img_attn_pool.to_q.weight'] = wo['img_attn_pool.to_q.weight'] * factor
    wo = {k: v.requires_grad_(True) for k, v in wo.items()}
    g = torch.Generator().manual_seed(6)
    ctx = torch.randn(3, 65, c['dim'], generator=g)
    cot = torch.randn(3, c['queries'], width, generator=g)
    co = ctx.double().requires_grad_(True)
    q = wo['img_queries'][None].expand(3, -1, -1)
    pooled = O.cross_attention_pool(q, co, wo, 'img_attn_pool.', H)
    O.coca_layer_norm(pooled, wo['img_attn_pool_norm.gamma']).mul(cot.double()).sum().backward()
    with torch.no_grad():                               # the scaled scores of the oracle are not degenerate
        xq = O.coca_layer_norm(wo['img_queries'], wo['img_attn_pool.norm.gamma'])
        kv = torch.nn.functional.linear(O.coca_layer_norm(co, wo['img_attn_pool.context_norm.gamma']), wo['img_attn_pool.to_kv.weight'])
        qq = torch.nn.functional.linear(xq, wo['img_attn_pool.to_q.weight']).reshape(-1, H, 64) * 0.125
        sd = torch.einsum('nhd,bjd->bhnj', qq, kv[..., :64]).std().item()
    assert 1.0 <= sd <= 3.0, sd
    m.zero_grad(set_to_none=True)
    cd = ctx.to(DEV).requires_grad_(True)
    with torch.autocast('cuda', dtype=BF):
        norm(pool(queries, cd)).float().mul(cot.to(DEV)).sum().backward()
    got = {'img_queries': queries.grad, 'img_attn_pool_norm.gamma': norm.gamma.grad}
    got.update({f'img_attn_pool.{k}': p.grad for k, p in pool.named_parameters()})
    rel = {k: ((got[k].double().cpu() - wo[k].grad).norm() / wo[k].grad.norm()).item() for k in names}
    rel['context'] = ((cd.grad.double().cpu() - co.grad).norm() / co.grad.norm()).item()
    print(f'[pooler module] score std {sd:.2f}; rel L2 {({k: round(v, 4) for k, v in rel.items()})}')
    assert max(rel.values()) <= 1e-1, rel


@pytest.mark.parametrize('variant', ['freq1_gated', 'freq2_plain'])
def test_narrator_end_to_end_training_step(variant):
    from lavila.models.loss import CaptionLoss
    m, c, d, v, video, tok = _golden_model(variant)
    text = v['text'].to(DEV)
    w = O.narrator_weights(v['shapes'], seed=v['weight_seed'])
    wo = {k: t.double().requires_grad_(True) for k, t in w.items()}
    wo['text_decoder.lm_head.weight'] = wo['text_decoder.transformer.wte.weight']
    oo = O.narrator_forward(video.cpu().double(), v['text'], wo, c['heads'], c['pool_heads'], c['pool_heads'])
    loss_want = _caption_loss64(oo['text_tokens_logits'], oo['labels'], v['pad'])
    loss_want.backward()
    crit = CaptionLoss(tokenizer=tok)

    def step():
        m.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=BF):
            out = m(video, text)
            res = crit(out)
        res['loss'].backward()
        torch.cuda.synchronize()
        return res['loss'].item(), out['text_tokens_logits'].detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}

    loss, logits, got = step()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())     # tower and img_queries included
    want = {k: wo[k].grad for k in got}
    _compare_step(f'narrator step {variant}', got, want, loss, loss_want.item())
    _poison()
    _, logits2, got2 = step()
    assert torch.equal(logits, logits2)
    for k in got:
        assert torch.equal(got[k], got2[k]), k
    opt = torch.optim.AdamW(m.parameters(), lr=1e-2)
    opt.step()
    _, logits3, _ = step()
    assert not torch.equal(logits3, logits)              # the bf16 weight images were refreshed after the optimizer step


def test_training_plan_refusals():
    from lavila_amd._cabi import HipExtensionError
    m, c, d, w = _mid_model('autocast')
    dec = m.text_decoder
    ids = torch.ones(2, 4, dtype=torch.long, device=DEV)
    enc = torch.randn(2, 300, c['text_width'], device=DEV)
    with torch.autocast('cuda', dtype=BF), pytest.raises(HipExtensionError, match='256'):
        dec(ids, encoder_hidden_states=enc)
    with pytest.raises(NotImplementedError):             # float32 with gradients
        dec(ids, encoder_hidden_states=enc[:, :24])
    dec.config.resid_pdrop = 0.1
    dec.train()
    with torch.autocast('cuda', dtype=BF), pytest.raises(NotImplementedError, match='resid_pdrop'):
        dec(ids, encoder_hidden_states=enc[:, :24])
    dec.eval()
    with torch.autocast('cuda', dtype=BF):
        assert dec(ids, encoder_hidden_states=enc[:, :24]).logits.requires_grad
