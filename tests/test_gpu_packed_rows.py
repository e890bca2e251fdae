"""GPU (-m gpu): packed caption rows -- the two row kernels (csrc/pack_rows.hip) against torch indexing, the decoder on
packed rows (`GPT2LMHeadModel.forward(row_lengths=...)`) against the float64 oracle for inference and for the training step,
and `VCLM_HF.forward` with `narrator.PACK_CAPTIONS`.

What the tests rest on: a position behind a caption's last non-pad label has a pad label, so its loss
term is 0, and the causal mask keeps it from every position in front -- dropping it changes no kept row and removes only
gradient terms that are products with an exact zero. NOT claimed: the bits of the padded run (the weight-gradient GEMMs sum
another number of rows). Every ragged case keeps R < B L rows, one caption of length 1 and one of length L."""
import functools
import math
import types

import pytest
import torch

import dropout_reference as R
from caption_loss_reference import reduce3, rows_forward
from oracle import oracle as O
from lavila_amd.guards import forbid_library_gemm
from test_gpu_caption_loss import EPS, _rel, bounds
from test_gpu_decoder_dropout import _attn64, _kernel_mask
from test_gpu_narrator import _golden_model, _mid_model
from test_gpu_narrator_train import _caption_loss64, _compare_step, _decoder_oracle
from test_gpu_selective_recompute import _poison

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF = torch.bfloat16
NAN = float('nan')
SENTINEL = 7.0


# ----------------------------------------------------------------------------------------------------------------------
# 1. the kernels
# ----------------------------------------------------------------------------------------------------------------------
def _C():
    from lavila_amd import _cabi as C
    return C


def _cu(lengths):
    return torch.tensor([0] + torch.tensor(lengths).cumsum(0).tolist(), dtype=torch.int32, device=DEV)


def _rect(B, L, D, stride, dt, fill):
    """A [B, L, D] view with row stride `stride` into a buffer of B L + 2 rows filled with `fill`: (buffer, view)."""
    buf = torch.full((B * L + 2, stride), fill, dtype=dt, device=DEV)
    return buf, buf[:B * L].view(B, L, stride)[:, :, :D]


def _pack_into(src, cu, dst):
    C = _C()
    B, L, D = src.shape
    C.check(C.lib().lvl_rows_pack(C.ptr(src), src.stride(0), src.stride(1), C.ptr(cu), B, L, D, C.ptr(dst), C.dtype_code(src),
                                  C.stream_ptr()), 'lvl_rows_pack')


def _unpack_into(src, cu, dst):
    C = _C()
    B, L, D = dst.shape
    C.check(C.lib().lvl_rows_unpack(C.ptr(src), C.ptr(cu), B, L, D, C.ptr(dst), dst.stride(0), dst.stride(1),
                                    C.dtype_code(src), C.stream_ptr()), 'lvl_rows_unpack')


def _check_pair(B, L, D, lengths, dt, strided, seed):
    g = torch.Generator().manual_seed(seed)
    stride = D + 8 if strided else D
    keep = (torch.arange(L)[None] < torch.tensor(lengths)[:, None]).to(DEV)             # [B, L]
    rows = int(keep.sum())
    x = torch.randn(B, L, D, generator=g).to(dt).to(DEV)
    # pack: NaN behind the source's last row and in its columns [D, stride); sentinel rows behind the result
    src_buf, src = _rect(B, L, D, stride, dt, NAN)
    src.copy_(x)
    dst = torch.full((rows + 2, D), SENTINEL, dtype=dt, device=DEV)
    cu = _cu(lengths)
    _pack_into(src, cu, dst)
    assert torch.equal(dst[:rows], x[keep]) and (dst[rows:] == SENTINEL).all()
    # unpack: NaN rows behind the packed rows; sentinel rows behind the rectangle and sentinel columns in [D, stride)
    y = torch.randn(rows, D, generator=g).to(dt).to(DEV)
    ysrc = torch.cat([y, torch.full((2, D), NAN, dtype=dt, device=DEV)])
    out_buf, out = _rect(B, L, D, stride, dt, SENTINEL)
    _unpack_into(ysrc, cu, out)
    want = torch.zeros(B, L, D, dtype=dt, device=DEV)
    want[keep] = y
    assert torch.equal(out, want)
    assert (out_buf[B * L:] == SENTINEL).all() and (out_buf[:, D:] == SENTINEL).all()
    # each undoes the other on the kept rows
    back_buf, back = _rect(B, L, D, stride, dt, SENTINEL)
    _unpack_into(dst, cu, back)
    assert torch.equal(back, x * keep[:, :, None])
    again = torch.full((rows + 2, D), SENTINEL, dtype=dt, device=DEV)
    _pack_into(out, cu, again)
    assert torch.equal(again[:rows], y) and (again[rows:] == SENTINEL).all()
    return x, y, keep, cu, rows


@pytest.mark.parametrize('strided', [False, True])
@pytest.mark.parametrize('dt', [BF, torch.float32])
@pytest.mark.parametrize('D', [8, 768, 1600])
def test_row_kernels_equal_torch_indexing(D, dt, strided):
    from lavila_amd import ops
    lengths = (12, 1, 7, 0, 12)                                      # the raw kernels take an empty caption
    x, y, keep, cu, rows = _check_pair(5, 12, D, lengths, dt, strided, seed=D)
    # the host wrappers and the autograd pair: each one's backward is the other
    assert torch.equal(ops.rows_pack_raw(x, cu, rows), x[keep])
    xr, yr = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    dy, dx = torch.randn_like(y), torch.randn_like(x)
    ops.pack_rows(xr, cu, rows).backward(dy)
    ops.unpack_rows(yr, cu, 5, 12).backward(dx)
    assert torch.equal(xr.grad, ops.rows_unpack_raw(dy, cu, 5, 12)) and torch.equal(yr.grad, dx[keep])


@pytest.mark.parametrize('dt', [BF, torch.float32])
def test_row_kernels_past_the_grid_cap(dt):
    """4096 workgroups of 256 threads is the cap; a row of D = 256 takes 32 (bf16) / 64 (f32) lanes, so 81920 rows make
    10240 / 20480 row groups: every workgroup strides."""
    B, L = 4096, 20
    lengths = torch.randint(0, L + 1, (B,), generator=torch.Generator().manual_seed(3))
    lengths[0], lengths[1], lengths[-1] = L, 1, L
    _check_pair(B, L, 256, lengths.tolist(), dt, False, seed=4)


def test_row_kernels_refuse_what_they_do_not_serve():
    C = _C()
    x = torch.zeros(2, 4, 16, dtype=BF, device=DEV)
    flat = torch.zeros(2 * 4 * 16 + 8, dtype=BF, device=DEV)
    cu = _cu([4, 2])
    out = torch.zeros(6, 16, dtype=BF, device=DEV)
    import ctypes
    off = ctypes.c_void_p(flat.data_ptr() + 2)

    def pack(src, D, dtype):
        C.check(C.lib().lvl_rows_pack(src, 4 * 16, 16, C.ptr(cu), 2, 4, D, C.ptr(out), dtype, C.stream_ptr()), 'lvl_rows_pack')

    def unpack(dst, D, dtype):
        C.check(C.lib().lvl_rows_unpack(C.ptr(out), C.ptr(cu), 2, 4, D, dst, 4 * 16, 16, dtype, C.stream_ptr()),
                'lvl_rows_unpack')

    for call, ptr in ((pack, C.ptr(x)), (unpack, C.ptr(x))):
        with pytest.raises(C.HipExtensionError, match='aligned'):
            call(off, 16, C.LVL_BF16)
        with pytest.raises(C.HipExtensionError, match='multiple of 8'):
            call(ptr, 12, C.LVL_BF16)
        with pytest.raises(C.HipExtensionError, match='dtype'):
            call(ptr, 16, 7)
    torch.cuda.synchronize()
    assert (out == 0).all() and (x == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# the decoder's inputs: B = 4 captions of L = 12 positions, 24 image tokens; 27 of 48 rows are kept
# ----------------------------------------------------------------------------------------------------------------------
B, L, LENGTHS = 4, 12, (12, 9, 5, 1)
ROWS = sum(LENGTHS)


@functools.lru_cache(maxsize=None)
def _inputs(vocab=331, width=256, queries=24):
    g = torch.Generator().manual_seed(17)
    ids = torch.randint(1, vocab, (B, L), generator=g)
    ids[0, 3] = 0                                        # the pad id INSIDE caption 0: the token "!", its row stays
    labels = torch.randint(1, vocab, (B, L), generator=g)
    labels[0, 5] = 0                                     # ... and as a label inside a caption: ignored, the row stays
    for b, n in enumerate(LENGTHS):
        labels[b, n:] = 0
    enc = torch.randn(B, queries, width, generator=g)
    assert ROWS < B * L and 1 in LENGTHS and L in LENGTHS
    from lavila_amd.narrator import caption_row_lengths
    assert tuple(caption_row_lengths(labels, 0).tolist()) == LENGTHS
    return ids, labels, enc


def _kept():
    return torch.arange(L)[None] < torch.tensor(LENGTHS)[:, None]        # [B, L] bool


def _packed_step(dec, ids, labels, enc, lengths, between=None):
    """forward(row_lengths=lengths) -> CaptionLoss -> backward: (loss, logits, parameter gradients, image-token gradient)."""
    from lavila.models.loss import CaptionLoss
    dec.zero_grad(set_to_none=True)
    e = enc.to(DEV).requires_grad_(True)
    crit = CaptionLoss(tokenizer=types.SimpleNamespace(pad_token_id=0))
    kw = {} if lengths is None else dict(row_lengths=lengths)
    with torch.autocast('cuda', dtype=BF), forbid_library_gemm():
        logits = dec(ids.to(DEV), encoder_hidden_states=e, **kw).logits
        out = crit({'text_tokens_logits': logits.permute(0, 2, 1), 'labels': labels.to(DEV)})
        if between is not None:
            between()
        out['loss'].backward()
    torch.cuda.synchronize()
    return out['loss'].item(), logits.detach().clone(), {k: p.grad for k, p in dec.named_parameters()}, e.grad


def _same_step(a, b):
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    for k in a[2]:
        assert (a[2][k] is None and b[2][k] is None) or torch.equal(a[2][k], b[2][k]), k


# ----------------------------------------------------------------------------------------------------------------------
# 2. inference against the float64 oracle
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['bf16', 'f32'])
def test_packed_decoder_inference_vs_oracle(mode):
    m, c, d, w = _mid_model(mode)
    ids, _, enc = _inputs()
    want, _ = O.gpt2_lm_logits(ids, enc, w, c['pool_heads'], prefix='text_decoder.')
    dec = m.text_decoder.bfloat16() if mode == 'bf16' else m.text_decoder
    enc_dev = enc.to(DEV).bfloat16() if mode == 'bf16' else enc.to(DEV)
    kept = _kept()
    with torch.no_grad(), forbid_library_gemm():
        got = dec(ids.to(DEV), encoder_hidden_states=enc_dev, row_lengths=torch.tensor(LENGTHS, device=DEV)).logits
        listed = dec(ids.to(DEV), encoder_hidden_states=enc_dev, row_lengths=list(LENGTHS)).logits
        host = dec(ids.to(DEV), encoder_hidden_states=enc_dev, row_lengths=torch.tensor(LENGTHS, dtype=torch.int32)).logits
        plain = dec(ids.to(DEV)[:, :5], row_lengths=[5, 4, 5, 1]).logits              # no image tokens: plain GPT-2
    assert torch.equal(got, listed) and torch.equal(got, host)
    assert got.shape == (B, L, d['vocab']) and got.dtype == (BF if mode == 'bf16' else torch.float32)
    got = got.float().cpu()
    assert (got[~kept] == 0).all()                                            # exact zeros at and behind len_b
    if mode == 'bf16':                                                        # the bars of test_gpu_narrator.py:579 / :604
        err, scale = (got[kept] - want[kept]).abs().max().item(), want[kept].abs().max().item()
        print(f'[packed inference bf16] max err {err:.3e} of scale {scale:.3e}')
        assert err < 0.04 * scale
    else:
        torch.testing.assert_close(got[kept], want[kept].float(), atol=2e-3, rtol=1e-3)
    assert (plain[1, 4] == 0).all() and plain[1, 3].abs().max() > 0 and plain[3, 1:].abs().max() == 0


# ----------------------------------------------------------------------------------------------------------------------
# 3. what lies behind len_b is never read
# ----------------------------------------------------------------------------------------------------------------------
def test_packed_step_never_reads_behind_the_lengths():
    m, c, d, w = _mid_model('autocast')
    dec = m.text_decoder
    ids, labels, enc = _inputs()
    other = ids.clone()
    other[~_kept()] = (ids[~_kept()] + 100) % d['vocab']                     # other tokens behind every caption
    assert not torch.equal(other, ids) and torch.equal(other[_kept()], ids[_kept()])
    a = _packed_step(dec, ids, labels, enc, list(LENGTHS))
    _poison()                                        # what the next run's buffers (the rectangles' filler too) start as: NaN
    b = _packed_step(dec, other, labels, enc, list(LENGTHS), between=_poison)
    _same_step(a, b)
    assert all(torch.isfinite(g).all() for g in b[2].values()) and torch.isfinite(b[3]).all()
    assert (a[1][~_kept().to(DEV)] == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# 4. the training step against the oracle
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('freq,gated', [(1, True), (2, False)])
def test_packed_training_step_vs_oracle(freq, gated):
    m, c, d, w = _mid_model('autocast', freq=freq)
    dec = m.text_decoder
    if not gated:                                       # the plain variant: no tanh gates
        for blk in dec.transformer.h:
            if hasattr(blk, 'alpha_cattn'):
                del blk.alpha_cattn, blk.alpha_dense
        w = {k: v for k, v in w.items() if 'alpha_' not in k}
    ids, labels, enc = _inputs()
    loss_want, want, denc_want = _decoder_oracle(w, ids, labels, enc, c['pool_heads'])
    # the inputs must not hide the kernels (the asserts of test_decoder_training_step_vs_oracle)
    scale = math.sqrt(sum(v.norm().item() ** 2 for v in want.values()) / len(want))
    small = [k for k, v in want.items() if v.norm().item() < 1e-2 * scale]
    assert len(small) <= 0.1 * len(want), small
    assert not [k for k in small if k.endswith('crossattention.q_attn.weight') or k.endswith('crossattention.c_attn.weight')]

    first = _packed_step(dec, ids, labels, enc, torch.tensor(LENGTHS, device=DEV))
    loss, logits, got, denc = first
    e_enc = ((denc.double().cpu() - denc_want).norm() / denc_want.norm()).item()
    _compare_step(f'packed decoder step freq={freq} gated={gated}', got, want, loss, loss_want, [('d enc rel L2', e_enc)])
    assert e_enc <= 1e-1
    _same_step(first, _packed_step(dec, ids, labels, enc, list(LENGTHS)))          # repeats are bit-identical

    dec.freeze_lm_weights()
    _, logits_f, frozen, denc_f = _packed_step(dec, ids, labels, enc, list(LENGTHS))
    assert torch.equal(logits_f, logits) and torch.equal(denc_f, denc)
    for k, p in dec.named_parameters():
        if p.requires_grad:
            assert ('crossattention' in k or 'cross_attn' in k or 'alpha_' in k) and torch.equal(frozen[k], got[k]), k
        else:
            assert frozen[k] is None, k


# ----------------------------------------------------------------------------------------------------------------------
# 5. work accounting
# ----------------------------------------------------------------------------------------------------------------------
def test_packed_step_runs_its_gemms_on_the_kept_rows(monkeypatch):
    """Every decoder GEMM of a packed step works on R = 27 rows (the image keys / values on the 4 x 24 image tokens), none on
    the B L = 48 of the padded run; with every length equal to L the packed run IS the padded one: same kernels, same rows."""
    from lavila_amd import ops
    m, c, d, w = _mid_model('autocast')
    dec = m.text_decoder
    ids, labels, enc = _inputs()
    seen = []
    real_tn, real_wgrad = ops.linear_tn_raw, ops._wgrad
    monkeypatch.setattr(ops, 'linear_tn_raw', lambda x, *a, **k: (seen.append(('tn', x.shape[0])), real_tn(x, *a, **k))[1])
    monkeypatch.setattr(ops, '_wgrad', lambda dy, x, wdt: (seen.append(('wgrad', dy.shape[0])), real_wgrad(dy, x, wdt))[1])
    image_rows, n_cross = B * enc.shape[1], sum(1 for blk in dec.transformer.h if blk.has_cross)
    convs = 4 * d['layers'] + 4 * n_cross + 1                    # the caption-row Conv1Ds and the lm_head

    padded = _packed_step(dec, ids, labels, enc, None)
    assert {r for _, r in seen} == {B * L, image_rows}
    n_tn, n_wgrad = sum(k == 'tn' for k, _ in seen), sum(k == 'wgrad' for k, _ in seen)
    seen.clear()
    packed = _packed_step(dec, ids, labels, enc, list(LENGTHS))
    assert {r for _, r in seen} == {ROWS, image_rows}, seen
    assert sum(k == 'tn' for k, _ in seen) == n_tn and sum(k == 'wgrad' for k, _ in seen) == n_wgrad
    assert sum(1 for k, r in seen if k == 'wgrad' and r == ROWS) == convs
    assert sum(1 for k, r in seen if k == 'tn' and r == ROWS) == 2 * convs              # forward and input gradient
    kept = _kept().to(DEV)
    assert not torch.equal(packed[1], padded[1]) and (packed[1][~kept] == 0).all()

    full = _packed_step(dec, ids, labels, enc, [L] * B)
    assert torch.equal(full[1], padded[1])
    with torch.no_grad(), torch.autocast('cuda', dtype=BF):      # ... and on the inference image
        e = enc.to(DEV)
        assert torch.equal(dec(ids.to(DEV), encoder_hidden_states=e, row_lengths=[L] * B).logits,
                           dec(ids.to(DEV), encoder_hidden_states=e).logits)


# ----------------------------------------------------------------------------------------------------------------------
# 6. VCLM_HF.forward -> CaptionLoss -> backward with the switch
# ----------------------------------------------------------------------------------------------------------------------
def test_narrator_end_to_end_with_packed_captions(monkeypatch):
    from lavila.models.loss import CaptionLoss
    from lavila_amd import narrator as N
    m, c, d, v, video, tok = _golden_model('freq1_gated')
    text_cpu = v['text'].clone()
    text_cpu[2, 2:] = v['pad']                           # caption 2 keeps one label; caption 1 has its own pads; caption 0 is full
    T = text_cpu.shape[1] - 1
    lengths = N.caption_row_lengths(text_cpu[:, 1:], v['pad']).tolist()
    assert lengths[0] == T and lengths[2] == 1 and sum(lengths) < len(lengths) * T
    assert m.caption_pad_id == v['pad']
    text = text_cpu.to(DEV)
    crit = CaptionLoss(tokenizer=tok)

    def step():
        m.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=BF):
            out = m(video, text)
            res = crit(out)
        res['loss'].backward()
        torch.cuda.synchronize()
        return res, out, {k: p.grad.clone() for k, p in m.named_parameters()}

    assert N.PACK_CAPTIONS is None and not N.pack_captions_enabled()
    _, out_before, grads_before = step()                 # before the switch was ever touched

    wo = {k: t.double().requires_grad_(True) for k, t in O.narrator_weights(v['shapes'], seed=v['weight_seed']).items()}
    wo['text_decoder.lm_head.weight'] = wo['text_decoder.transformer.wte.weight']
    oo = O.narrator_forward(video.cpu().double(), text_cpu, wo, c['heads'], c['pool_heads'], c['pool_heads'])
    loss_want = _caption_loss64(oo['text_tokens_logits'], oo['labels'], v['pad'])
    loss_want.backward()

    monkeypatch.setattr(N, 'PACK_CAPTIONS', True)
    res, out, got = step()
    assert list(out) == ['text_tokens_logits', 'labels'] and torch.equal(out['labels'], text[:, 1:])
    logits = out['text_tokens_logits']
    assert logits.shape == out_before['text_tokens_logits'].shape and logits.dtype == BF
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    _compare_step('narrator step, packed captions', got, {k: wo[k].grad for k in got}, res['loss'].item(), loss_want.item())
    kept = (torch.arange(T)[None] < torch.tensor(lengths)[:, None]).to(DEV)
    rows = logits.detach().permute(0, 2, 1)
    assert (rows[~kept] == 0).all() and not torch.equal(rows, out_before['text_tokens_logits'].permute(0, 2, 1))
    # the criterion's outputs against float64 on the returned logits (the bars of test_module_bf16_against_float64_...)
    V = rows.shape[-1]
    x64 = rows.double().cpu().reshape(-1, V)
    _, nll, _, correct, counted = rows_forward(x64, text_cpu[:, 1:].reshape(-1), v['pad'])
    want3 = reduce3(nll, correct, counted, len(lengths), T)
    _, nll_tol, _, _ = bounds(BF, V, 16.0)
    assert x64.abs().max() <= 16.0
    n_add = T + 1 + 6 + 4
    assert abs(res['loss'].item() - want3[0].item()) <= nll_tol + (n_add + 1) * EPS * want3[0].item()
    assert torch.equal(res['caption_loss'], res['loss'])
    assert res['caption_acc'].item() == pytest.approx(want3[1].item(), rel=4 * EPS)
    worst_nll = 16 + math.log(V) + 16
    assert _rel(res['ppl'].item(), want3[2].item()) <= math.expm1(nll_tol) + (T + 1) * EPS * worst_nll + (n_add + 5) * EPS

    monkeypatch.setattr(N, 'PACK_CAPTIONS', False)       # off again: the default path did not move
    _, out_after, grads_after = step()
    assert torch.equal(out_after['text_tokens_logits'], out_before['text_tokens_logits'])
    for k in grads_before:
        assert torch.equal(grads_after[k], grads_before[k]), k


# ----------------------------------------------------------------------------------------------------------------------
# 7. dropout on packed rows
# ----------------------------------------------------------------------------------------------------------------------
def _packed_dropout_masks(seed, p, heads, width, queries, layers, cross):
    """The masks a packed step applies, read from lvl_dropout_mask: row sites index their elements as packed_row * D + col
    (laid out here on [B, L, D]; what lies behind len_b is never used), attention sites as on the rectangle [B, longest]."""
    kept, longest = _kept(), max(LENGTHS)

    def row_site(site):
        full = torch.ones(B, L, width, dtype=torch.bool)
        full[kept] = _kernel_mask(seed, site, 0, ROWS * width, p).reshape(ROWS, width)
        return full

    def attn_site(site, keys, all_keys):                 # `longest` queries over `keys` keys, laid out on [B, H, L, all_keys]
        full = torch.ones(B, heads, L, all_keys, dtype=torch.bool)
        mask = _kernel_mask(seed, site, 0, B * heads * longest * 256, p).reshape(B, heads, longest, 256)[..., :keys]
        full[:, :, :longest, :keys] = mask
        return full

    masks = {0: row_site(0)}
    for i in range(layers):
        s = R.site_of(i, 0)
        if cross(i):
            masks.update({s: attn_site(s, queries, queries), s + 1: row_site(s + 1), s + 2: row_site(s + 2)})
        masks.update({s + 3: attn_site(s + 3, longest, L), s + 4: row_site(s + 4), s + 5: row_site(s + 5)})
    return masks


def _dropout_decoder64(w, ids, enc, heads, masks, scale, eps=1e-5):
    """O.gpt2_lm_logits in float64 with the reference's dropout sites (gpt2_gated.py:186-187, 230, 354, 389-395, 737, 899)
    under explicit masks."""
    p = 'text_decoder.transformer.'
    D = w[p + 'wte.weight'].shape[1]
    depth = 1 + max(int(k[len(p) + 2:].split('.')[0]) for k in w if k.startswith(p + 'h.'))
    drop = lambda t, site: t * masks[site].double() * scale                   # noqa: E731
    x = drop(w[p + 'wte.weight'][ids] + w[p + 'wpe.weight'][:ids.shape[1]], 0)
    for i in range(depth):
        b, s = f'{p}h.{i}.', R.site_of(i, 0)
        if (b + 'crossattention.q_attn.weight') in w:
            h = O.layer_norm(x, w[b + 'ln_cross_attn.weight'], w[b + 'ln_cross_attn.bias'], eps)
            q = O.conv1d(h, w[b + 'crossattention.q_attn.weight'], w[b + 'crossattention.q_attn.bias'])
            kv = O.conv1d(enc, w[b + 'crossattention.c_attn.weight'], w[b + 'crossattention.c_attn.bias'])
            a = _attn64(q, kv[..., :D], kv[..., D:], heads, False, masks[s], scale)
            a = drop(O.conv1d(a, w[b + 'crossattention.c_proj.weight'], w[b + 'crossattention.c_proj.bias']), s + 1)
            x = x + (torch.tanh(w[b + 'alpha_cattn']) * a if (b + 'alpha_cattn') in w else a)
            h = O.layer_norm(x, w[b + 'ln_2_crossattention.weight'], w[b + 'ln_2_crossattention.bias'], eps)
            f = drop(O.gpt2_mlp(h, w, b + 'mlp_crossattention.', squared_relu=True), s + 2)
            x = x + (torch.tanh(w[b + 'alpha_dense']) * f if (b + 'alpha_dense') in w else f)
        h = O.layer_norm(x, w[b + 'ln_1.weight'], w[b + 'ln_1.bias'], eps)
        qkv = O.conv1d(h, w[b + 'attn.c_attn.weight'], w[b + 'attn.c_attn.bias'])
        a = _attn64(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], heads, True, masks[s + 3], scale)
        x = x + drop(O.conv1d(a, w[b + 'attn.c_proj.weight'], w[b + 'attn.c_proj.bias']), s + 4)
        h = O.layer_norm(x, w[b + 'ln_2.weight'], w[b + 'ln_2.bias'], eps)
        x = x + drop(O.gpt2_mlp(h, w, b + 'mlp.', squared_relu=False), s + 5)
    x = O.layer_norm(x, w[p + 'ln_f.weight'], w[p + 'ln_f.bias'], eps)
    return x @ w[p + 'wte.weight'].t()


def test_packed_dropout_step(monkeypatch):
    from lavila_amd import gpt2_gated as G
    m, c, d, w = _mid_model('autocast')
    dec = m.text_decoder
    ids, labels, enc = _inputs()
    prob, heads = 0.1, c['pool_heads']
    scale = float(R.scale(prob))
    has_cross = lambda i: dec.transformer.h[i].has_cross                      # noqa: E731

    def oracle(seed):
        masks = _packed_dropout_masks(seed, prob, heads, c['text_width'], enc.shape[1], d['layers'], has_cross)
        wo = {k: t.double().requires_grad_(True) for k, t in w.items()
              if k.startswith('text_decoder.') and k != 'text_decoder.lm_head.weight'}     # tied: the oracle reads wte
        eo = enc.double().requires_grad_(True)
        loss = _caption_loss64(_dropout_decoder64(wo, ids, eo, heads, masks, scale).permute(0, 2, 1), labels, 0)
        loss.backward()
        return loss.item(), {k[len('text_decoder.'):]: t.grad for k, t in wo.items()}, eo.grad, masks

    # The seed is chosen from the ORACLE's numbers alone, by the rule of tests/golden/narrator_dropout.pt:
    # the first candidate under which no gradient norm falls below a tenth of the step's without dropout. A gate's gradient is
    # one number; where the masks make it cancel, a relative bound on it measures the rounding of terms many times larger.
    _, plain, _ = _decoder_oracle(w, ids, labels, enc, heads)
    for seed in range(0x9E3779B97F4A7C15, 0x9E3779B97F4A7C15 + 8):
        loss_want, want, denc_want, masks = oracle(seed)
        low = {k: (v.norm() / plain[k].norm()).item() for k, v in want.items() if v.norm() < 0.1 * plain[k].norm()}
        print(f'[packed dropout] seed {seed:#x}: gradient norms below a tenth of the step without dropout: {low}')
        if not low:
            break
    else:
        raise AssertionError('no candidate seed leaves every gradient norm above a tenth of the step without dropout')
    monkeypatch.setattr(G, 'DECODER_DROPOUT', True)
    for k in ('resid_pdrop', 'embd_pdrop', 'attn_pdrop'):
        setattr(dec.config, k, prob)
    dec.train()
    assert dec.applies_dropout()
    with G.fixed_dropout_seed(seed):
        first = _packed_step(dec, ids, labels, enc, list(LENGTHS))
        _same_step(first, _packed_step(dec, ids, labels, enc, torch.tensor(LENGTHS, device=DEV)))
    with G.fixed_dropout_seed(seed ^ 1):
        other = _packed_step(dec, ids, labels, enc, list(LENGTHS))
    assert not torch.equal(other[1], first[1])
    with G.fixed_dropout_seed(seed):                       # another random stream than the padded run's: caption 2's rows start
        padded = _packed_step(dec, ids, labels, enc, None)     # at packed row 21, not 24 (caption 0's sit at 0 in both)
    assert torch.equal(padded[1][0], first[1][0]) and not torch.equal(padded[1][2, :LENGTHS[2]], first[1][2, :LENGTHS[2]])

    assert 0.05 < 1 - masks[0][_kept()].float().mean().item() < 0.15
    loss, _, got, denc = first
    e_enc = ((denc.double().cpu() - denc_want).norm() / denc_want.norm()).item()
    _compare_step('packed decoder step with dropout', got, want, loss, loss_want, [('d enc rel L2', e_enc)])
    assert e_enc <= 1e-1
    with pytest.raises(AssertionError):                    # the criterion sees another seed's masks
        _compare_step('packed decoder step with dropout, wrong seed', other[2], want, other[0], loss_want)
