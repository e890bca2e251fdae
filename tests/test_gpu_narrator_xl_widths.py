"""GPU (-m gpu): a gated decoder whose widths are multiples of 64 but not of 256 trains and runs teacher-forced on the
project's own GEMMs -- forward, input gradient and weight gradient -- under guards.forbid_library_gemm().

Width 320 with 5 heads is the smallest GPT-2 layout with GPT-2 XL's arithmetic (1600 = 25 heads of 64): c_attn 960 has the
column remainder 192, c_proj / q_attn 320 have 64, the cross c_attn 640 has 128, c_fc 1280 tiles, and every weight-gradient
side is a multiple of 160. It carries the comparison against the float64 oracle (procedure and bars of
test_gpu_narrator_train.py::test_decoder_training_step_vs_oracle); width 1600 itself is run for finiteness and repeatability."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import oracle as O
from test_gpu_narrator import _mid_model
from test_gpu_narrator_train import _compare_step, _decoder_inputs, _decoder_oracle, _decoder_step

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF = torch.bfloat16


def _plain(dec, w):
    """the variant without tanh gates"""
    for blk in dec.transformer.h:
        if hasattr(blk, 'alpha_cattn'):
            del blk.alpha_cattn, blk.alpha_dense
    return {k: v for k, v in w.items() if 'alpha_' not in k}


# (4, 2, True) is XL's layout: cross-attention in every second block
@pytest.mark.parametrize('layers,freq,gated', [(2, 1, True), (2, 2, False), (4, 2, True)])
def test_decoder_320_training_step_vs_oracle(layers, freq, gated, monkeypatch):
    from lavila_amd import ops
    m, c, d, w = _mid_model('autocast', width=320, heads=5, layers=layers, freq=freq)
    dec = m.text_decoder
    if not gated:
        w = _plain(dec, w)
    H = c['pool_heads']
    ids, labels, enc = _decoder_inputs(d, c['text_width'], c['queries'])
    loss_want, want, denc_want = _decoder_oracle(w, ids, labels, enc, H)
    # the inputs must not hide the kernels under test (the condition of test_decoder_training_step_vs_oracle)
    scale = math.sqrt(sum(v.norm().item() ** 2 for v in want.values()) / len(want))
    small = [k for k, v in want.items() if v.norm().item() < 1e-2 * scale]
    assert len(small) <= 0.1 * len(want), small
    assert not [k for k in small if k.endswith('crossattention.q_attn.weight') or k.endswith('crossattention.c_attn.weight')]

    calls, gemms = [], {'tn': 0, 'ragged': 0}
    real, real_tn, real_rg = ops._wgrad, ops.linear_tn_raw, ops.linear_tn_ragged_raw
    monkeypatch.setattr(ops, '_wgrad', lambda dy, x, wdt: (calls.append((dy.shape[1], x.shape[1])), real(dy, x, wdt))[1])
    monkeypatch.setattr(ops, 'linear_tn_raw', lambda *a, **k: (gemms.__setitem__('tn', gemms['tn'] + 1), real_tn(*a, **k))[1])
    monkeypatch.setattr(ops, 'linear_tn_ragged_raw',
                        lambda *a, **k: (gemms.__setitem__('ragged', gemms['ragged'] + 1), real_rg(*a, **k))[1])
    loss, got, denc = _decoder_step(dec, ids, labels, enc)          # under forbid_library_gemm()
    n_full = len(calls)
    e_enc = ((denc.double().cpu() - denc_want).norm() / denc_want.norm()).item()
    _compare_step(f'decoder 320 step layers={layers} freq={freq} gated={gated}', got, want, loss, loss_want,
                  [('d enc rel L2', e_enc)])
    assert e_enc <= 1e-1
    n_cross = sum(1 for blk in dec.transformer.h if blk.has_cross)
    assert n_full == 4 * layers + 5 * n_cross + 1                   # every Conv1D and the tied lm_head
    # forward + input gradient of every Conv1D and of the lm_head; the image tokens want a gradient too. On lvl_linear_tn:
    # c_fc forward and the MLP c_proj's input gradient (1280 columns each) and the lm_head forward (512); everything else
    # -- c_fc's input gradient and the lm_head's included -- has a ragged width
    n_mlp = layers + n_cross
    assert gemms == {'tn': 2 * n_mlp + 1, 'ragged': 2 * (4 * layers + 5 * n_cross + 1) - 2 * n_mlp - 1}, gemms

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


def test_decoder_320_teacher_forced_forward_on_own_gemms(monkeypatch):
    """bf16 parameters, many-rows branch forced (row thresholds 0) as test_decoder_low_precision_on_own_gemms does: the ragged
    entry serves c_attn / c_proj / q_attn / the cross c_attn / the MLP's c_proj, lvl_linear_tn serves c_fc and the lm_head."""
    from lavila_amd import gpt2_gated as G
    from lavila_amd import ops
    m, c, d, w = _mid_model('bf16', width=320, heads=5, layers=2, freq=1)
    H = c['pool_heads']
    g = torch.Generator().manual_seed(9)
    B, L, NQ = 3, 11, c['queries']
    ids = torch.randint(1, d['vocab'], (B, L), generator=g)
    enc = torch.randn(B, NQ, c['text_width'], generator=g)
    want, _ = O.gpt2_lm_logits(ids, enc, w, H, prefix='text_decoder.')
    calls = {'tn': [], 'ragged': []}
    real_tn, real_rg = ops.linear_tn_raw, ops.linear_tn_ragged_raw
    monkeypatch.setattr(ops, 'linear_tn_raw', lambda x, w_, *a, **k: (calls['tn'].append(w_.shape[0]), real_tn(x, w_, *a, **k))[1])
    monkeypatch.setattr(ops, 'linear_tn_ragged_raw',
                        lambda x, w_, *a, **k: (calls['ragged'].append(w_.shape[0]), real_rg(x, w_, *a, **k))[1])
    monkeypatch.setattr(F, 'linear', lambda *a, **k: (_ for _ in ()).throw(AssertionError('library GEMM in the decoder')))
    monkeypatch.setattr(G, 'SKINNY_MAX_ROWS', 0)
    monkeypatch.setattr(G, 'FUSED_LN_MAX_ROWS', 0)
    dec = m.text_decoder.bfloat16()
    with torch.no_grad():
        got = dec(ids.to(DEV), encoder_hidden_states=enc.to(DEV).bfloat16()).logits
    assert got.dtype == BF
    scale = want.abs().max().item()
    err = (got.float().cpu() - want).abs().max().item()
    print(f'[decoder 320 teacher-forced] max|d logits| {err:.3e} (bound {0.04 * scale:.3e})')
    assert err < 0.04 * scale
    layers = d['layers']
    # per block (freq 1): self c_attn 960, c_proj 320, c_fc 1280, c_proj 320; cross q_attn 320, image k|v 640, c_proj 320,
    # c_fc 1280, c_proj 320; then the lm_head on the vocabulary padded to 512
    assert sorted(calls['tn']) == sorted([1280] * (2 * layers) + [512]), calls
    assert sorted(calls['ragged']) == sorted(([960] + [640] + [320] * 5) * layers), calls


def _xl_step_inputs(d, queries):
    g = torch.Generator().manual_seed(13)
    B, L = 2, 9
    ids = torch.randint(1, d['vocab'], (B, L), generator=g)
    labels = torch.randint(1, d['vocab'], (B, L), generator=g)
    labels[1, 6:] = 0
    return ids, labels, torch.randn(B, queries, 1600, generator=g)


def test_decoder_1600_training_step_runs_on_own_kernels():
    """GPT-2 XL's layout at 3 blocks (the layout of test_gpt2_xl_widths_decode): one step under forbid_library_gemm(), finite
    gradients everywhere, a second identical step gives equal bits. The oracle comparison is the 320-wide model's."""
    m, c, d, w = _mid_model('autocast', width=1600, heads=25, layers=3, vocab=331, freq=2)
    dec = m.text_decoder
    ids, labels, enc = _xl_step_inputs(d, c['queries'])
    loss, got, denc = _decoder_step(dec, ids, labels, enc)
    assert math.isfinite(loss)
    for k, p in dec.named_parameters():
        if p.requires_grad:
            assert got[k] is not None and torch.isfinite(got[k]).all(), k
    assert torch.isfinite(denc).all() and denc.abs().max() > 0
    got = {k: v.clone() for k, v in got.items() if v is not None}
    loss2, got2, denc2 = _decoder_step(dec, ids, labels, enc)
    assert loss2 == loss and torch.equal(denc, denc2)
    for k in got:
        assert torch.equal(got[k], got2[k]), k


def test_decoder_320_training_step_with_dropout(monkeypatch):
    """DECODER_DROPOUT on, pinned seed: the 320-wide step runs under the guard and repeats bit for bit"""
    from lavila_amd import gpt2_gated as G
    m, c, d, w = _mid_model('autocast', width=320, heads=5, layers=2, freq=1)
    dec = m.text_decoder
    monkeypatch.setattr(G, 'DECODER_DROPOUT', True)
    for k in ('resid_pdrop', 'embd_pdrop', 'attn_pdrop'):
        setattr(dec.config, k, 0.1)
    dec.train()
    assert dec.applies_dropout()
    ids, labels, enc = _decoder_inputs(d, c['text_width'], c['queries'])
    with G.fixed_dropout_seed(1234):
        loss, got, denc = _decoder_step(dec, ids, labels, enc)
        got = {k: v.clone() for k, v in got.items()}
        loss2, got2, denc2 = _decoder_step(dec, ids, labels, enc)
    dec.eval()
    loss_eval, _, _ = _decoder_step(dec, ids, labels, enc)
    assert math.isfinite(loss) and loss == loss2 and torch.equal(denc, denc2)
    assert loss_eval != loss                                         # the masks did drop something
    for k in got:
        assert torch.isfinite(got[k]).all() and torch.equal(got[k], got2[k]), k
