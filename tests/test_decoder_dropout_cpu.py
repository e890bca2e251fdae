"""CPU: the host side of the decoder's opt-in dropout -- the numpy restatement of the mask (tests/dropout_reference.py) against
Philox4x32-10's known answers, the threshold formula, the keep rate, the switch semantics of gpt2_config() against the
installed transformers, and the golden of tools/gen_narrator_dropout_golden.py (the unmodified reference in `.train()` under
the restated masks)."""
import math

import numpy as np
import pytest

import dropout_reference as R
from conftest import load_golden


def test_restatement_reproduces_known_answers():
    for ctr, key, want in R.KNOWN_ANSWERS:
        out = R.philox4x32_10([np.array([x], dtype=np.uint64) for x in ctr], key)
        assert tuple(int(o[0]) for o in out) == want, (ctr, key)
    # vectorised over counters: the same answers side by side
    ctr = [np.array([k[0][i] for k in R.KNOWN_ANSWERS[:1] * 2], dtype=np.uint64) for i in range(4)]
    out = R.philox4x32_10(ctr, R.KNOWN_ANSWERS[0][1])
    assert all(int(o[0]) == int(o[1]) == w for o, w in zip(out, R.KNOWN_ANSWERS[0][2]))


def test_threshold_formula():
    assert R.threshold(0.0) == 0 and R.scale(0.0) == np.float32(1.0)
    # float32(0.1) = 13421773 * 2^-27: p * 2^32 = 429496736 exactly
    assert R.threshold(0.1) == 13421773 * 32 == 429496736
    assert R.threshold(0.5) == 1 << 31 and R.scale(0.5) == np.float32(2.0)
    below_one = np.nextafter(np.float32(1.0), np.float32(0.0))          # 1 - 2^-24
    assert R.threshold(below_one) == (1 << 32) - 256 <= (1 << 32) - 1
    assert R.scale(0.1) == np.float32(1.0) / (np.float32(1.0) - np.float32(0.1))
    assert R.keep_mask(1, 0, 0, 4096, 0.0).all()                        # p = 0 keeps everything


def test_keep_rate_within_five_sigma():
    n, p = 1 << 20, 0.1
    kept = int(R.keep_mask(0x1234567890ABCDEF, 4, 0, n, p).sum())
    q = 1.0 - float(np.float32(p))
    sigma = math.sqrt(n * q * (1.0 - q))
    print(f'[keep rate] kept {kept} of {n}: {kept / n:.5f} (expected {q:.5f}, {abs(kept - n * q) / sigma:.2f} sigma)')
    assert abs(kept - n * q) <= 5.0 * sigma


def test_sites_seeds_and_offsets_give_different_masks():
    a = R.keep_mask(7, 0, 0, 4096, 0.5)
    assert not np.array_equal(a, R.keep_mask(7, 1, 0, 4096, 0.5))                   # another site
    assert not np.array_equal(a, R.keep_mask(8, 0, 0, 4096, 0.5))                   # another low seed word
    assert not np.array_equal(a, R.keep_mask(7 | (1 << 32), 0, 0, 4096, 0.5))       # another high seed word
    assert not np.array_equal(a, R.keep_mask(7, 0, 1 << 34, 4096, 0.5))             # the high counter word
    # a range is a window of the one element stream, whatever its alignment
    assert np.array_equal(a[5:133], R.keep_mask(7, 0, 5, 128, 0.5))
    big = (1 << 34) - 8
    assert np.array_equal(R.keep_mask(7, 3, big, 16, 0.5)[8:], R.keep_mask(7, 3, 1 << 34, 8, 0.5))
    # the layouts are reshapes of that stream
    assert np.array_equal(R.row_mask(7, 2, 3, 16, 0.5).reshape(-1), R.keep_mask(7, 2, 0, 48, 0.5))
    m = R.attn_mask(7, 1, 2, 3, 5, 37, 0.5)
    assert m.shape == (2, 3, 5, 37)
    e = (((1 * 3 + 2) * 5 + 4) << 8) | 36
    assert m[1, 2, 4, 36] == R.keep_mask(7, 1, e, 1, 0.5)[0]


def test_gpt2_config_switch_follows_transformers(monkeypatch):
    from transformers import GPT2Config
    from lavila_amd import gpt2_gated as G
    hf = GPT2Config()
    names = ('resid_pdrop', 'embd_pdrop', 'attn_pdrop')
    monkeypatch.setattr(G, 'DECODER_DROPOUT', None)
    monkeypatch.delenv('LAVILA_DECODER_DROPOUT', raising=False)
    assert not G.decoder_dropout_enabled()
    assert all(getattr(G.gpt2_config('gpt2'), k) == 0.0 for k in names)
    monkeypatch.setenv('LAVILA_DECODER_DROPOUT', '1')                    # read per call, not at import
    assert G.decoder_dropout_enabled()
    cfg = G.gpt2_config('gpt2-xl')
    assert all(getattr(cfg, k) == getattr(hf, k) and getattr(hf, k) > 0 for k in names)
    monkeypatch.delenv('LAVILA_DECODER_DROPOUT')
    assert all(getattr(G.gpt2_config('gpt2'), k) == 0.0 for k in names)
    monkeypatch.setattr(G, 'DECODER_DROPOUT', True)
    cfg = G.gpt2_config('gpt2', attn_pdrop=0.25)                          # overrides still win
    assert cfg.attn_pdrop == 0.25 and cfg.resid_pdrop == hf.resid_pdrop and cfg.embd_pdrop == hf.embd_pdrop
    aug = G.augment_gpt2_config(cfg)
    assert aug.attn_pdrop == 0.25 and aug.resid_pdrop == hf.resid_pdrop
    monkeypatch.setenv('LAVILA_DECODER_DROPOUT', '1')
    monkeypatch.setattr(G, 'DECODER_DROPOUT', False)                     # the attribute, when set, decides
    assert G.gpt2_config('gpt2').resid_pdrop == 0.0


def test_switch_lifts_the_refusal_and_reports_applies_dropout(monkeypatch):
    """Switch on: the refusal of a non-zero probability is gone (the forward then needs a device, which it says);
    applies_dropout() follows switch, mode and probabilities; fixed_dropout_seed pins and restores the seed."""
    import torch
    from lavila_amd import gpt2_gated as G
    from lavila_amd._cabi import HipExtensionError
    monkeypatch.setattr(G, 'DECODER_DROPOUT', True)
    cfg = G.augment_gpt2_config(G.gpt2_config('gpt2', vocab_size=50, n_positions=16, n_embd=64, n_layer=1, n_head=1))
    dec = G.GPT2LMHeadModel(cfg).bfloat16().train()
    assert dec.applies_dropout()
    with pytest.raises(HipExtensionError):                                # past the refusal: no device on this machine
        dec(torch.ones(1, 4, dtype=torch.long))
    dec.config.resid_pdrop = 1.0
    with pytest.raises(ValueError, match='resid_pdrop'):
        dec(torch.ones(1, 4, dtype=torch.long))
    dec.config.resid_pdrop = 0.1
    assert not dec.eval().applies_dropout()
    dec.train()
    monkeypatch.setattr(G, 'DECODER_DROPOUT', False)
    assert not dec.applies_dropout()
    with pytest.raises(NotImplementedError, match='LAVILA_DECODER_DROPOUT'):
        dec(torch.ones(1, 4, dtype=torch.long))
    monkeypatch.setattr(G, 'DECODER_DROPOUT', True)
    for k in ('resid_pdrop', 'embd_pdrop', 'attn_pdrop'):
        setattr(dec.config, k, 0.0)
    assert not dec.applies_dropout()
    with G.fixed_dropout_seed(0xFEDCBA9876543210):
        assert G._draw_seed() == 0xFEDCBA9876543210
        with G.fixed_dropout_seed(5):
            assert G._draw_seed() == 5
        assert G._draw_seed() == 0xFEDCBA9876543210
    torch.manual_seed(11)
    a, b = G._draw_seed(), G._draw_seed()
    torch.manual_seed(11)
    assert a != b and G._draw_seed() == a and 0 <= a < 1 << 64


def test_golden_probabilities_and_site_census():
    from transformers import GPT2Config
    g = load_golden('narrator_dropout.pt')
    fx = load_golden('narrator_decoder.pt')
    hf = GPT2Config()
    assert g['format'] == 2 and g['seed'] >> 32 != 0
    assert g['pdrop'] == {k: float(getattr(hf, k)) for k in ('resid_pdrop', 'embd_pdrop', 'attn_pdrop')}
    layers = fx['decoder']['layers']
    for name, v in g['variants'].items():
        freq = fx['variants'][name]['variant']['cross_attn_freq']
        want = [0]
        for i in range(layers):
            want += [R.site_of(i, k) for k in ((0, 1, 2, 3, 4, 5) if i % freq == 0 else (3, 4, 5))]
        assert v['sites'] == sorted(want), name
        assert len(set(v['sites'])) == len(v['sites'])
        assert set(v['grads']) | set(v['grad_slices']) == set(v['grad_norms'])


@pytest.mark.parametrize('variant', ['freq1_gated', 'freq2_plain'])
def test_golden_loss_differs_from_the_eval_step(variant):
    drop = load_golden('narrator_dropout.pt')['variants'][variant]
    plain = load_golden('narrator_train.pt')['variants'][variant]
    assert math.isfinite(drop['loss']) and abs(drop['loss'] - plain['loss']) > 1e-2
    assert set(drop['grad_norms']) == set(plain['grad_norms'])
    # the seed rule of tools/gen_narrator_dropout_golden.py: no gradient (a gate's is ONE number) cancels under the masks
    weak = [k for k, n in drop['grad_norms'].items() if n < 0.1 * plain['grad_norms'][k]]
    assert not weak, weak
