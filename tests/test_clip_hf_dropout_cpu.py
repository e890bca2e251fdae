"""CPU (-m "not gpu"): the text tower's dropout at the host boundary -- the restated mask contract
(tests/distilbert_dropout_reference.py) against the decoder's restatement and against itself on subset-of-rows calls, the
float64 restatement under dropout pinned to tests/golden/clip_hf_distilbert_dropout.pt (the unmodified reference under
injected masks) at the bars with which tests/test_clip_hf_cpu.py pins the undropped one, and the hygiene of the switch."""
import numpy as np
import pytest
import torch

import clip_hf_helpers as H
import distilbert_dropout_reference as DD
import distilbert_reference as R
import dropout_reference as DR
from conftest import load_golden


def _fx():
    return load_golden('clip_hf_distilbert_dropout.pt')


def _text_weights():
    return {k[len('textual.'):]: v for k, v in H.weights().items() if k.startswith('textual.')}


def test_fixture_belongs_to_the_undropped_one():
    fx, base = _fx(), H.fixture()
    assert fx['config'] == base['config'] and fx['weight_seed'] == base['weight_seed']
    assert fx['input_seed'] == base['input_seed']
    assert fx['sites'] == list(range(1 + 2 * fx['config']['t_layers']))
    assert fx['seed'] >> 32 and 0 <= fx['seed_index'] < 32
    assert int(base['mask_a'].sum(1).max()) == base['ids'].shape[1], 'the trim must change no index of (A)'
    for part in 'AB':                                        # the seed rule of the tool, from the reference's numbers alone
        for k, n in fx[part]['grad_norms'].items():
            assert n >= 0.1 * fx['plain_grad_norms'][part][k], (part, k)
    assert not torch.equal(fx['A']['text_embed'], base['A']['text_embed'])


def test_p0_restatement_is_the_undropped_tower_bit_for_bit():
    fx = H.fixture()
    w = R.doubles(_text_weights(), grad=False)
    for mask in (fx['mask_a'], fx['mask_b'], None):
        a = R.tower(fx['ids'], mask, w, fx['config']['t_heads'])
        b = DD.tower(fx['ids'], mask, w, fx['config']['t_heads'], 0x1234567890ABCDEF, 0.0, 0.0)
        assert torch.equal(a, b)


def test_float64_restatement_under_dropout_reproduces_the_fixture():
    """The bars of tests/test_clip_hf_cpu.py::test_float64_restatement_reproduces_the_fixture."""
    from oracle import oracle as O
    fx, base = _fx(), H.fixture()
    c, A, Bp = fx['config'], fx['A'], fx['B']
    seed, pd, pa = fx['seed'], fx['dropout']['dropout'], fx['dropout']['attention_dropout']
    w = R.doubles(H.weights())
    out = DD.clip_hf_forward(H.video().double(), base['ids'], base['mask_a'], w, c['heads'], c['t_heads'], seed, pd, pa,
                             norm_embed=True)
    lhs = DD.tower(base['ids'], base['mask_a'], w, c['t_heads'], seed, pd, pa, 'textual.')
    vis = base['mask_a'].bool()
    torch.testing.assert_close(lhs[vis], A['last_hidden_state'].double()[vis], atol=1e-4, rtol=1e-4)
    for k in ('image_embed', 'text_embed', 'logit_scale'):
        torch.testing.assert_close(out[k], A[k].double(), atol=1e-5, rtol=1e-5, msg=lambda m, k=k: f'{k}: {m}')
    loss = O.clip_loss(out['image_embed'], out['text_embed'], out['logit_scale'])['loss']
    assert abs(loss.item() - A['loss'].item()) < 1e-5
    loss.backward()
    w['textual.embeddings.word_embeddings.weight'].grad[0] = 0           # nn.Embedding(padding_idx=0)
    n = H.check_selected({k: v.grad for k, v in w.items()}, A, 1e-6, 1e-3, 'A')
    assert n == len(base['param_names'])
    wb = R.doubles(_text_weights())
    lhs = DD.tower(base['ids'], base['mask_b'], wb, c['t_heads'], seed, pd, pa)
    visb = base['mask_b'].bool()
    torch.testing.assert_close(lhs[visb], Bp['last_hidden_state'].double()[visb], atol=1e-4, rtol=1e-4)
    (lhs * base['upstream_b'].double() * base['mask_b'].double()[..., None]).sum().backward()
    wb['embeddings.word_embeddings.weight'].grad[0] = 0
    H.check_selected({k: v.grad for k, v in wb.items()}, Bp, 1e-4, 1e-3, 'B')


@pytest.mark.parametrize('p', [0.1, 0.5])
def test_attention_index_with_s8_is_the_decoders(p):
    seed = 0xC0FFEE1234567
    for B, Hh, L, Tk in ((2, 3, 5, 5), (1, 2, 7, 256), (3, 1, 1, 1)):
        assert DD.attn_shift(Tk) == 8
        assert np.array_equal(DD.attn_keep(seed, 3, B, Hh, L, Tk, p), DR.attn_mask(seed, 3, B, Hh, L, Tk, p))
    assert np.array_equal(DD.row_keep(seed, 4, 6, 40, p), DR.row_mask(seed, 4, 6, 40, p))
    k = DD.attn_keep(seed, 3, 4, 4, 64, 64, 0.5)
    assert 0.45 < k.mean() < 0.55


def test_shift_beyond_256_keys():
    assert [DD.attn_shift(t) for t in (1, 255, 256, 257, 300, 512, 513)] == [8, 8, 8, 9, 9, 9, 10]
    seed, site, p = 77, 5, 0.5
    for Tk in (257, 512):
        B, Hh, L = 2, 2, 3
        k = DD.attn_keep(seed, site, B, Hh, L, Tk, p)
        flat = DR.keep_mask(seed, site, 0, B * Hh * L * 512, p).reshape(B, Hh, L, 512)[..., :Tk]
        assert np.array_equal(k, flat)
        # ... and it is NOT the s = 8 map continued: key 256 of a row is not key 0 of the next
        assert not np.array_equal(k[..., 0, 256:], k[..., 1, :Tk - 256])


def test_subset_of_rows_calls_address_the_full_calls_elements():
    seed, p = 0xABCDEF0123456789, 0.5
    B, Hh, L, D = 3, 2, 7, 64
    for Tk in (7, 300):
        full = DD.attn_keep(seed, 1, B, Hh, L, Tk, p)
        row0 = DD.attn_keep(seed, 1, B, Hh, 1, Tk, p, idx_qrep=L)
        assert np.array_equal(row0, full[:, :, :1])
        five = DD.attn_keep(seed, 1, B, Hh, 5, Tk, p, idx_qrep=L)
        assert np.array_equal(five, full[:, :, :5])
        assert not np.array_equal(DD.attn_keep(seed, 1, B, Hh, 1, Tk, p), full[:, :, :1])      # idx_qrep matters
    rows = DD.row_keep(seed, 2, B * L, D, p).reshape(B, L, D)
    assert np.array_equal(DD.row_keep(seed, 2, B, D, p, row_index_stride=L * D), rows[:, 0])
    assert not np.array_equal(DD.row_keep(seed, 2, B, D, p), rows[:, 0])


def test_config_under_the_switch_is_transformers(monkeypatch):
    tf = pytest.importorskip('transformers')
    from lavila_amd import distilbert
    monkeypatch.setattr(distilbert, 'TEXT_DROPOUT', True)
    on, hf = distilbert.distilbert_config(), tf.DistilBertConfig()
    assert on.dropout == hf.dropout and on.attention_dropout == hf.attention_dropout
    assert distilbert._HF_DROPOUT == {'dropout': hf.dropout, 'attention_dropout': hf.attention_dropout}


def test_switch_hygiene(monkeypatch):
    from lavila_amd import distilbert
    from lavila_amd._cabi import HipExtensionError
    c = H.fixture()['config']
    ids = torch.zeros(2, 5, dtype=torch.long)
    monkeypatch.delenv('LAVILA_TEXT_DROPOUT', raising=False)
    assert distilbert.TEXT_DROPOUT is None and not distilbert.text_dropout_enabled()
    off = distilbert.distilbert_config()
    assert off.dropout == 0.0 and off.attention_dropout == 0.0
    t = H.build_text(c, dropout=0.1, attention_dropout=0.1)
    with pytest.raises(NotImplementedError, match='the DistilBERT tower has no dropout: config.dropout / attention_dropout '
                                                  'must be 0.0 to train'):
        t.train()(ids)
    # on: read per call, from the module attribute or the environment
    monkeypatch.setenv('LAVILA_TEXT_DROPOUT', '1')
    assert distilbert.text_dropout_enabled()
    monkeypatch.setattr(distilbert, 'TEXT_DROPOUT', False)
    assert not distilbert.text_dropout_enabled()
    monkeypatch.delenv('LAVILA_TEXT_DROPOUT')
    monkeypatch.setattr(distilbert, 'TEXT_DROPOUT', True)
    on = distilbert.distilbert_config()
    assert on.dropout == 0.1 and on.attention_dropout == 0.1
    assert H.build_text(c).config.dropout == 0.1
    with pytest.raises(HipExtensionError):          # the training forward is let through; there is no CPU path behind it
        t.train()(ids)
    monkeypatch.setattr(distilbert, 'TEXT_DROPOUT', None)
    with pytest.raises(NotImplementedError, match='has no dropout'):
        t.train()(ids)
