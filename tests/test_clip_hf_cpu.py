"""CPU (-m "not gpu"): CLIP_HF and the DistilBERT tower at the drop-in boundary -- state-dict names / shapes and signatures
against the reference's (tests/golden/clip_hf_distilbert.pt), checkpoint round trips, every refusal before any device work,
load_pretrained_distilbert, and the float64 restatement (tests/distilbert_reference.py) pinned to the fixture."""
import contextlib
import inspect
import io
import warnings

import pytest
import torch

import clip_hf_helpers as H
import distilbert_reference as R


def test_state_dict_and_signatures_equal_the_references():
    from lavila.models import models
    fx = H.fixture()
    m = H.build_model(fx['config'])
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == fx['state_dict']
    assert [k for k, _ in m.named_parameters()] == fx['param_names']
    assert [k for k, _ in m.textual.named_buffers()] == fx['textual_buffers'] == ['embeddings.position_ids']
    for k, want in fx['signatures']['CLIP_HF'].items():
        assert str(inspect.signature(getattr(models.CLIP_HF, k))) == want, k
    for name in ('CLIP_OPENAI_TIMESFORMER_BASE_DISTILBERT_BASE', 'CLIP_OPENAI_TIMESFORMER_LARGE_DISTILBERT_BASE',
                 'CLIP_OPENAI_TIMESFORMER_LARGE_336PX_DISTILBERT_BASE'):
        assert str(inspect.signature(getattr(models, name))) == fx['signatures'][name], name
        assert models.get_metric_names(name) == ['loss', 'clip_loss', 'clip_acc']
    assert m.projection == 'default' and m.text_use_cls_token is True and m.text_is_regressive is False
    with pytest.raises(AttributeError):         # the reference's build_attention_mask reads a context_length it never sets
        m.build_attention_mask()


def test_initialisation_is_transformers():
    c = H.fixture()['config']
    torch.manual_seed(0)
    t = H.build_text(c)
    sd = t.state_dict()
    assert float(sd['embeddings.word_embeddings.weight'][0].abs().max()) == 0            # padding_idx row
    for k, v in sd.items():
        if k.endswith('LayerNorm.weight') or k.endswith('layer_norm.weight'):
            assert torch.equal(v, torch.ones_like(v)), k
        elif k.endswith('.bias'):
            assert not v.any(), k
        else:
            assert abs(float(v.std()) - 0.02) < 2e-3, (k, float(v.std()))
    assert t.embeddings.word_embeddings.padding_idx == 0


def test_round_trip_with_transformers():
    tf = pytest.importorskip('transformers')
    c = H.fixture()['config']
    hf = tf.DistilBertModel(tf.DistilBertConfig(
        vocab_size=c['vocab'], max_position_embeddings=c['positions'], dim=c['t_dim'], n_heads=c['t_heads'],
        n_layers=c['t_layers'], hidden_dim=c['t_hidden']))
    ours = H.build_text(c)
    assert list(ours.state_dict()) == list(hf.state_dict())
    print(ours.load_state_dict(hf.state_dict(), strict=True))
    for k, v in hf.state_dict().items():
        assert torch.equal(ours.state_dict()[k], v), k
    other = H.build_text(c)
    print(hf.load_state_dict(other.state_dict(), strict=True))
    assert torch.equal(hf.state_dict()['transformer.layer.1.ffn.lin2.weight'], other.transformer.layer[1].ffn.lin2.weight)


def test_position_ids_key_of_older_checkpoints_is_dropped():
    c = H.fixture()['config']
    src, dst = H.build_text(c), H.build_text(c)
    sd = dict(src.state_dict())
    sd['embeddings.position_ids'] = torch.arange(c['positions']).expand((1, -1))
    dst.load_state_dict(sd, strict=True)
    assert 'embeddings.position_ids' in sd, 'the caller\'s dict must stay as it was'
    assert torch.equal(dst.embeddings.LayerNorm.weight, src.embeddings.LayerNorm.weight)
    # ... and below `textual.` in a LaViLa checkpoint
    m = H.build_model(c)
    full = dict(H.weights())
    full['textual.embeddings.position_ids'] = sd['embeddings.position_ids']
    m.load_state_dict(full, strict=True)
    with pytest.raises(RuntimeError, match='Unexpected'):
        dst.load_state_dict({**sd, 'embeddings.other': torch.zeros(1)}, strict=True)


def test_refusals_come_before_any_device_work():
    from lavila.models import models
    from lavila_amd._cabi import HipExtensionError
    from lavila_amd.graph_step import GraphedTrainStep
    c = H.fixture()['config']
    with pytest.raises(NotImplementedError, match='head_dim 64'):
        H.build_text(c, n_heads=2)
    with pytest.raises(NotImplementedError, match='sinusoidal'):
        H.build_text(c, sinusoidal_pos_embds=True)
    with pytest.raises(NotImplementedError, match='gelu'):
        H.build_text(c, activation='relu')
    kw = dict(embed_dim=c['embed'], vision_width=c['dim'], vision_model=H.build_vision(c), text_width=c['t_dim'],
              text_model=H.build_text(c), text_use_cls_token=True, text_is_regressive=False)
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(NotImplementedError, match='frozen_in_time'):
            models.CLIP_HF(**kw, projection='frozen_in_time')
        with pytest.raises(NotImplementedError, match='pooler_output'):
            models.CLIP_HF(**{**kw, 'text_use_cls_token': False})
        with pytest.raises(NotImplementedError, match='regressive'):
            models.CLIP_HF(**{**kw, 'text_is_regressive': True})
        with pytest.raises(NotImplementedError, match='DistilBertModel'):
            models.CLIP_HF(**{**kw, 'text_model': torch.nn.Linear(4, 4)})
        with pytest.raises(KeyError):           # the reference pops text_use_cls_token without a default (models.py:532)
            models.CLIP_OPENAI_TIMESFORMER_BASE_DISTILBERT_BASE()
    t = H.build_text(c)
    ids = torch.zeros(2, 5, dtype=torch.long)
    for bad in (dict(head_mask=torch.ones(2)), dict(inputs_embeds=torch.zeros(2, 5, c['t_dim'])),
                dict(output_attentions=True), dict(output_hidden_states=True), dict(position_ids=ids),
                dict(return_dict=False)):
        with pytest.raises(NotImplementedError, match='CLIP_HF path'):
            t(ids, **bad)
    drop = H.build_text(c, dropout=0.1, attention_dropout=0.1)
    with pytest.raises(NotImplementedError, match='dropout / attention_dropout'):
        drop.train()(ids)
    with pytest.raises(HipExtensionError):      # eval mode passes the dropout check; there is no CPU path behind it
        drop.eval()(ids)
    with pytest.raises(ValueError, match='attention_mask'):
        t(ids, attention_mask=torch.ones(2, 4))
    t.gradient_checkpointing_enable()
    t.gradient_checkpointing_disable()
    m = H.build_model(c)
    with pytest.raises(ValueError, match='use_checkpoint'):
        m(torch.zeros(1), ids, use_checkpoint='everything')
    with pytest.raises(NotImplementedError, match='CLIP_HF'):
        GraphedTrainStep(m, None, None, (2, 3, 2, 32, 32), (2, 5), 'cuda')


def test_load_pretrained_distilbert(tmp_path, monkeypatch):
    from lavila.models import models
    c = H.fixture()['config']
    monkeypatch.delenv('LAVILA_DISTILBERT_WEIGHTS_DIR', raising=False)
    with pytest.warns(UserWarning, match='LAVILA_DISTILBERT_WEIGHTS_DIR'):
        assert models.load_pretrained_distilbert('distilbert-base-uncased') is None
    monkeypatch.setenv('LAVILA_DISTILBERT_WEIGHTS_DIR', str(tmp_path))
    with pytest.raises(RuntimeError, match='not found'):
        models.load_pretrained_distilbert('distilbert-base-uncased')
    src = H.build_text(c)
    torch.save(src.state_dict(), tmp_path / 'tiny.pt')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        sd = models.load_pretrained_distilbert('tiny')
    dst = H.build_text(c)
    dst.load_state_dict(sd, strict=True)
    assert all(torch.equal(a, b) for a, b in zip(src.state_dict().values(), dst.state_dict().values()))


def test_float64_restatement_reproduces_the_fixture():
    """tests/distilbert_reference.py against the unmodified reference's float32 results: the reference's own error is
    float32 round-off through a 2-layer tower (1e-5 on O(1) rows); 1e-4 / 1e-3 leaves the GPU tests' bars (1e-3 on
    activations, 1e-4 / 5e-3 on gradients) their meaning."""
    from oracle import oracle as O
    fx = H.fixture()
    c, A, Bp = fx['config'], fx['A'], fx['B']
    w = R.doubles(H.weights())
    out = R.clip_hf_forward(H.video().double(), fx['ids'], fx['mask_a'], w, c['heads'], c['t_heads'], norm_embed=True)
    lhs = R.tower(fx['ids'], fx['mask_a'], w, c['t_heads'], 'textual.')
    vis = fx['mask_a'].bool()
    torch.testing.assert_close(lhs[vis], A['last_hidden_state'].double()[vis], atol=1e-4, rtol=1e-4)
    for k in ('image_embed', 'text_embed', 'logit_scale'):
        torch.testing.assert_close(out[k], A[k].double(), atol=1e-5, rtol=1e-5, msg=lambda m, k=k: f'{k}: {m}')
    loss = O.clip_loss(out['image_embed'], out['text_embed'], out['logit_scale'])['loss']
    assert abs(loss.item() - A['loss'].item()) < 1e-5
    loss.backward()
    wg = w['textual.embeddings.word_embeddings.weight'].grad
    assert wg[0].any()                        # one visible token has the padding id: the plain gather differentiates it,
    wg[0] = 0                                 # nn.Embedding(padding_idx=0) does not
    n = H.check_selected({k: v.grad for k, v in w.items()}, A, 1e-6, 1e-3, 'A')
    assert n == len(fx['param_names'])
    pg = w['textual.embeddings.position_embeddings.weight'].grad
    assert not pg[int(fx['mask_a'].sum(1).max()):].any() and pg[:5].abs().min() > 0
    # mask set B, the text tower alone: holes, key 0 hidden, only the last key visible
    wb = R.doubles({k[len('textual.'):]: v for k, v in H.weights().items() if k.startswith('textual.')})
    lhs = R.tower(fx['ids'], fx['mask_b'], wb, c['t_heads'])
    visb = fx['mask_b'].bool()
    assert not visb[0, 0] and visb[1].sum() == 1 and visb[1, -1] and visb[2].all()
    torch.testing.assert_close(lhs[visb], Bp['last_hidden_state'].double()[visb], atol=1e-4, rtol=1e-4)
    (lhs * fx['upstream_b'].double() * fx['mask_b'].double()[..., None]).sum().backward()
    wb['embeddings.word_embeddings.weight'].grad[0] = 0           # nn.Embedding(padding_idx=0)
    H.check_selected({k: v.grad for k, v in wb.items()}, Bp, 1e-4, 1e-3, 'B')


def test_keymask_reference_properties():
    """The restatement's mask rule: hidden keys do not exist, a sample without visible keys is uniform."""
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(2, 5, 128, generator=g, dtype=torch.float64) for _ in range(3))
    mask = torch.tensor([[1, 0, 1, 1, 0], [0, 0, 0, 0, 0]])
    k2, v2 = k.clone(), v.clone()
    k2[0, [1, 4]] *= 2.0 ** 40
    v2[0, [1, 4]] *= -2.0 ** 40
    a, b = R.keymask_attention(q, k, v, mask, 2), R.keymask_attention(q, k2, v2, mask, 2)
    assert torch.equal(a[0], b[0])
    assert torch.allclose(a[1], v[1].mean(0, keepdim=True).expand(5, -1), atol=1e-14, rtol=0)
    assert torch.equal(R.keymask_attention(q, k, v, None, 2), R.keymask_attention(q, k, v, torch.ones(2, 5), 2))
