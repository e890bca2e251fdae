"""CPU (-m "not gpu"): the narrator's criterion (lavila_amd/loss.py: CaptionLoss) without its kernels -- the float64
restatement the GPU tests measure against is pinned to the reference's own outputs (tests/golden/caption_loss.pt,
tools/gen_caption_loss_golden.py), the drop-in boundary, and the host logic (layouts, label views, the gradient view) with
the kernel hooks replaced by the restatement."""
import inspect
import math
from types import SimpleNamespace

import pytest
import torch

from conftest import load_golden
import caption_loss_reference as R


def _close(got, want, rel):
    if math.isnan(want):
        return math.isnan(got)
    return abs(got - want) <= rel * abs(want)


def _case_input(case):
    """The golden's logits in the layout the reference was run on."""
    logits = case['logits']                                             # stored contiguous [B,V,T]
    if case['layout'] == 'permuted':
        logits = logits.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    return logits, case['labels'], case['pad']


@pytest.mark.parametrize('name', list(R.CASES))
def test_restatement_matches_reference(name):
    fx = load_golden('caption_loss.pt')
    case = fx['cases'][name]
    made = R.make_case(name)
    assert torch.equal(made[0], case['logits']) and torch.equal(made[1], case['labels']) and made[2] == case['pad']
    assert made[0].is_contiguous() == (case['layout'] == 'contiguous')
    res, grad = R.loss_and_grad(case['logits'], case['labels'], case['pad'])
    for k, key in enumerate(('loss', 'acc', 'ppl')):
        assert _close(res[k].item(), case[key], 1e-6), (key, res[k].item(), case[key])
    torch.testing.assert_close(grad.float(), case['grad'], rtol=1e-4, atol=1e-8)
    assert case['grad'].abs().max() > 1e-4


def test_golden_covers_what_it_should():
    fx = load_golden('caption_loss.pt')
    cases = fx['cases']
    assert math.isnan(cases['ragged_pad0']['ppl']) and not math.isnan(cases['ragged_pad0']['loss'])     # all-pad caption
    assert any(c['pad'] != 0 for c in cases.values())
    assert {c['layout'] for c in cases.values()} == {'permuted', 'contiguous'}
    assert all(c['logits'].shape[1] % 2 == 1 for c in cases.values())                                   # odd V
    assert all(0 < c['acc'] < 100 for c in cases.values())
    for v in fx['narrator'].values():
        assert v['stored']['acc'] == 0 and 0 < v['hit']['acc'] < 100 and v['gap'] > 2 * 0.0168


@pytest.mark.parametrize('variant', ['freq1_gated', 'freq2_plain'])
def test_restatement_matches_reference_on_narrator_logits(variant):
    fx = load_golden('caption_loss.pt')['narrator'][variant]
    v = load_golden('narrator_decoder.pt')['variants'][variant]
    top2 = v['logits'].topk(2, dim=1).values
    assert abs((top2[:, 0] - top2[:, 1]).min().item() - fx['gap']) < 1e-6
    for tag, labels in (('stored', v['labels']), ('hit', fx['labels_hit'])):
        res, _ = R.loss_and_grad(v['logits'], labels, fx['pad'])
        for k, key in enumerate(('loss', 'acc', 'ppl')):
            assert _close(res[k].item(), fx[tag][key], 1e-6), (tag, key, res[k].item(), fx[tag][key])


def test_drop_in_boundary():
    import lavila.models.loss
    import lavila_amd.loss
    from lavila_amd._cabi import HipExtensionError
    fx = load_golden('caption_loss.pt')
    cls = lavila.models.loss.CaptionLoss
    assert cls is lavila_amd.loss.CaptionLoss
    assert str(inspect.signature(cls.__init__)) == fx['signatures']['init']
    assert str(inspect.signature(cls.forward)) == fx['signatures']['forward']
    tok = SimpleNamespace(pad_token_id=7)
    crit = cls(tokenizer=tok)
    assert crit.pad_id == 7 and crit.tokenizer is tok and crit.state_dict() == {}
    assert cls(pad_id=3, tokenizer=SimpleNamespace(pad_token_id=0)).pad_id == 0       # the tokenizer wins, as in the reference
    with pytest.raises(AttributeError):                                               # ... and is required, as there
        cls()
    with pytest.raises(HipExtensionError):                                            # no CPU fallback
        crit({'text_tokens_logits': torch.randn(2, 9, 3), 'labels': torch.zeros(2, 3, dtype=torch.long)})


def _restated(pad):
    from lavila.models.loss import CaptionLoss

    class Restated(R.Hooks, CaptionLoss):                   # kernel hooks -> CPU restatement (test-only)
        pass

    return Restated(tokenizer=SimpleNamespace(pad_token_id=pad))


@pytest.mark.parametrize('name', list(R.CASES))
def test_module_host_logic_matches_reference(name):
    """Layout handling, the label copy, the reduce and the gradient view, kernels replaced by the restatement."""
    fx = load_golden('caption_loss.pt')
    case = fx['cases'][name]
    logits, labels, pad = _case_input(case)
    leaf = logits.detach().clone().requires_grad_(True)
    assert leaf.stride() == logits.stride()
    crit = _restated(pad)
    out = crit({'text_tokens_logits': leaf, 'labels': labels})
    assert list(out) == fx['output_keys'] and out['loss'] is out['caption_loss']
    for key, gkey in (('loss', 'loss'), ('caption_acc', 'acc'), ('ppl', 'ppl')):
        assert out[key].dim() == 0 and out[key].dtype == torch.float32
        assert _close(out[key].item(), case[gkey], 1e-6), (key, out[key].item(), case[gkey])
    assert out['loss'].requires_grad and not out['caption_acc'].requires_grad and not out['ppl'].requires_grad
    seen = type(crit).seen
    B, V, T = logits.shape
    assert tuple(seen.shape) == (B * T, V) and seen.stride(1) == 1
    if case['layout'] == 'permuted':                         # read in place: the hook saw the caller's memory
        assert seen.data_ptr() == leaf.data_ptr() and seen.stride(0) == V
    else:                                                    # one copy into padded rows
        assert seen.data_ptr() != leaf.data_ptr() and seen.stride(0) == R.padded(V)
    out['loss'].backward()
    assert leaf.grad.shape == leaf.shape and leaf.grad.dtype == torch.float32
    torch.testing.assert_close(leaf.grad, case['grad'], rtol=1e-4, atol=1e-8)


def test_module_takes_label_views_upstream_factors_and_other_dtypes():
    fx = load_golden('caption_loss.pt')
    case = fx['cases']['ragged_pad0']
    logits, labels, pad = _case_input(case)
    B, V, T = logits.shape
    text = torch.cat([torch.full((B, 1), 5), labels], dim=1)              # labels = text[:, 1:], as VCLM_HF.forward
    view = text[:, 1:]
    assert not view.is_contiguous()
    crit = _restated(pad)
    leaf = logits.detach().clone().requires_grad_(True)
    out = crit({'text_tokens_logits': leaf, 'labels': view})
    (2.5 * out['loss']).backward()
    assert _close(out['loss'].item(), case['loss'], 1e-6)
    torch.testing.assert_close(leaf.grad, 2.5 * case['grad'], rtol=1e-4, atol=1e-8)
    # a padded product seen through [:, :V] (pack.logits()): read in place, the row stride is the padded one
    wide = torch.full((B, T, R.padded(V)), float('nan'))
    wide[:, :, :V] = logits.permute(0, 2, 1)
    out = crit({'text_tokens_logits': wide[:, :, :V].permute(0, 2, 1), 'labels': labels})
    assert type(crit).seen.data_ptr() == wide.data_ptr() and type(crit).seen.stride(0) == R.padded(V)
    assert _close(out['loss'].item(), case['loss'], 1e-6)
    # float16: computed in float32, the gradient comes back as float16; bf16 stays bf16
    for dt, kept in ((torch.float16, torch.float32), (torch.bfloat16, torch.bfloat16)):
        leaf = logits.detach().to(dt).clone().requires_grad_(True)
        out = crit({'text_tokens_logits': leaf, 'labels': labels})
        assert type(crit).seen.dtype == kept and out['loss'].dtype == torch.float32
        out['loss'].backward()
        assert leaf.grad.dtype == dt and leaf.grad.shape == leaf.shape
        want, gwant = R.loss_and_grad(leaf.detach(), labels, pad)
        assert _close(out['loss'].item(), want[0].item(), 1e-6)
        # one rounding to the caller's dtype: 2^-8 relative (bf16), float16's subnormal spacing 2^-24 absolute
        torch.testing.assert_close(leaf.grad.double(), gwant, rtol=2.0 ** -8, atol=2.0 ** -24)
    with pytest.raises(ValueError, match='labels'):
        crit({'text_tokens_logits': logits, 'labels': labels[:, :-1]})


def test_out_of_range_label_is_nan_not_an_address():
    logits, labels, pad = R.make_case('no_pad')
    labels = labels.clone()
    labels[0, 1] = logits.shape[1]
    labels[1, 2] = -5
    res, grad = R.loss_and_grad(logits, labels, pad)
    assert math.isnan(res[0].item())
    assert grad[0, :, 1].isnan().all() and grad[1, :, 2].isnan().all() and grad[0, :, 0].isfinite().all()
    # a pad id outside [0, V) is compared first: such labels are pads, not errors
    labels[0, 1], labels[1, 2] = -100, -100
    res, grad = R.loss_and_grad(logits, labels, -100)
    assert torch.isfinite(res).all() and (grad[0, :, 1] == 0).all()
