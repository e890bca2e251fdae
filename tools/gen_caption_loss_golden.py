"""Writes tests/golden/caption_loss.pt from the UNMODIFIED reference CaptionLoss (lavila/models/loss.py:220-253,
imported through oracle.ref_import.load_reference()) with a SimpleNamespace(pad_token_id=...) tokenizer. Data only:

  signatures, output_keys     constructor / forward signatures and the keys of the output dict;
  cases[name]                 the synthetic float32 cases of tests/caption_loss_reference.CASES (ragged pad tails, an
                              all-pad caption, a pad id that is not 0, permuted-view and contiguous layouts): logits,
                              labels, pad, layout and the reference's loss, acc, ppl and full logits gradient;
  narrator[variant]           the reference criterion on the logits / labels stored in tests/golden/narrator_decoder.pt,
                              once with the stored labels ('stored') and once with the labels at even positions replaced
                              by the reference's own argmax ('hit', so that caption_acc is not zero), and the smallest
                              top-2 gap of those logits.

    python tools/gen_caption_loss_golden.py        (needs the reference tree; see oracle/ref_import.py)
"""
import inspect
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from oracle.ref_import import load_reference  # noqa: E402
import caption_loss_reference as R  # noqa: E402


def run_reference(ref, logits, labels, pad, want_grad=True):
    crit = ref.loss.CaptionLoss(tokenizer=SimpleNamespace(pad_token_id=pad))
    assert crit.pad_id == pad and crit.state_dict() == {}
    leaf = logits.detach().clone().requires_grad_(want_grad)          # keeps the layout (clone preserves strides)
    assert leaf.stride() == logits.stride()
    out = crit({'text_tokens_logits': leaf, 'labels': labels})
    keys = list(out)
    res = {'loss': out['loss'].item(), 'acc': float(out['caption_acc']), 'ppl': float(out['ppl'])}
    if want_grad:
        out['loss'].backward()
        res['grad'] = leaf.grad.detach().contiguous().clone()         # [B,V,T]
    return res, keys


def main():
    ref = load_reference()
    cls = ref.loss.CaptionLoss
    fx = {'signatures': {'init': str(inspect.signature(cls.__init__)), 'forward': str(inspect.signature(cls.forward))},
          'cases': {}, 'narrator': {}}
    for name, spec in R.CASES.items():
        logits, labels, pad = R.make_case(name)
        res, keys = run_reference(ref, logits, labels, pad)
        fx['output_keys'] = keys
        fx['cases'][name] = dict(res, logits=logits.contiguous().clone(), labels=labels.clone(), pad=pad, layout=spec[4])
        print(f'[golden] {name}: loss={res["loss"]:.6f} acc={res["acc"]:.3f} ppl={res["ppl"]:.4f}')
    nd = torch.load(os.path.join(ROOT, 'tests', 'golden', 'narrator_decoder.pt'), weights_only=False)
    for vname, v in nd['variants'].items():
        logits, labels, pad = v['logits'], v['labels'], v['pad']
        top2 = logits.topk(2, dim=1).values
        hit = labels.clone()
        hit[:, 0::2] = logits.argmax(dim=1)[:, 0::2]
        entry = {'pad': pad, 'gap': (top2[:, 0] - top2[:, 1]).min().item(), 'labels_hit': hit,
                 'max_abs_logit': logits.abs().max().item()}
        for tag, lab in (('stored', labels), ('hit', hit)):
            entry[tag], _ = run_reference(ref, logits, lab, pad, want_grad=False)
            print(f'[golden] {vname} {tag}: {entry[tag]}')
        print(f'[golden] {vname}: smallest top-2 gap {entry["gap"]:.4f}')
        fx['narrator'][vname] = entry
    path = os.path.join(ROOT, 'tests', 'golden', 'caption_loss.pt')
    torch.save(fx, path)
    print(f'[golden] -> {path} ({os.path.getsize(path)} bytes)')


if __name__ == '__main__':
    main()
