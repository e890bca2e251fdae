"""Bit-for-bit A/B of the fused residual chain between two trees (a refactor of the Python layer above the kernels).

    python tools/ab_chain_outputs.py run OUT.pt            every case of tests/chain_cases.py on THIS tree: output, loss, every
                                                           gradient and the bytes kept for backward (per distinct storage)
    python tools/ab_chain_outputs.py compare A.pt B.pt     torch.equal on every tensor, == on the byte counts; exit status 1
                                                           when anything differs

Run it twice on the parent (it must reproduce itself), once on the tree, and compare."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def run(path):
    import chain_cases
    res = {}
    for name in chain_cases.CASES:
        r = chain_cases.run(name, count_saved=True)
        res[name] = {'out': r['out'].cpu(), 'loss': None if r['loss'] is None else r['loss'].cpu(),
                     'grads': {k: g.cpu() for k, g in r['grads'].items()}, 'saved_bytes': r['saved_bytes']}
    torch.save(res, path)
    print(f'{len(res)} cases -> {path}')


def compare(path_a, path_b):
    a, b = torch.load(path_a), torch.load(path_b)
    bad = []
    if list(a) != list(b):
        bad.append(f'case lists differ: {sorted(set(a) ^ set(b))}')
    for name in a:
        if name not in b:
            continue
        x, y, diffs = a[name], b[name], []
        if not torch.equal(x['out'], y['out']):
            diffs.append('out')
        if (x['loss'] is None) != (y['loss'] is None) or (x['loss'] is not None and not torch.equal(x['loss'], y['loss'])):
            diffs.append('loss')
        if set(x['grads']) != set(y['grads']):
            diffs.append(f'gradient names {sorted(set(x["grads"]) ^ set(y["grads"]))}')
        diffs += [f'grad {k}' for k in x['grads'] if k in y['grads'] and not torch.equal(x['grads'][k], y['grads'][k])]
        if x['saved_bytes'] != y['saved_bytes']:
            diffs.append(f'saved bytes {x["saved_bytes"]} != {y["saved_bytes"]}')
        if diffs:
            bad.append(f'{name}: ' + ', '.join(diffs))
    tensors = sum(2 + len(v['grads']) for v in a.values())
    print(f'{path_a} vs {path_b}: {len(a)} cases, {tensors} tensors, {len(bad)} cases differ')
    for line in bad:
        print('  DIFFERS', line)
    return not bad


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == 'run':
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == 'compare':
        sys.exit(0 if compare(sys.argv[2], sys.argv[3]) else 1)
    else:
        sys.exit(__doc__)
