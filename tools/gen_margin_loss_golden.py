"""Writes tests/golden/max_margin_loss.pt from the UNMODIFIED reference (lavila/models/loss.py:256-367, imported through
oracle.ref_import.load_reference()): loss and gradients of MaxMarginRankingLoss and AdaptiveMaxMarginRankingLoss, both
fix_norm settings, in a single process and on 2 and 3 gloo ranks (every rank's loss and local gradients, so the W x
gradient convention of GatherLayer is on record), plus the constructor / forward signatures. Data only.

The inputs are tests/rank_loss_reference.make_inputs in float32. The seed is the first for which every hinge argument
of every case keeps |c_i + x| >= GAP in float64: no term of the fixture can be decided differently by float32-class
arithmetic, so the fixture pins active sets as well as values.

    python tools/gen_margin_loss_golden.py        (needs the reference tree; see oracle/ref_import.py)
"""
import inspect
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from oracle.ref_import import load_reference  # noqa: E402
import rank_loss_reference as R  # noqa: E402

E = 64
SINGLE_G = 16
B_LOCAL = 4
WORLDS = (2, 3)
GAP = 1e-4
CLASSES = (('MaxMarginRankingLoss', 0.2), ('AdaptiveMaxMarginRankingLoss', 0.4))
PORT = 29841


def cases():
    for name, margin in CLASSES:
        for fix_norm in (True, False):
            yield name, margin, fix_norm


def smallest_gap(seed):
    gap = float('inf')
    for G in (SINGLE_G,) + tuple(w * B_LOCAL for w in WORLDS):
        img, txt, w = (t.float() for t in R.make_inputs(G, E, seed))
        for name, margin in CLASSES:
            weight = w if name.startswith('Adaptive') else None
            for z in R.hinge_arguments(img, txt, margin, weight):
                gap = min(gap, z[~z.isnan()].abs().min().item())
            if weight is not None:
                gap = min(gap, (margin * weight.double()).abs().min().item())      # the diagonal terms of fix_norm=False
    return gap


def run_reference(ref, name, margin, fix_norm, li, lt, lw):
    crit = getattr(ref.loss, name)(margin=margin, fix_norm=fix_norm)
    li, lt = li.clone().requires_grad_(True), lt.clone().requires_grad_(True)
    out = crit({'image_embed': li, 'text_embed': lt}, lw)
    assert sorted(out) == ['loss', 'max_margin_loss']
    out['loss'].backward()
    return out['loss'].item(), li.grad, lt.grad


def _rank_worker(rank, world, port, seed, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    ref = load_reference()
    img, txt, w = (t.float() for t in R.make_inputs(world * B_LOCAL, E, seed))
    sl = slice(rank * B_LOCAL, (rank + 1) * B_LOCAL)
    res = {}
    for name, margin, fix_norm in cases():
        loss, di, dt = run_reference(ref, name, margin, fix_norm, img[sl], txt[sl], w[sl].clone())
        res[(name, fix_norm)] = (loss, di.tolist(), dt.tolist())
    q.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


def main():
    import torch.multiprocessing as mp
    ref = load_reference()
    seed = next(s for s in range(1000) if smallest_gap(s) >= GAP)
    fx = {'E': E, 'seed': seed, 'gap': smallest_gap(seed), 'required_gap': GAP, 'single_G': SINGLE_G, 'B_local': B_LOCAL,
          'worlds': WORLDS, 'margins': dict(CLASSES), 'single': {}, 'multi': {}, 'signatures': {}}
    for name, _ in CLASSES:
        cls = getattr(ref.loss, name)
        fx['signatures'][name] = {'init': str(inspect.signature(cls.__init__)), 'forward': str(inspect.signature(cls.forward))}
    fx['signatures']['sim_matrix'] = str(inspect.signature(ref.loss.sim_matrix))
    fx['output_keys'] = ['loss', 'max_margin_loss']
    img, txt, w = (t.float() for t in R.make_inputs(SINGLE_G, E, seed))
    for name, margin, fix_norm in cases():
        loss, di, dt = run_reference(ref, name, margin, fix_norm, img, txt, w.clone())
        fx['single'][(name, fix_norm)] = {'loss': loss, 'dimg': di, 'dtxt': dt}
        print(f'[golden] {name} fix_norm={fix_norm}: loss={loss:.6f}')
    ctx = mp.get_context('spawn')
    for k, world in enumerate(WORLDS):
        q = ctx.Queue()
        procs = [ctx.Process(target=_rank_worker, args=(r, world, PORT + k, seed, q)) for r in range(world)]
        for p in procs:
            p.start()
        got = sorted([q.get(timeout=600) for _ in range(world)], key=lambda t: t[0])
        for p in procs:
            p.join()
        for name, _, fix_norm in cases():
            fx['multi'][(world, name, fix_norm)] = {
                'loss': [g[1][(name, fix_norm)][0] for g in got],
                'dimg': torch.cat([torch.tensor(g[1][(name, fix_norm)][1]) for g in got]),
                'dtxt': torch.cat([torch.tensor(g[1][(name, fix_norm)][2]) for g in got])}
        print(f'[golden] {world} ranks done')
    path = os.path.join(ROOT, 'tests', 'golden', 'max_margin_loss.pt')
    torch.save(fx, path)
    print(f'[golden] seed {seed}, smallest |hinge argument| {fx["gap"]:.3e} -> {path} ({os.path.getsize(path)} bytes)')


if __name__ == '__main__':
    main()
