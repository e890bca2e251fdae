"""Times the max-margin ranking loss at the fine-tune's shape (B = 256 local rows of G = 2048, E = 256), float32 and bf16.

    python tools/probe_margin_loss.py                 device-event times of loss forward + backward, profiler off:
                                                      the kernels (lavila_amd.loss.MaxMarginRankingLoss on one slab, as one
                                                      of 8 ranks runs it) and the dense formulation (the whole G x G cosine
                                                      matrix and both hinge matrices through torch autograd, as every rank
                                                      of the reference computes them: tests/rank_loss_reference.dense_loss)
                                                      on the same device, alternated in one process, both warmed up
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/probe_margin_loss.py --kernels-only
                                                      the kernels alone, for per-kernel times
Needs an MI355X; prints what it measured, asserts nothing.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import rank_loss_reference as R  # noqa: E402
from lavila_amd import ops  # noqa: E402

B, G, E, ROW0, MARGIN = 256, 2048, 256, 512, 0.2


def kernels_step(img_all, txt_all, up):
    N = 2 * G * (G - 1)
    prep = ops.margin_loss_prepare_raw(img_all, txt_all, None, MARGIN)
    hinge, _ = ops.margin_loss_fwd_raw(img_all, txt_all, prep, B, ROW0, False)
    part = hinge.sum() / N
    dimg, dtxt = ops.margin_loss_bwd_raw(img_all, txt_all, prep, up, 8.0 / N, B, ROW0)
    return part, dimg, dtxt


def timed(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / reps      # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--reps', type=int, default=200)
    args = ap.parse_args()
    img, txt, _ = R.make_inputs(G, E, 100)
    up = torch.ones(1, device='cuda')
    for dt in (torch.float32, torch.bfloat16):
        i_all, t_all = img.to(dt).cuda(), txt.to(dt).cuda()
        li, lt = i_all.clone().requires_grad_(True), t_all.clone().requires_grad_(True)

        def new():
            return kernels_step(i_all, t_all, up)

        def old():
            li.grad = lt.grad = None
            R.dense_loss(li, lt, MARGIN, None, True).backward()

        for _ in range(10):
            new()
        torch.cuda.synchronize()
        if args.kernels_only:
            for _ in range(20):
                new()
            torch.cuda.synchronize()
            continue
        for _ in range(5):
            old()
        rounds = [(timed(new, args.reps), timed(old, max(args.reps // 10, 5))) for _ in range(5)]
        tn, to = sorted(r[0] for r in rounds), sorted(r[1] for r in rounds)
        part = new()[0].item()
        print(f'{str(dt):15s} B={B} G={G} E={E}: kernels (prepare + forward + backward, one of 8 slabs) '
              f'median {tn[2]:.1f} us (min {tn[0]:.1f}, max {tn[-1]:.1f}); dense torch formulation, whole '
              f'batch as every rank of the reference computes it, forward + backward median {to[2]:.1f} us (min {to[0]:.1f}, max {to[-1]:.1f}); '
              f'slab share of the loss {part:.6f}')


if __name__ == '__main__':
    main()
