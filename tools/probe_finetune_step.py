"""Times one step of the classification fine-tune (main_finetune_classification.py, EK-100): forward, three label-smoothed
cross-entropies, backward, AdamW, under bf16 autocast, on `CLIP_OPENAI_TIMESFORMER_BASE(num_frames=16, drop_path_rate=0.1)
.visual` below `VideoClassifierMultiHead` with 97 / 300 / 3806 classes: local batch 16, 16 x 224^2 clips (3137 tokens each),
random weights and inputs. HIP events around the timed steps after `--warmup` untimed ones, and around every single step for the
spread; peak memory of the timed window.

The file also runs from a checkout that has no classifier class yet (to time the tree before this probe existed on the same
machine): the heads are then the plain stand-in below. `--kernels` times lvl_droppath_add_layernorm_fwd / _bwd alone at the
step's shape (50192 rows of 768) beside lvl_layernorm_fwd / _bwd with the same operands.

    python tools/probe_finetune_step.py [--steps 8 --warmup 3 --kernels --out profiles/finetune_classification_step.txt]
    rocprofv3 --kernel-trace --stats -d DIR -o ft -- python tools/probe_finetune_step.py --steps 2 --warmup 2
    python tools/kernel_stats.py DIR/.../ft_results.db 4
"""
import argparse
import contextlib
import io
import os
import sys
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES = (97, 300, 3806)


class _StandInHeads(nn.Module):
    """What a driver would write without the package's class: three nn.Linear heads on the tower's features."""

    def __init__(self, vision_model, dropout, num_classes_list):
        super().__init__()
        self.visual = vision_model
        self.dropout = nn.Dropout(dropout)
        self.fc_cls = nn.ModuleList([nn.Linear(vision_model.num_features, n) for n in num_classes_list])

    def forward(self, image, use_checkpoint=False):
        e = self.visual(image, use_checkpoint=use_checkpoint)
        return [m(self.dropout(e)) for m in self.fc_cls]


def build(frames, drop_path_rate):
    from lavila.models import models
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        torch.manual_seed(0)
        vis = models.CLIP_OPENAI_TIMESFORMER_BASE(num_frames=frames, drop_path_rate=drop_path_rate).visual
    with torch.no_grad():           # the constructor's zeros-initialised time attention would make its branch a no-op
        for blk in vis.blocks:
            blk.timeattn.qkv.weight.normal_(0, 0.02)
            blk.timeattn.proj.weight.normal_(0, 0.02)
    cls = getattr(models, 'VideoClassifierMultiHead', None)
    own = cls is not None
    model = (cls or _StandInHeads)(vis, dropout=0.0, num_classes_list=list(CLASSES))
    return model.cuda().train(), own


def run(model, batch, frames, steps, warmup, use_checkpoint):
    opt = torch.optim.AdamW(model.parameters(), lr=1e-5)
    g = torch.Generator().manual_seed(1)
    video = torch.randn(batch, 3, frames, 224, 224, generator=g).cuda()
    targets = [torch.randint(0, n, (batch,), generator=g).cuda() for n in CLASSES]

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            logits = model(video, use_checkpoint=use_checkpoint)
            loss = sum(F.cross_entropy(lg.float(), t, label_smoothing=0.1) for lg, t in zip(logits, targets))
        loss.backward()
        opt.step()
        return loss

    torch.manual_seed(2)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for i in range(steps):
        loss = step()
        ev[i + 1].record()
    torch.cuda.synchronize()
    per = [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]
    return ev[0].elapsed_time(ev[-1]) / steps, per, torch.cuda.max_memory_allocated() / 2 ** 30, loss.item()


def time_kernels(rows_per_sample=3137, samples=16, cols=768, reps=20):
    """us per call and GB/s of algorithmic bytes (E = 2): the scaled pair against the plain pair on the same operands."""
    from lavila_amd import ops
    if not hasattr(ops, 'droppath_add_layernorm_fwd_raw'):
        return []
    rows = rows_per_sample * samples
    g = torch.Generator(device='cuda').manual_seed(3)
    res, y, dh, dadd = (torch.randn(rows, cols, generator=g, device='cuda').bfloat16() for _ in range(4))
    yb, gamma, beta = (torch.randn(cols, generator=g, device='cuda') for _ in range(3))
    scale = (torch.rand(samples, generator=g, device='cuda') < 0.9).float() / 0.9
    h, s, mean, rstd = ops.droppath_add_layernorm_fwd_raw(res, y, yb, scale, rows_per_sample, gamma, beta, 1e-6)
    E = 2 * rows * cols
    cases = [
        ('lvl_droppath_add_layernorm_fwd (2 in, 2 out)', 4 * E,
         lambda: ops.droppath_add_layernorm_fwd_raw(res, y, yb, scale, rows_per_sample, gamma, beta, 1e-6)),
        ('lvl_layernorm_fwd add keep_sum (2 in, 2 out)', 4 * E, lambda: ops.layernorm_fwd_raw(res, y, yb, gamma, beta, 1e-6, True)),
        ('lvl_layernorm_fwd add (2 in, 1 out)', 3 * E, lambda: ops.layernorm_fwd_raw(res, y, yb, gamma, beta, 1e-6, False)),
        ('lvl_droppath_add_layernorm_bwd dadd + dysum (fused form: 3 in, 2 out)', 5 * E,
         lambda: ops.droppath_add_layernorm_bwd_raw(dh, s, gamma, mean, rstd, scale, dadd, rows_per_sample, True)),
        ('lvl_layernorm_bwd dadd + dxsum (3 in, 1 out)', 4 * E,
         lambda: ops.layernorm_bwd_raw(dh, s, None, None, gamma, mean, rstd, dadd, True)),
    ]
    out = []
    for name, nbytes, fn in cases:
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        us = 1e3 * a.elapsed_time(b) / reps
        out.append(f'  {name}: {us:.1f} us per call (output allocation included), {nbytes / us / 1e3:.0f} GB/s of algorithmic bytes')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--drop-path-rate', type=float, default=0.1)
    ap.add_argument('--use-checkpoint', action='store_true')
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--tag', default='')
    ap.add_argument('--out', default=None, help='append the result lines to this file')
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    model, own = build(args.frames, args.drop_path_rate)
    ms, per, peak, loss = run(model, args.batch, args.frames, args.steps, args.warmup, args.use_checkpoint)
    heads = 'VideoClassifierMultiHead' if own else 'stand-in nn.Linear heads'
    say(f'{args.tag}classification fine-tune step, TSF-B/16 x {args.frames} frames, drop_path_rate {args.drop_path_rate:g}, '
        f'{heads} {CLASSES}, bf16 autocast, local batch {args.batch}'
        f'{", block checkpointing" if args.use_checkpoint else ""}: {ms:.1f} ms per step ({1e3 * args.batch / ms:.1f} clips/s), '
        f'per-step events {[round(x, 1) for x in per]}, peak memory {peak:.1f} GiB, loss {loss:.4f}')
    if args.kernels:
        for line in time_kernels():
            say(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
