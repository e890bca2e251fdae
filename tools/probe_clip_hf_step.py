"""One bf16 training step of CLIP_OPENAI_TIMESFORMER_LARGE_336PX_DISTILBERT_BASE (4 frames) at the largest local batch of
`--batches` that fits, and beside it the same video tower with CLIP_OPENAI_TIMESFORMER_LARGE_336PX's own text tower at that
batch: milliseconds per step (median of `--steps` after `--warmup`) and peak device memory. Random weights, synthetic
clips; captions of 12-32 tokens in 77 positions. Forward under bf16 autocast, CLIPLoss, backward, AdamW step.

    python tools/probe_clip_hf_step.py [--batches 96,64,48,32] [--out profiles/clip_hf_distilbert_step.txt]
"""
import argparse
import contextlib
import io
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def build(name):
    from lavila.models import models
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        torch.manual_seed(0)
        return getattr(models, name)(num_frames=4, text_use_cls_token=False, project_embed_dim=256)


def batch(B, hf, seed=1):
    g = torch.Generator().manual_seed(seed)
    video = torch.randn(B, 3, 4, 336, 336, generator=g)
    lens = torch.randint(12, 33, (B,), generator=g)
    pos = torch.arange(77)[None]
    if hf:          # DistilBERT: [CLS] ... [SEP] then padding id 0, and the tokenizer's float32 mask
        ids = torch.randint(1000, 30000, (B, 77), generator=g) * (pos < lens[:, None])
        return video, ids, (pos < lens[:, None]).float()
    ids = torch.randint(1, 49406, (B, 77), generator=g) * (pos < lens[:, None])
    ids[torch.arange(B), lens - 1] = 49407
    return video, ids, None


def run(name, B, steps, warmup):
    from lavila.models.loss import CLIPLoss
    hf = 'DISTILBERT' in name
    model = build(name).cuda().train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-5)
    crit = CLIPLoss(use_vissl=False, cache_labels=True, rank=0, world_size=1)
    video, ids, mask = (t.cuda() if t is not None else None for t in batch(B, hf))
    torch.cuda.reset_peak_memory_stats()
    times = []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        with torch.autocast('cuda', dtype=torch.bfloat16):
            out = model(video, ids, mask=mask, norm_embed=True) if hf else model(video, ids, norm_embed=True)
            loss = crit(out)['loss']
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    assert torch.isfinite(loss)
    n_text = sum(p.numel() for k, p in model.named_parameters() if k.startswith(('textual.', 'transformer.', 'token_emb')))
    return sorted(times)[len(times) // 2], torch.cuda.max_memory_allocated() / 2 ** 30, n_text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='96,64,48,32')
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = [f'device: {torch.cuda.get_device_name(0)}; 4 frames x 336 x 336, bf16 autocast, forward + CLIPLoss + backward + '
             f'AdamW; median of {args.steps} steps after {args.warmup}']
    fit = None
    for B in (int(b) for b in args.batches.split(',')):
        try:
            ms, gib, n = run('CLIP_OPENAI_TIMESFORMER_LARGE_336PX_DISTILBERT_BASE', B, args.steps, args.warmup)
        except torch.OutOfMemoryError:
            lines.append(f'CLIP_OPENAI_TIMESFORMER_LARGE_336PX_DISTILBERT_BASE  batch {B}: out of memory')
            torch.cuda.empty_cache()
            continue
        lines.append(f'CLIP_OPENAI_TIMESFORMER_LARGE_336PX_DISTILBERT_BASE  batch {B}: {ms:.1f} ms / step '
                     f'({B / ms * 1e3:.1f} pairs/s), peak {gib:.1f} GiB, text tower {n / 1e6:.1f} M parameters')
        fit = B
        break
    if fit is not None:
        torch.cuda.empty_cache()
        ms, gib, n = run('CLIP_OPENAI_TIMESFORMER_LARGE_336PX', fit, args.steps, args.warmup)
        lines.append(f'CLIP_OPENAI_TIMESFORMER_LARGE_336PX (CLIP text tower)  batch {fit}: {ms:.1f} ms / step '
                     f'({fit / ms * 1e3:.1f} pairs/s), peak {gib:.1f} GiB, text tower {n / 1e6:.1f} M parameters')
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
