"""What text dropout costs: one bf16 training step of the CLIP_OPENAI_TIMESFORMER_BASE_DISTILBERT_BASE geometry (4 frames,
224 x 224) with distilbert.TEXT_DROPOUT off and on, alternating, and the times of the two kinds of call that change -- the
key-masked attention pair (forward + backward) and the FFN site (lin2 + residual + LayerNorm, forward + backward) -- with
and without dropout at the tower's shapes. Random weights, synthetic clips; captions of 12-32 tokens in 77 positions (the
batch is trimmed to its longest caption). Forward under bf16 autocast, CLIPLoss, backward, AdamW step.

Every measurement runs in a fresh child process under its own time limit; the parent never opens the device.

    python tools/probe_clip_hf_dropout_step.py [--batch 32] [--out profiles/clip_hf_dropout_step.txt]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tools')]
NAME = 'CLIP_OPENAI_TIMESFORMER_BASE_DISTILBERT_BASE'


def _median_ms(fn, warmup, steps):
    import torch
    times = []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def child_step(on, B, steps, warmup):
    import torch
    from lavila.models.loss import CLIPLoss
    from lavila_amd import distilbert
    import probe_clip_hf_step as P
    distilbert.TEXT_DROPOUT = bool(on)
    g = torch.Generator().manual_seed(1)
    model = P.build(NAME).cuda().train()
    assert model.textual.config.dropout == (0.1 if on else 0.0)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-5)
    crit = CLIPLoss(use_vissl=False, cache_labels=True, rank=0, world_size=1)
    video = torch.randn(B, 3, 4, 224, 224, generator=g).cuda()
    lens = torch.randint(12, 33, (B,), generator=g)
    pos = torch.arange(77)[None]
    ids = (torch.randint(1000, 30000, (B, 77), generator=g) * (pos < lens[:, None])).cuda()
    mask = (pos < lens[:, None]).float().cuda()
    state = {}

    def step():
        with torch.autocast('cuda', dtype=torch.bfloat16):
            state['loss'] = crit(model(video, ids, mask=mask, norm_embed=True))['loss']
        state['loss'].backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
    ms = _median_ms(step, warmup, steps)
    assert torch.isfinite(state['loss'])
    print(f'RESULT step dropout={"on" if on else "off"} batch {B}: {ms:.2f} ms / step ({B / ms * 1e3:.1f} pairs/s), longest '
          f'caption {int(lens.max())}')


def child_kernels(B, steps, warmup):
    import torch
    from lavila_amd import ops
    g = torch.Generator().manual_seed(2)
    L, H, D, HID = 32, 12, 768, 3072
    bf = torch.bfloat16
    q, k, v = (torch.randn(B, L, D, generator=g).to(bf).cuda().requires_grad_(True) for _ in range(3))
    do = torch.randn(B, L, D, generator=g).to(bf).cuda()
    lens = torch.randint(12, 33, (B,), generator=g)
    mask = (torch.arange(L)[None] < lens[:, None]).to(torch.uint8).cuda()
    a = torch.randn(B, L, HID, generator=g).to(bf).cuda().requires_grad_(True)
    h = torch.randn(B, L, D, generator=g).to(bf).cuda().requires_grad_(True)
    w = (torch.randn(D, HID, generator=g) * HID ** -0.5).cuda().requires_grad_(True)
    b, gamma, beta = (torch.randn(D, generator=g).cuda().requires_grad_(True) for _ in range(3))
    seed = 0x5EEDC0DE0B5E55ED

    def attn(p):
        def run():
            o = ops.keymask_attention(q, k, v, mask, H, (L, seed, 1, p) if p else None)
            o.backward(do)
        return run

    def ffn(p):
        def run():
            with torch.autocast('cuda', dtype=bf):
                if p:
                    o = ops.dropout_add_layer_norm(h, ops.linear(a, w, b), gamma, beta, 1e-12, D, seed, 2, p)
                else:
                    fused = ops.linear_residual_layer_norm(a, w, b, h, gamma, beta, 1e-12)
                    o = fused[1] if fused is not None else ops.add_layer_norm(h, ops.linear(a, w), b, gamma, beta, 1e-12,
                                                                              keep_sum=False)[1]
            o.backward(do)
        return run
    for name, make in (('key-masked attention fwd+bwd', attn), ('FFN site (lin2 + add + LayerNorm) fwd+bwd', ffn)):
        for p in (0.0, 0.1, 0.0, 0.1):
            ms = _median_ms(make(p), warmup, steps)
            print(f'RESULT {name} [B {B}, L {L}, D {D}] p={p}: {ms * 1e3:.1f} us (host-timed, launch overhead included)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--limit', type=int, default=240, help='seconds per child process')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', default=None)
    args = ap.parse_args()
    if args.child in ('off', 'on'):
        return child_step(args.child == 'on', args.batch, args.steps, args.warmup)
    if args.child == 'kernels':
        return child_kernels(args.batch, 20, 5)
    lines = [f'{NAME} geometry, 4 frames x 224 x 224, bf16 autocast, forward + CLIPLoss + backward + AdamW; median of '
             f'{args.steps} steps after {args.warmup}; switch alternated off / on, one fresh process each']
    for mode in ('off', 'on', 'off', 'on', 'kernels'):
        cmd = [sys.executable, os.path.abspath(__file__), '--child', mode, '--batch', str(args.batch), '--steps',
               str(args.steps), '--warmup', str(args.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        got = [ln[len('RESULT '):] for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
        if r.returncode != 0 or not got:
            lines.append(f'{mode}: FAILED with exit status {r.returncode}: {r.stderr.strip()[-400:]}')
            break                                            # nothing more on the device after a failure
        lines += got
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
