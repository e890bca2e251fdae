"""Times one narrator training step (main_pretrain.py --model VCLM_OPENAI_TIMESFORMER_BASE_GPT2: TSF-B/16 x 4 frames, the
256-query pooler, gated-cross-attention GPT-2 of 12 blocks, CaptionLoss, AdamW, bf16 autocast, `.train()`) with and without
the decoder's dropout: local batch 32, captions of 77 tokens, random weights and inputs. HIP events around the timed steps
after `--warmup` untimed ones and around every single step for the spread; peak memory of the timed window.

`--pdrop zero` runs with resid / embd / attn_pdrop = 0 (the plan without dropout; the file also runs from a checkout that has
no dropout switch yet, to time the tree before this feature on the same machine), `--pdrop ref` with the switch on and the
probabilities gpt2_config() then holds (transformers' 0.1). `--kernels` times the four kernel kinds alone at the step's shapes
(2464 rows of 768; 32 captions x 12 heads, 77 positions, 256 image tokens), each beside its form without dropout on the same
operands.

    python tools/probe_narrator_dropout_step.py --pdrop ref [--steps 8 --warmup 3 --kernels --out profiles/decoder_dropout_step.txt]
"""
import argparse
import contextlib
import io
import os
import sys
import types
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VOCAB, PAD = 50257, 50256


def build(frames, drop):
    from lavila.models import models
    from lavila_amd import gpt2_gated as G
    has_switch = hasattr(G, 'decoder_dropout_enabled')
    if drop and not has_switch:
        raise SystemExit('this checkout has no decoder dropout: --pdrop ref needs the switch')
    if has_switch:
        G.DECODER_DROPOUT = bool(drop)
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        torch.manual_seed(0)
        model = models.VCLM_OPENAI_TIMESFORMER_BASE_GPT2(gated_xattn=True, random_init_gpt2=True, num_frames=frames)
    with torch.no_grad():           # zeros-initialised time attention and gates would make their branches no-ops
        for blk in model.visual.blocks:
            blk.timeattn.qkv.weight.normal_(0, 0.02)
            blk.timeattn.proj.weight.normal_(0, 0.02)
        for blk in model.text_decoder.transformer.h:
            blk.alpha_cattn.fill_(0.5)
            blk.alpha_dense.fill_(0.5)
    cfg = model.text_decoder.config
    return model.cuda().train(), (cfg.resid_pdrop, cfg.embd_pdrop, cfg.attn_pdrop), has_switch


def run(model, batch, frames, length, steps, warmup):
    from lavila.models.loss import CaptionLoss
    crit = CaptionLoss(tokenizer=types.SimpleNamespace(pad_token_id=PAD))
    opt = torch.optim.AdamW(model.parameters(), lr=1e-5)
    g = torch.Generator().manual_seed(1)
    video = torch.randn(batch, 3, frames, 224, 224, generator=g).cuda()
    text = torch.randint(0, VOCAB - 1, (batch, length), generator=g).cuda()

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            loss = crit(model(video, text))['loss']
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


def time_kernels(batch=32, length=77, heads=12, keys=256, p=0.1, reps=50):
    """us per call (output allocation included) of each kernel kind with and without dropout on the same operands."""
    from lavila_amd import gpt2_gated as G
    from lavila_amd import ops
    D, rows, seed = heads * 64, batch * length, 0x1234567890ABCDEF
    g = torch.Generator(device='cuda').manual_seed(3)
    bf = lambda *s: torch.randn(*s, generator=g, device='cuda').bfloat16()
    res, y, dh, dadd, q, do = (bf(rows, D) for _ in range(6))
    kv, qkv = bf(batch, keys, 2 * D), bf(rows, 3 * D)
    gamma, beta = (torch.randn(D, generator=g, device='cuda') for _ in range(2))
    alpha = torch.tensor(0.5, device='cuda')
    for t in (res, y, q, kv, qkv):
        t.requires_grad_(True)
    cases = []

    def pair(name, make, ins, grads):
        """The forward call, and the backward of one such call on a retained graph."""
        outs = make()
        outs = outs if isinstance(outs, tuple) else (outs,)
        cases.append((f'{name} forward', make))
        cases.append((f'{name} backward', lambda: torch.autograd.grad(outs, ins, grads, retain_graph=True)))

    pair('gated add + LayerNorm, without dropout', lambda: G._GatedAddLnFn.apply(res, y, alpha, gamma, beta, 1e-5),
         (res, y), (dadd, dh))
    pair(f'gated add + LayerNorm, p = {p}', lambda: G._GatedAddLnFn.apply(res, y, alpha, gamma, beta, 1e-5, (seed, 8, p)),
         (res, y), (dadd, dh))
    pair(f'cross-attention ({length} x {keys}), without dropout', lambda: G._RowsAttnFn.apply(q, kv, length, heads),
         (q, kv), (do,))
    pair(f'cross-attention ({length} x {keys}), p = {p}', lambda: G._RowsAttnFn.apply(q, kv, length, heads, (seed, 7, p)),
         (q, kv), (do,))
    pair(f'causal self-attention (L = {length}), without dropout: ops.causal_attention',
         lambda: ops.causal_attention(qkv.reshape(batch, length, 3 * D), heads).reshape(rows, D), (qkv,), (do,))
    pair(f'causal self-attention (L = {length}), p = {p}: rows kernel, causal',
         lambda: G._RowsAttnFn.apply(qkv, None, length, heads, (seed, 4, p)), (qkv,), (do,))
    x = res.detach()
    cases.append((f'lvl_dropout_apply (embedding site), p = {p}', lambda: G._DropoutFn._apply(x, (seed, 0, p))))
    out = []
    for name, fn in cases:
        for _ in range(5):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(f'  {name}: {1e3 * a.elapsed_time(b) / reps:.1f} us per call')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=4)
    ap.add_argument('--length', type=int, default=77)
    ap.add_argument('--pdrop', choices=['zero', 'ref'], default='zero')
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--tag', default='')
    ap.add_argument('--out', default=None, help='append the result lines to this file')
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.steps > 0:
        model, pdrop, has_switch = build(args.frames, args.pdrop == 'ref')
        ms, per, peak, loss = run(model, args.batch, args.frames, args.length, args.steps, args.warmup)
        say(f'{args.tag}narrator training step, VCLM_OPENAI_TIMESFORMER_BASE_GPT2 (gated) x {args.frames} frames, '
            f'{args.batch} captions of {args.length} tokens, bf16 autocast, resid / embd / attn_pdrop {pdrop}'
            f'{"" if has_switch else " (no dropout switch in this checkout)"}: {ms:.1f} ms per step '
            f'({1e3 * args.batch / ms:.1f} clips/s), per-step events {[round(x, 1) for x in per]}, peak memory {peak:.1f} GiB, '
            f'loss {loss:.4f}')
    if args.kernels:
        say(f'{args.tag}kernels alone at the step\'s shapes (autograd Function call, output allocation included):')
        for line in time_kernels(args.batch, args.length):
            say(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
