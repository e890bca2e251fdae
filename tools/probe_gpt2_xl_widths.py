"""Times the GEMMs of a GPT-2 XL narrator decoder (width 1600 = 25 heads of 64) on this package against the library calls
they replace, and one training step of an XL-layout decoder.

  --gemms   the seven shapes -- c_attn, attention c_proj, q_attn, cross c_attn, c_fc, MLP c_proj and the lm_head's input
            gradient at the padded vocabulary -- at M = 2464 and 9856 rows (32 and 128 captions x 77 tokens): forward, input
            gradient and weight gradient, own path (ops.linear_tn_rows / ops._wgrad) against F.linear / dy @ w.t() / x.t() @ dy,
            ALTERNATING in rounds inside this process (median of the rounds). For a ragged width the main launch is also timed
            alone (lvl_linear_tn on W[:N0]); the two launches of lvl_linear_tn_ragged run back to back on one stream, so the
            difference is the edge kernel's time.
  --step    forward + CaptionLoss + backward of a decoder with width 1600, 25 heads, 4 blocks, cross-attention in every second
            block, gated, the real vocabulary (50257), 32 captions x 77 tokens against 256 image tokens, bf16 autocast; with
            --freeze-lm the `--freeze-lm-vclm` recipe (only the cross-attention side trains). `--root DIR` imports the package
            from another checkout (A/B against an older commit: run the two alternately, one process each).

    python tools/probe_gpt2_xl_widths.py --gemms --step --out profiles/gpt2_xl_widths.txt
"""
import argparse
import os
import statistics
import sys
import types

import torch
import torch.nn.functional as F

BF = torch.bfloat16
D = 1600
VOCAB_PAD = 50432
SHAPES = (('c_attn', 3 * D, D), ('attn c_proj', D, D), ('q_attn', D, D), ('cross c_attn', 2 * D, D), ('c_fc', 4 * D, D),
          ('mlp c_proj', D, 4 * D))


def _time(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return 1e3 * s.elapsed_time(e) / reps


def alternate(fns, reps=20, rounds=5):
    """fns: name -> callable. Every round times each of them in turn; returns name -> median microseconds per call."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            got[k].append(_time(fn, reps))
    return {k: statistics.median(v) for k, v in got.items()}


def gemms(rows_list, say):
    from lavila_amd import ops
    g = torch.Generator().manual_seed(0)

    def rnd(*shape, scale=1.0):
        return (scale * torch.randn(*shape, generator=g)).to('cuda').to(BF)

    def fmt(t, key='own'):
        extra = ''
        if 'main' in t:
            extra = f' (main launch alone {t["main"]:.1f}, edge kernel {t[key] - t["main"]:.1f})'
        return f'own {t[key]:8.1f} us{extra}, library {t["lib"]:8.1f} us, own / library {t[key] / t["lib"]:.2f}'

    def tn_pair(x, w, bias, lib):
        """own (lvl_linear_tn or lvl_linear_tn_ragged) against `lib`; + the main launch alone where the width is ragged"""
        fns = {'own': lambda: ops.linear_tn_rows(x, w, bias), 'lib': lib}
        n0 = w.shape[0] // 256 * 256
        if 0 < n0 < w.shape[0]:
            w0, b0 = w[:n0].contiguous(), None if bias is None else bias[:n0].contiguous()
            fns['main'] = lambda: ops.linear_tn_raw(x, w0, b0)
        return alternate(fns)

    for M in rows_list:
        say(f'--- M = {M} rows ---')
        for name, n_out, n_in in SHAPES:
            x, dy = rnd(M, n_in), rnd(M, n_out)
            w_out_in = rnd(n_out, n_in, scale=n_in ** -0.5)
            w_in_out = w_out_in.t().contiguous()
            bias = torch.randn(n_out, generator=g).cuda()
            bias_bf = bias.to(BF)
            t = tn_pair(x, w_out_in, bias, lambda: F.linear(x, w_out_in, bias_bf))
            say(f'{name:13s} [{n_in}->{n_out}] forward        : {fmt(t)}')
            t = tn_pair(dy, w_in_out, None, lambda: dy @ w_in_out.t())
            say(f'{name:13s} [{n_in}->{n_out}] input gradient : {fmt(t)}')
            t = alternate({'own': lambda: ops._wgrad(x, dy, torch.float32), 'lib': lambda: (x.t() @ dy).float()})
            say(f'{name:13s} [{n_in}->{n_out}] weight gradient: {fmt(t)}')
            del x, dy, w_out_in, w_in_out
        dl = rnd(M, VOCAB_PAD)
        w = rnd(VOCAB_PAD, D, scale=D ** -0.5)
        wt = w.t().contiguous()
        t = tn_pair(dl, wt, None, lambda: dl @ w)
        say(f'lm_head       [{D}->{VOCAB_PAD}] input gradient : {fmt(t)}')
        del dl, w, wt
        torch.cuda.empty_cache()


def step(freeze_lm, steps, warmup, say, tag):
    from lavila.models.loss import CaptionLoss
    from lavila_amd.gpt2_gated import GPT2LMHeadModel, augment_gpt2_config, gpt2_config
    torch.manual_seed(0)
    base = gpt2_config('gpt2', vocab_size=50257, n_positions=1024, n_embd=D, n_layer=4, n_head=25)
    dec = GPT2LMHeadModel(augment_gpt2_config(base, cross_attn_freq=2, gated_xattn=True)).cuda().eval()
    with torch.no_grad():                        # open gates: tanh(0) = 0 would hide the gated branches
        for blk in dec.transformer.h:
            if hasattr(blk, 'alpha_cattn'):
                blk.alpha_cattn.fill_(0.5)
                blk.alpha_dense.fill_(0.5)
    if freeze_lm:
        dec.freeze_lm_weights()
    g = torch.Generator().manual_seed(1)
    B, L, NQ = 32, 77, 256
    ids = torch.randint(1, 50257, (B, L), generator=g).cuda()
    labels = torch.randint(1, 50257, (B, L), generator=g).cuda()
    labels[:, 60:] = 0
    enc = torch.randn(B, NQ, D, generator=g).cuda().requires_grad_(True)
    crit = CaptionLoss(tokenizer=types.SimpleNamespace(pad_token_id=0))

    def one():
        dec.zero_grad(set_to_none=True)
        enc.grad = None
        with torch.autocast('cuda', dtype=BF):
            logits = dec(ids, encoder_hidden_states=enc).logits
            out = crit({'text_tokens_logits': logits.permute(0, 2, 1), 'labels': labels})
        out['loss'].backward()
        return out['loss']

    for _ in range(warmup):
        one()
    torch.cuda.synchronize()
    per = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        loss = one()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b))
    say(f'[{tag}] XL-layout decoder step (width 1600, 25 heads, 4 blocks, cross-attention every 2nd, vocabulary 50257, '
        f'{B} x {L} tokens, {NQ} image tokens, bf16 autocast, {"frozen LM" if freeze_lm else "everything trains"}): '
        f'median {statistics.median(per):.2f} ms, min {min(per):.2f}, max {max(per):.2f} over {steps} steps, loss {loss.item():.4f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gemms', action='store_true')
    ap.add_argument('--step', action='store_true')
    ap.add_argument('--freeze-lm', action='store_true')
    ap.add_argument('--rows', type=int, nargs='+', default=[2464, 9856])
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--tag', default='this tree')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import warnings
    warnings.simplefilter('ignore')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.gemms:
        gemms(args.rows, say)
    if args.step:
        step(args.freeze_lm, args.steps, args.warmup, say, args.tag)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
