"""Times one training step of the narrator on this package: VCLM_OPENAI_TIMESFORMER_BASE_GPT2(gated_xattn=True,
freeze_lm_vclm=True, freeze_visual_vclm=True) -- the reference's `main_pretrain.py --model VCLM_OPENAI_TIMESFORMER_BASE_GPT2
--gated-xattn --freeze-lm-vclm --freeze-visual-vclm` recipe -- forward + CaptionLoss + backward + AdamW, 4 frames of 224^2,
77 tokens, bf16 autocast, random weights and inputs. HIP events around the timed steps after `--warmup` untimed ones, as
bench.py does; a pair of events around every `--event-stride`-th step gives the per-step spread. The local batch is the first
of `--batches` that fits (an out-of-memory step moves on to the next). Also times lvl_cross_attn_rows_fwd / _bwd alone at
(64 contexts, qrep 76, 12 heads, Tk 256).

`--caption-lengths standin` gives caption b `6 + (11 b) % 19` tokens (BOS / EOS included, 6..24: a stand-in for Ego4D's short
narrations; there is no dataset here) followed by pad id 0, instead of 60 tokens each; `--pack-captions` switches
narrator.PACK_CAPTIONS on (off: the environment's LAVILA_PACK_CAPTIONS decides). The kept share R / (B L) of the decoder rows is
printed either way, and lvl_rows_pack / lvl_rows_unpack are timed alone at the probe's shape (--row-kernels).

    python tools/probe_narrator_train.py [--steps 10 --warmup 3 --out profiles/narrator_train.txt]
    python tools/probe_narrator_train.py --batches 128 --caption-lengths standin --pack-captions --row-kernels
    rocprofv3 --kernel-trace --stats -d DIR -o nt -- python tools/probe_narrator_train.py --steps 3 --warmup 1 \
        --batches 128 --no-kernels;  python tools/kernel_stats.py DIR/.../nt_results.db 4
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


def build():
    from lavila.models import models
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        torch.manual_seed(0)
        m = models.VCLM_OPENAI_TIMESFORMER_BASE_GPT2(gated_xattn=True, random_init_gpt2=True, freeze_lm_vclm=True,
                                                     freeze_visual_vclm=True, num_frames=4)
    with torch.no_grad():                        # open gates: the tanh(0) = 0 of a fresh model would hide the gated branches
        for blk in m.text_decoder.transformer.h:
            blk.alpha_cattn.fill_(0.5)
            blk.alpha_dense.fill_(0.5)
    return m.cuda().eval()                       # eval(): drop_path off; nothing in this model draws random numbers then


def captions(batch, lengths, g):
    """[batch, 77] token ids: `lengths` = 'full' -> 60 tokens per caption (the record of profiles/narrator_train.txt),
    'standin' -> 6 + (11 b) % 19 tokens for caption b; pad id 0 behind."""
    text = torch.randint(1, 50257, (batch, 77), generator=g)
    tokens = torch.full((batch,), 60) if lengths == 'full' else 6 + (11 * torch.arange(batch)) % 19
    text[torch.arange(77)[None] >= tokens[:, None]] = 0
    return text


def kept_rows(text):
    """(R, B L) of the decoder's rows: R up to every caption's last non-pad label (narrator.caption_row_lengths)."""
    labels = text[:, 1:]
    last = ((labels != 0) * torch.arange(1, labels.shape[1] + 1)).amax(dim=1).clamp(min=1)
    return int(last.sum()), labels.numel()


def run(model, batch, steps, warmup, stride, lengths='full'):
    from lavila.models import models
    crit = models.get_loss('VCLM_OPENAI_TIMESFORMER_BASE_GPT2', None, tokenizer=types.SimpleNamespace(pad_token_id=0))
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=1e-5)
    g = torch.Generator().manual_seed(1)
    video = torch.randn(batch, 3, 4, 224, 224, generator=g).cuda()
    text = captions(batch, lengths, g)
    rows = kept_rows(text)
    text = text.cuda()

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            out = crit(model(video, text))
        out['loss'].backward()
        opt.step()
        return out['loss']

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    pairs = []
    s.record()
    for i in range(steps):
        if i % stride == 0:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
        loss = step()
        if i % stride == 0:
            b.record()
            pairs.append((a, b))
    e.record()
    torch.cuda.synchronize()
    ms = s.elapsed_time(e) / steps
    per = [a.elapsed_time(b) for a, b in pairs]
    return ms, per, torch.cuda.max_memory_allocated() / 2 ** 30, loss.item(), sum(p.numel() for p in params), rows


def time_kernels(reps=20):
    from lavila_amd import _cabi as C
    contexts, qrep, H, Tk = 64, 76, 12, 256
    D, rows = H * 64, contexts * qrep
    q = torch.randn(rows, D, device='cuda').bfloat16()
    kv = torch.randn(contexts, Tk, 2 * D, device='cuda').bfloat16()
    do = torch.randn(rows, D, device='cuda').bfloat16()
    out, dq, dkv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(kv)
    fwd = lambda: C.check(C.lib().lvl_cross_attn_rows_fwd(C.ptr(q), C.ptr(kv), C.ptr(out), rows, qrep, Tk, H, 1,
                                                          C.stream_ptr()), 'fwd')
    bwd = lambda: C.check(C.lib().lvl_cross_attn_rows_bwd(C.ptr(q), C.ptr(kv), C.ptr(do), C.ptr(dq), C.ptr(dkv), rows, qrep,
                                                          Tk, H, 1, C.stream_ptr()), 'bwd')
    res = []
    for fn in (fwd, bwd):
        for _ in range(3):
            fn()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        res.append(1e3 * s.elapsed_time(e) / reps)
    return res


def time_row_kernels(batch, lengths, reps=20):
    """lvl_rows_pack / lvl_rows_unpack alone on the probe's captions: the decoder's [B, 76, 768] bf16 rows and the lm_head's
    padded product [R, 50432] -> [B, 76, 50432]: (name, us per call, GB/s read + written)."""
    from lavila_amd import ops
    text = captions(batch, lengths, torch.Generator().manual_seed(1))
    labels = text[:, 1:]
    n = ((labels != 0) * torch.arange(1, 77)).amax(dim=1).clamp(min=1)
    R = int(n.sum())
    cu = torch.cat([torch.zeros(1, dtype=torch.long), n.cumsum(0)]).to(torch.int32).cuda()
    res = []
    for D in (768, 2304, 50432):
        x = torch.randn(batch, 76, D, device='cuda').bfloat16()
        y = ops.rows_pack_raw(x, cu, R)
        out = torch.empty_like(x)
        for name, fn, moved in (('lvl_rows_pack', lambda: ops.rows_pack_raw(x, cu, R), 2 * R * D * 2),
                                ('lvl_rows_unpack', lambda: ops.rows_unpack_raw(y, cu, batch, 76, out=out),
                                 (R + batch * 76) * D * 2)):
            for _ in range(3):
                fn()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                fn()
            e.record()
            torch.cuda.synchronize()
            us = 1e3 * s.elapsed_time(e) / reps
            res.append((f'{name} [{batch}, 76, {D}] bf16, R = {R}', us, moved / us * 1e-3))
        del x, y, out
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--event-stride', type=int, default=4)
    ap.add_argument('--batches', type=int, nargs='+', default=[256, 128, 64, 32, 16])
    ap.add_argument('--no-kernels', action='store_true')
    ap.add_argument('--caption-lengths', choices=['full', 'standin'], default='full')
    ap.add_argument('--pack-captions', action='store_true')
    ap.add_argument('--row-kernels', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    packing = False
    if args.pack_captions:
        from lavila_amd import narrator
        narrator.PACK_CAPTIONS = packing = True
    elif os.environ.get('LAVILA_PACK_CAPTIONS', '0') == '1':
        packing = True
    model = build()
    ran = None
    for batch in args.batches:
        try:
            ms, per, peak, loss, n, (R, BL) = run(model, batch, args.steps, args.warmup, max(1, args.event_stride),
                                                  args.caption_lengths)
        except torch.OutOfMemoryError:
            say(f'local batch {batch}: out of memory')
            model.zero_grad(set_to_none=True)
            torch.cuda.empty_cache()
            continue
        say(f'narrator train step, TSF-B + GPT-2 gated, frozen LM and spatial tower ({n / 1e6:.1f} M trainable parameters), '
            f'4 frames, 77 tokens, bf16 autocast, local batch {batch}: {ms:.1f} ms per step, {1e3 * batch / ms:.1f} clips/s, '
            f'peak memory {peak:.1f} GiB, per-step events {[round(x, 1) for x in per]}, loss {loss:.3f}; captions '
            f'{args.caption_lengths}, packed rows {"ON" if packing else "off"}, R / (B L) = {R} / {BL} = {R / BL:.3f}')
        ran = batch
        break
    if not args.no_kernels:
        f, b = time_kernels()
        say(f'lvl_cross_attn_rows (64 contexts, qrep 76, 12 heads, Tk 256): forward {f:.1f} us, backward {b:.1f} us '
            f'({b / f:.2f}x)')
    if args.row_kernels and ran is not None:
        for name, us, gbs in time_row_kernels(ran, args.caption_lengths):
            say(f'{name}: {us:.1f} us per call, {gbs:.0f} GB/s')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
