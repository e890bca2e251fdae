"""Times the narrator's criterion at the GPT-2 vocabulary (V = 50257, 76 label positions, 32 and 256 captions, bf16).

    python tools/probe_caption_loss.py [--captions 32 256] [--out FILE]

For each batch and for two layouts of the [B*T, V] logits -- the [:, :V] view of a padded product (row stride 50264) and
row stride 50257 (the F.linear fallback, the reference's own tensors) -- device-event times, profiler off, of
  new        lavila_amd.loss.CaptionLoss on the [B,V,T] permuted view: forward (loss, caption_acc, ppl) and
             forward + backward;
  composite  F.cross_entropy(logits.float(), labels, ignore_index=pad, reduction='none') plus the reference's metric loop
             (loss.py:234-252: an argmax of [V,T] per caption, B read-backs for ppl), forward and forward + backward
on the same tensors in the same process, alternated, both warmed up; 5 rounds, median (min, max). Also the bytes each
pass of the new path has to move (forward: the logits once; backward: the logits once + the gradient once) over its time
against the 6.3 TB/s copy rate, and torch.cuda.max_memory_allocated of a forward + backward of each above the tensors
that exist before it. Needs an MI355X; prints what it measured, asserts nothing.
"""
import argparse
import os
import sys
from types import SimpleNamespace

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from lavila_amd.loss import CaptionLoss  # noqa: E402

V, T, PAD = 50257, 76, 0
COPY_RATE = 6.3e12


def timed(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / reps      # microseconds


def composite(logits, labels):
    """The reference's forward (loss.py:227-253) with the float32 copy GPT2LMHeadModel.forward(labels=) makes."""
    loss = F.cross_entropy(logits.float(), labels, ignore_index=PAD, reduction='none')
    with torch.no_grad():
        correct, total, ppls = 0., 0., []
        for i in range(logits.size(0)):
            pred = torch.argmax(logits[i], dim=0)
            nopad = labels[i].ne(PAD)
            correct += (pred.eq(labels[i]) & nopad).sum()
            total += nopad.sum()
            ppls.append(torch.exp(loss[i].sum() / nopad.sum()))
        acc = 100 * correct / (total + 1e-8)
    return loss.mean(), acc, torch.tensor(ppls).mean()


def peak_above(fn, leaf):
    leaf.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--captions', type=int, nargs='+', default=[32, 256])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    crit = CaptionLoss(tokenizer=SimpleNamespace(pad_token_id=PAD))
    say(f'device {torch.cuda.get_device_name(0)}; V={V} T={T} bf16; times in us, median (min, max) of 5 rounds x {args.reps} reps')
    for B in args.captions:
        g = torch.Generator().manual_seed(B)
        labels = torch.randint(1, V, (B, T), generator=g)
        for b in range(B):
            labels[b, 20 + (b * 7) % 50:] = PAD                          # ragged pad tails
        labels = labels.cuda()
        for stride in ((V + 7) // 8 * 8, V):
            base = torch.empty(B, T, stride, dtype=torch.bfloat16, device='cuda')
            for b0 in range(0, B, 32):                                      # filled in pieces: no [B,T,V] float32 image
                base[b0:b0 + 32] = (3.0 * torch.randn(min(32, B - b0), T, stride, device='cuda')).bfloat16()
            leaf = base[:, :, :V].permute(0, 2, 1).detach().requires_grad_(True)      # [B,V,T], read in place
            outputs = {'text_tokens_logits': leaf, 'labels': labels}

            def new_fwd():
                with torch.no_grad():
                    return crit(outputs)

            def new_both():
                leaf.grad = None
                crit(outputs)['loss'].backward()

            def old_fwd():
                with torch.no_grad():
                    return composite(leaf, labels)

            def old_both():
                leaf.grad = None
                composite(leaf, labels)[0].backward()

            fns = (new_fwd, new_both, old_fwd, old_both)
            for fn in fns:
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            rounds = [[timed(fn, args.reps if k < 2 else max(args.reps // 4, 2)) for k, fn in enumerate(fns)]
                      for _ in range(5)]
            med = [sorted(r[k] for r in rounds) for k in range(4)]
            new_out, old_out = new_fwd(), old_fwd()
            rows, esz = B * T, 2
            counted = int((labels != PAD).sum())
            fwd_bytes = rows * V * esz                                     # every row is read in forward
            bwd_bytes = counted * V * esz + rows * ((V + 7) // 8 * 8) * esz  # pad rows are not read in backward
            t_f, t_fb = med[0][2], med[1][2]
            say(f'B={B} row stride {stride}:')
            say(f'  new        forward {t_f:9.1f} ({med[0][0]:.1f}, {med[0][-1]:.1f})   forward+backward {t_fb:9.1f} '
                f'({med[1][0]:.1f}, {med[1][-1]:.1f})')
            say(f'  composite  forward {med[2][2]:9.1f} ({med[2][0]:.1f}, {med[2][-1]:.1f})   forward+backward '
                f'{med[3][2]:9.1f} ({med[3][0]:.1f}, {med[3][-1]:.1f})')
            say(f'  new: forward {fwd_bytes / 2 ** 20:.0f} MiB -> {fwd_bytes / (t_f * 1e-6) / 1e12:.2f} TB/s '
                f'({100 * fwd_bytes / (t_f * 1e-6) / COPY_RATE:.0f} % of the copy rate, whole criterion incl. launches); '
                f'backward {bwd_bytes / 2 ** 20:.0f} MiB in {t_fb - t_f:.1f} us -> '
                f'{bwd_bytes / ((t_fb - t_f) * 1e-6) / 1e12:.2f} TB/s '
                f'({100 * bwd_bytes / ((t_fb - t_f) * 1e-6) / COPY_RATE:.0f} %)')
            say(f'  peak memory above the inputs, forward+backward: new {peak_above(new_both, leaf):.0f} MiB, composite '
                f'{peak_above(old_both, leaf):.0f} MiB (logits {rows * stride * esz / 2 ** 20:.0f} MiB)')
            say(f'  values: new loss {new_out["loss"].item():.5f} acc {new_out["caption_acc"].item():.4f} ppl '
                f'{new_out["ppl"].item():.2f}; composite loss {old_out[0].item():.5f} acc {old_out[1].item():.4f} ppl '
                f'{old_out[2].item():.2f}')
            del leaf, base, outputs
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
