"""Times the clip ingest at the pretraining step's shape: 256 clips x 4 frames of 288 x 384 uint8 source, RandomResizedCrop
blocks (one per clip) and a flip per clip, to S = 224 / 16-pixel patches and to S = 336 / 14-pixel patches (ld = 640).

    python tools/probe_clip_ingest.py                 device-event times, profiler off, the variants alternating in one process:
      two    lvl_clip_ingest (float32 clip) + lvl_patchify (bf16 patches): the clip exists
      fused  lvl_clip_ingest_patches alone (bf16 patches, zero pad columns included)
      torch  the composed device path both replace: per clip .float(), slice, F.interpolate, flip, normalise, stack;
             then lvl_patchify (and F.pad to 640 for the 14-pixel patches)
      torch1 the same with ONE block for the whole batch (one slice, one interpolate): what the composed path costs when
             the launches per clip are taken out of it -- not the reference's semantics (it crops per clip)
    and the host-to-device copy, from pinned memory, of the uint8 source against the float32 clip.
    Bytes: the source bytes of the regions (read once) + the bytes written (+ the clip written and read again for `two`),
    over the time, against the copy ceiling of profiles/r04_hbm_mix_ceiling.txt (1 read + 1 write: 5.47 TB/s).
Needs an MI355X; prints what it measured, asserts only that the three paths agree.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from lavila_amd import ops  # noqa: E402
from lavila_amd.ingest import OPENAI_MEAN_STD, ClipIngest, random_resized_crop_params  # noqa: E402

COPY_CEILING = 5.47e12          # bytes / s, profiles/r04_hbm_mix_ceiling.txt, "copy", grid 8192 x 256


def event_time(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3, out      # microseconds


def alternate(variants, reps, warmup=3):
    """name -> sorted list of times (us); one call of every variant per round, in turn"""
    times = {k: [] for k in variants}
    for r in range(warmup + reps):
        for k, fn in variants.items():
            t, _ = event_time(fn)
            if r >= warmup:
                times[k].append(t)
    return {k: sorted(v) for k, v in times.items()}


def report(name, ts, nbytes=None):
    med, lo = statistics.median(ts), ts[0]
    line = f'  {name:<8} median {med:9.1f} us   min {lo:9.1f} us   max {ts[-1]:9.1f} us'
    if nbytes is not None:
        rate = nbytes / (lo * 1e-6)
        line += f'   {nbytes / 1e6:8.1f} MB -> {rate / 1e12:5.2f} TB/s at the min = {rate / COPY_CEILING:5.2f} of the copy ceiling'
    print(line, flush=True)


def composed(frames, params, flip, S, mean, std, patch, pad_to):
    B = frames.shape[0]
    m = torch.tensor(mean, device=frames.device).view(3, 1, 1, 1)
    s = torch.tensor(std, device=frames.device).view(3, 1, 1, 1)
    rows = params.tolist()
    flips = flip.tolist()

    def run():
        out = []
        for b in range(B):
            top, left, h, w = rows[b][:4]
            x = frames[b, :, top:top + h, left:left + w].float().permute(3, 0, 1, 2)
            x = F.interpolate(x, size=(S, S), mode='bilinear', align_corners=False)
            if flips[b]:
                x = x.flip(-1)
            out.append((x - m) / s)
        p = ops.patchify(torch.stack(out), patch, torch.bfloat16)
        return F.pad(p, (0, pad_to - p.shape[-1])) if pad_to > p.shape[-1] else p
    return run


def composed_one_block(frames, block, S, mean, std, patch, pad_to):
    m = torch.tensor(mean, device=frames.device).view(1, 3, 1, 1, 1)
    s = torch.tensor(std, device=frames.device).view(1, 3, 1, 1, 1)
    top, left, h, w = block[:4]
    B, Fr = frames.shape[:2]

    def run():
        x = frames[:, :, top:top + h, left:left + w].float().permute(0, 1, 4, 2, 3).reshape(B * Fr, 3, h, w)
        x = F.interpolate(x, size=(S, S), mode='bilinear', align_corners=False).view(B, Fr, 3, S, S).permute(0, 2, 1, 3, 4)
        p = ops.patchify((x - m) / s, patch, torch.bfloat16)
        return F.pad(p, (0, pad_to - p.shape[-1])) if pad_to > p.shape[-1] else p
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clips', type=int, default=256)
    ap.add_argument('--frames', type=int, default=4)
    ap.add_argument('--height', type=int, default=288)
    ap.add_argument('--width', type=int, default=384)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    B, Fr, H, W = args.clips, args.frames, args.height, args.width
    mean, std = OPENAI_MEAN_STD
    g = torch.Generator().manual_seed(0)
    host = torch.randint(0, 256, (B, Fr, H, W, 3), dtype=torch.uint8, generator=g).pin_memory()
    frames = host.cuda()
    flip = (torch.rand(B, generator=g) < 0.5).to(torch.int32)
    print(f'{torch.cuda.get_device_name(0)}; {B} clips x {Fr} frames, source {H} x {W} uint8 ({host.numel() / 1e6:.1f} MB), '
          f'{args.reps} rounds, variants alternating', flush=True)
    for S, P, ld in ((224, 16, 768), (336, 14, 640)):
        ci = ClipIngest(S, mean, std)
        params = random_resized_crop_params(B, H, W, S, generator=g)
        pend = ci.pending(frames, params, flip)
        region = int((params[:, 2] * params[:, 3]).sum()) * 3 * Fr
        rows = B * Fr * (S // P) ** 2
        clip_bytes = B * 3 * Fr * S * S * 4
        variants = {
            'two': lambda: ops.patchify(pend.materialize(torch.float32), P, torch.bfloat16),
            'fused': lambda: ops.patchify(pend, P, torch.bfloat16, ld=ld),
            'torch': composed(frames, params, flip, S, mean, std, P, ld),
            'torch1': composed_one_block(frames, params[0].tolist(), S, mean, std, P, ld),
        }
        two, fused, torch_path = variants['two'](), variants['fused'](), variants['torch']()
        k = 3 * P * P
        assert torch.equal(two, fused[..., :k]) and bool((fused[..., k:] == 0).all())
        diff = (torch_path[..., :k].float() - two.float()).abs().max().item()
        print(f'\nS = {S}, P = {P}, ld = {ld}: {rows} patch rows; region bytes {region / 1e6:.1f} MB, float32 clip '
              f'{clip_bytes / 1e6:.1f} MB, bf16 patches {rows * ld * 2 / 1e6:.1f} MB; fused == two (bits); max |torch - two| = '
              f'{diff:.3g} (bf16 patches)', flush=True)
        del two, fused, torch_path
        ts = alternate(variants, args.reps)
        report('two', ts['two'], region + 2 * clip_bytes + rows * k * 2)
        report('fused', ts['fused'], region + rows * ld * 2)
        report('torch', ts['torch'])
        report('torch1', ts['torch1'])
        # the two kernels of `two`, each alone
        clip = pend.materialize(torch.float32)
        parts = alternate({'ingest': lambda: pend.materialize(torch.float32),
                           'patchify': lambda: ops.patchify(clip, P, torch.bfloat16)}, args.reps)
        report('ingest', parts['ingest'], region + clip_bytes)
        report('patchify', parts['patchify'], clip_bytes + rows * k * 2)
        # host to device, pinned
        clip_host = torch.empty(clip.shape, dtype=torch.float32).pin_memory()
        clip_host.copy_(clip)
        dst_u8, dst_f32 = torch.empty_like(frames), torch.empty_like(clip)
        h2d = alternate({'u8': lambda: dst_u8.copy_(host, non_blocking=True),
                         'f32': lambda: dst_f32.copy_(clip_host, non_blocking=True)}, 8, warmup=2)
        for name, n in (('u8', host.numel()), ('f32', clip_bytes)):
            lo = h2d[name][0]
            print(f'  h2d {name:<4} {n / 1e6:8.1f} MB pinned: median {statistics.median(h2d[name]) / 1e3:8.2f} ms, min '
                  f'{lo / 1e3:8.2f} ms = {n / lo / 1e3:6.1f} GB/s', flush=True)
        del clip, clip_host, dst_u8, dst_f32, pend
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
