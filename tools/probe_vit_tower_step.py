"""What the per-frame OpenAI CLIP image tower costs next to the TimeSformer of the same width, on one device in one call:

  (1) a bf16 training step (forward + CaptionLoss + backward, no optimizer) of a narrator with the ViT-B/16 tower
      (`VCLM_OPENAI_VITB16_*` geometry: 12 blocks of width 768, 197 tokens per frame) and a small decoder (GPT-2 width, 2 layers,
      cross-attention in every block, LM frozen), 4 frames, local batch 32, 32-token captions; beside it the same narrator
      around the TimeSformer-B tower (`VCLM_OPENAI_TIMESFORMER_BASE_*` geometry: one 785-token sequence per clip, divided
      space-time attention) as orientation -- the per-frame tower has no time attention and does strictly less attention work;
  (2) inference `encode_image` of the `CLIP_OPENAI_VITB16` geometry on 4-frame clips (batch 32, bf16 autocast), beside
      `CLIP_OPENAI_TIMESFORMER_BASE.encode_image` on the same clips;
  (3) `bench.py --gpus 1` at its defaults in this tree and, with --parent DIR (a built checkout of the commit before), in
      that tree, in child processes, alternating.

Every model runs in a child process of its own (models alternate, --rounds rounds each); times are device events around whole
steps, median [min .. max] of --steps steps after --warmup warm-up steps.

    python tools/probe_vit_tower_step.py [--parent DIR] [--rounds 2] [--out profiles/vit_tower_step.txt]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import types
import warnings

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, FRAMES, CAPTION = 32, 4, 32


def _timed(step, steps, warmup):
    import torch
    times = []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = step()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    return {'ms': statistics.median(times), 'min': min(times), 'max': max(times), 'check': out}


def _towers(kind):
    """(tower, vision width) at the B/16 geometry"""
    from lavila.models.openai_model import QuickGELU, VisionTransformer
    from lavila.models.timesformer import SpaceTimeTransformer
    if kind == 'vit':
        return VisionTransformer(224, 16, 768, 12, 12, 512)
    vis = SpaceTimeTransformer(num_frames=FRAMES, time_init='zeros', attention_style='frozen-in-time', ln_pre=True,
                               act_layer=QuickGELU)
    import torch
    vis.head = vis.pre_logits = vis.fc = torch.nn.Identity()
    return vis


def child_narrator(kind, steps, warmup):
    import torch
    from lavila.models.loss import CaptionLoss
    from lavila_amd.gpt2_gated import GPT2LMHeadModel, augment_gpt2_config, gpt2_config
    from lavila_amd.narrator import VCLM_HF
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        vis = _towers(kind)
        dec = GPT2LMHeadModel(augment_gpt2_config(gpt2_config('gpt2', n_layer=2), cross_attn_freq=1, gated_xattn=False))
        dec.freeze_lm_weights()
        m = VCLM_HF(vision_width=768, vision_model=vis, text_width=768, text_decoder=dec, num_img_queries=256, dim_head=64,
                    heads=12)
    m.cuda().train()
    g = torch.Generator().manual_seed(1)
    video = torch.randn(BATCH, 3, FRAMES, 224, 224, generator=g).cuda()
    text = torch.randint(1, 50000, (BATCH, CAPTION + 1), generator=g).cuda()
    crit = CaptionLoss(tokenizer=types.SimpleNamespace(pad_token_id=0))

    def step():
        m.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            res = crit(m(video, text))
        res['loss'].backward()
        return res['loss'].item()
    print(json.dumps(_timed(step, steps, warmup)), flush=True)


def child_encode(kind, steps, warmup):
    import torch
    from lavila.models import models
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = models.CLIP_OPENAI_VITB16() if kind == 'vit' else models.CLIP_OPENAI_TIMESFORMER_BASE(num_frames=FRAMES)
    m.cuda().eval()
    video = torch.randn(BATCH, 3, FRAMES, 224, 224, generator=torch.Generator().manual_seed(1)).cuda()

    def step():
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            return m.encode_image(video).float().norm().item()
    print(json.dumps(_timed(step, steps, warmup)), flush=True)


def _child(root, args, what, kind=None):
    env = dict(os.environ, PYTHONPATH=root)
    if what == 'bench':
        cmd = [sys.executable, 'bench.py', '--gpus', '1']
    else:
        cmd = [sys.executable, os.path.abspath(__file__), '--child', what, '--kind', kind, '--root', root, '--steps',
               str(args.steps), '--warmup', str(args.warmup)]
    out = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError(f'{cmd} in {root} failed ({out.returncode}):\n{out.stderr[-2000:]}')
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{')][-1])


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--parent', default=None, help='a built checkout of the commit before (its library compiled)')
    p.add_argument('--rounds', type=int, default=2)
    p.add_argument('--steps', type=int, default=8)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--out', default=os.path.join(HERE, 'profiles', 'vit_tower_step.txt'))
    p.add_argument('--skip-bench', action='store_true')
    p.add_argument('--child', default=None, choices=['narrator', 'encode'], help='internal: one measurement in --root')
    p.add_argument('--kind', default='vit', choices=['vit', 'timesformer'])
    p.add_argument('--root', default=HERE)
    args = p.parse_args()
    sys.path.insert(0, args.root)
    if args.child:
        return {'narrator': child_narrator, 'encode': child_encode}[args.child](args.kind, args.steps, args.warmup)
    import torch
    assert torch.cuda.is_available(), 'the probe needs an MI355X'
    lines = [f'# tools/probe_vit_tower_step.py on {torch.cuda.get_device_name(0)}; batch {BATCH} clips of {FRAMES} x 224^2, bf16 '
             f'autocast; median [min .. max] ms of {args.steps} steps after {args.warmup}, one child process per line, '
             'models alternating']
    titles = {'narrator': f'# (1) narrator training step (2-layer decoder, LM frozen, {CAPTION}-token captions): ViT-B/16 per '
                          'frame | TimeSformer-B',
              'encode': '# (2) inference encode_image: CLIP_OPENAI_VITB16 | CLIP_OPENAI_TIMESFORMER_BASE'}
    for what in ('narrator', 'encode'):
        lines.append(titles[what])
        for r in range(args.rounds):
            for kind in ('vit', 'timesformer'):
                rec = _child(HERE, args, what, kind)
                lines.append(f'{what:9s} {kind:12s} round {r}: {rec["ms"]:8.2f} ms  [{rec["min"]:.2f} .. {rec["max"]:.2f}]  '
                             f'check {rec["check"]:.4f}')
                print(lines[-1], flush=True)
    if not args.skip_bench:
        trees = [('this commit', HERE)] + ([('parent', os.path.abspath(args.parent))] if args.parent else [])
        lines.append('# (3) bench.py --gpus 1 (defaults), children alternating')
        for r in range(args.rounds):
            for name, root in trees:
                rec = _child(root, args, 'bench')
                lines.append(f'bench.py,   {name:12s} round {r}: {rec["value"]:9.2f} {rec["unit"]}, '
                             f'{rec["ms_per_step"]:.3f} ms per step, final loss {rec["config"]["final_loss"]}')
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('->', args.out)


if __name__ == '__main__':
    main()
