"""What the exact-GELU epilogues of lvl_linear_tn cost and what they buy, on one device in one call, versions alternating:

  (1) fc1 + activation at the TSF-B shape, rows 50240 (64 clips x (1 + 4 x 196)), 768 -> 3072, bf16: epilogue 8
      (LVL_EPI_BIAS_GELU_DERIV), epilogue 6 (LVL_EPI_BIAS_GELU), their QuickGELU twins 4 and 1, the plain epilogue 0, and the
      composed form a GELU tower ran before (epilogue 0 with the bias, then torch's GELU over [rows, 3072]);
  (2) the backward of the same: fc2's input gradient, 768 -> 3072, with epilogue 5 (LVL_EPI_MUL_AUX_COLSUM: what the fused
      GELU backward runs, the same launch as QuickGELU's), epilogue 7 (LVL_EPI_GELU_BWD) and its twin 2, and the composed form
      (plain GEMM, torch's GELU backward, the bias gradient as column sums);
      (1) and (2) time kernels that this library holds in both forms, interleaved, median of --rounds x --reps launches;
  (3) a bf16 training step (forward + backward, no optimizer) of the default-constructed SpaceTimeTransformer at TSF-B geometry
      (224 / 16, width 768, depth 12, 12 heads, 4 frames, batch 64): this tree and, with --parent DIR (a built checkout of the
      commit before), that tree, in child processes, alternating;
  (4) `bench.py --gpus 1` at its defaults in both trees, alternating.

    python tools/probe_gelu_tower_step.py [--parent DIR] [--rounds 3] [--out profiles/gelu_tower_step.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, D, HID = 64 * (1 + 4 * 196), 768, 3072


def _ms(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def kernels(rounds, reps):
    """(1) and (2): name -> (median ms, min, max) over the rounds"""
    import torch
    import torch.nn.functional as F
    from lavila_amd import _cabi as C
    from lavila_amd import ops
    g = torch.Generator(device='cuda').manual_seed(0)
    x = torch.randn(ROWS, D, device='cuda', generator=g).bfloat16()
    w1 = (torch.randn(HID, D, device='cuda', generator=g) * D ** -0.5).bfloat16()
    b1 = torch.randn(HID, device='cuda', generator=g) * 0.5
    dy = torch.randn(ROWS, D, device='cuda', generator=g).bfloat16()
    w2t = (torch.randn(HID, D, device='cuda', generator=g) * HID ** -0.5).bfloat16()      # fc2's weight, transposed copy
    _, u = ops.linear_tn_raw(x, w1, b1, C.EPI_BIAS_GELU)
    _, dg = ops.linear_tn_raw(x, w1, b1, C.EPI_BIAS_GELU_DERIV)
    _, dq = ops.linear_tn_raw(x, w1, b1, C.EPI_BIAS_QUICKGELU_DERIV)
    gelu_bwd = torch.ops.aten.gelu_backward

    def composed_fwd():
        return F.gelu(ops.linear_tn_raw(x, w1, b1, C.EPI_BIAS))

    def composed_bwd():
        du = gelu_bwd(ops.linear_tn_raw(dy, w2t, None, C.EPI_BIAS), u)
        return du, du.sum(0, dtype=torch.float32)
    cases = {
        'fwd  epilogue 8  bias + GELU, keeps gelu\'(u)': lambda: ops.linear_tn_raw(x, w1, b1, C.EPI_BIAS_GELU_DERIV),
        'fwd  epilogue 4  bias + QuickGELU, keeps quickgelu\'(u)': lambda: ops.linear_tn_raw(x, w1, b1, C.EPI_BIAS_QUICKGELU_DERIV),
        'fwd  epilogue 6  bias + GELU, keeps u': lambda: ops.linear_tn_raw(x, w1, b1, C.EPI_BIAS_GELU),
        'fwd  epilogue 1  bias + QuickGELU, keeps u': lambda: ops.linear_tn_raw(x, w1, b1, C.EPI_BIAS_QUICKGELU),
        'fwd  epilogue 0  bias only': lambda: ops.linear_tn_raw(x, w1, b1, C.EPI_BIAS),
        'fwd  composed    epilogue 0 + torch GELU pass': composed_fwd,
        'bwd  epilogue 5  acc * kept gelu\'(u), column sums': lambda: ops.linear_tn_raw(dy, w2t, None, C.EPI_MUL_AUX_COLSUM, aux_in=dg),
        'bwd  epilogue 5  acc * kept quickgelu\'(u), column sums': lambda: ops.linear_tn_raw(dy, w2t, None, C.EPI_MUL_AUX_COLSUM, aux_in=dq),
        'bwd  epilogue 7  acc * gelu\'(kept u), column sums': lambda: ops.linear_tn_raw(dy, w2t, None, C.EPI_GELU_BWD, aux_in=u),
        'bwd  epilogue 2  acc * quickgelu\'(kept u), column sums': lambda: ops.linear_tn_raw(dy, w2t, None, C.EPI_QUICKGELU_BWD, aux_in=u),
        'bwd  composed    epilogue 0 + torch GELU backward + column sums': composed_bwd,
    }
    for fn in cases.values():          # warm every shape and code object
        _ms(fn, 3)
    got = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            got[k].append(_ms(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def child_tower(steps, warmup):
    """(3), in the tree given by --root: prints one JSON line"""
    import contextlib
    import io
    import torch
    from lavila.models.timesformer import SpaceTimeTransformer
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        vis = SpaceTimeTransformer(num_frames=4, time_init='zeros', attention_style='frozen-in-time', num_classes=0)
    with torch.no_grad():
        for p in vis.parameters():
            if p.ndim > 1:
                p.normal_(0, 0.02)
    vis.cuda().train()
    video = torch.randn(64, 3, 4, 224, 224, generator=torch.Generator().manual_seed(1)).cuda()
    times = []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        vis.zero_grad(set_to_none=True)
        a.record()
        with torch.autocast('cuda', dtype=torch.bfloat16):
            out = vis(video)
        out.float().square().sum().backward()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    print(json.dumps({'tower_step_ms': statistics.median(times), 'min': min(times), 'max': max(times),
                      'out_norm': out.float().norm().item()}), flush=True)


def _child(root, args, what):
    env = dict(os.environ, PYTHONPATH=root)
    if what == 'tower':
        cmd = [sys.executable, os.path.abspath(__file__), '--child', '--root', root, '--steps', str(args.steps),
               '--warmup', str(args.warmup)]
    else:
        cmd = [sys.executable, 'bench.py', '--gpus', '1']
    out = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError(f'{cmd} in {root} failed ({out.returncode}):\n{out.stderr[-2000:]}')
    line = [ln for ln in out.stdout.splitlines() if ln.startswith('{')][-1]
    return json.loads(line)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--parent', default=None, help='a built checkout of the commit before (its library compiled)')
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--reps', type=int, default=20)
    p.add_argument('--steps', type=int, default=6)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--out', default=os.path.join(HERE, 'profiles', 'gelu_tower_step.txt'))
    p.add_argument('--skip-bench', action='store_true')
    p.add_argument('--child', action='store_true', help='internal: run (3) in the tree given by --root')
    p.add_argument('--root', default=HERE)
    args = p.parse_args()
    sys.path.insert(0, args.root)
    if args.child:
        return child_tower(args.steps, args.warmup)
    import torch
    assert torch.cuda.is_available(), 'the probe needs an MI355X'
    lines = [f'# tools/probe_gelu_tower_step.py on {torch.cuda.get_device_name(0)}; rows {ROWS}, {D} -> {HID}, bf16',
             f'# (1), (2): median [min .. max] ms per launch over {args.rounds} interleaved rounds of {args.reps} launches']
    for k, (med, lo, hi) in kernels(args.rounds, args.reps).items():
        lines.append(f'{k:68s} {med:7.3f}  [{lo:.3f} .. {hi:.3f}]')
        print(lines[-1], flush=True)
    trees = [('this commit', HERE)] + ([('parent', os.path.abspath(args.parent))] if args.parent else [])
    lines.append(f'# (3) bf16 training step of the default-constructed (GELU) SpaceTimeTransformer, TSF-B geometry, 4 frames, '
                 f'batch 64: median of {args.steps} steps per child, children alternating')
    for what in ('tower',) + (() if args.skip_bench else ('bench',)):
        if what == 'bench':
            lines.append('# (4) bench.py --gpus 1 (defaults), children alternating')
        for r in range(args.rounds if what == 'tower' else min(args.rounds, 2)):
            for name, root in trees:
                rec = _child(root, args, what)
                if what == 'tower':
                    lines.append(f'tower step, {name:12s} round {r}: {rec["tower_step_ms"]:8.2f} ms  [{rec["min"]:.2f} .. '
                                 f'{rec["max"]:.2f}]  |out| {rec["out_norm"]:.4f}')
                else:
                    lines.append(f'bench.py,   {name:12s} round {r}: {rec["value"]:9.2f} {rec["unit"]}, '
                                 f'{rec["ms_per_step"]:.2f} ms per step')
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('->', args.out)


if __name__ == '__main__':
    main()
