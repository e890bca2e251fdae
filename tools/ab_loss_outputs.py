"""Bit-for-bit A/B of the contrastive and ranking losses between two trees (a refactor of the slab kernels' shared device
code and of the exchange layer in lavila_amd/loss.py).

    python tools/ab_loss_outputs.py run OUT.pt            on THIS tree, seeded random embeddings, float32 and bfloat16:
                                                          every output (stats, argmax, logits, dimg, dtxt) of the four
                                                          contrastive entries over CLIP_SPECS + SSL_SPECS + LARGE_SPECS of
                                                          tests/clip_loss_reference.py, and on one rank the loss,
                                                          accuracies and input gradients of CLIPLoss, SSLCLIPLoss and
                                                          both margin losses
    python tools/ab_loss_outputs.py compare A.pt B.pt     torch.equal on every tensor; exit status 1 when anything differs

Run it twice on the parent (it must reproduce itself), once on the tree, and compare."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16}


def _embeddings(G, E, seed, dt):
    g = torch.Generator().manual_seed(seed)
    img = torch.nn.functional.normalize(torch.randn(G, E, generator=g), dim=-1)
    txt = torch.nn.functional.normalize(torch.randn(G, E, generator=g) + 0.5 * img, dim=-1)
    ind = torch.randint(0, 2, (G,), generator=g).to(torch.int32)
    return img.to(dt).cuda(), txt.to(dt).cuda(), ind.cuda()


def _kernels(res):
    import clip_loss_reference as R
    from lavila_amd import ops
    up = torch.tensor([0.7], device='cuda')
    for seed, (kind, B, G, E, row0, n) in enumerate(R.CLIP_SPECS + R.SSL_SPECS + R.LARGE_SPECS):
        for name, dt in DTYPES.items():
            img, txt, ind = _embeddings(G, E, 1000 + seed, dt)
            out = {}
            if kind == 'clip':
                scale = torch.tensor([14.285714], device='cuda')
                out['stats'], out['argmax'], out['logits'] = ops.clip_loss_fwd_raw(img, txt, scale, B, row0, want_logits=True)
                lse_all = ops.clip_loss_fwd_raw(img, txt, scale, G, 0)[0][..., 0].contiguous()      # all 2G row LSEs
                out['dimg'], out['dtxt'] = ops.clip_loss_bwd_raw(img, txt, lse_all, scale, up, 3.0 / (2 * G), B, row0)
                out['dimg_rows'], out['dtxt_rows'] = ops.clip_loss_bwd_raw(img, txt, lse_all, scale, up, 1.0 / (2 * B), B,
                                                                           row0, rows_only=True)
            else:
                s3 = torch.tensor([12.5, (12.5 * 14.285714) ** 0.5, 14.285714], device='cuda')
                out['stats'], out['argmax'], out['logits'] = ops.ssl_clip_loss_fwd_raw(img, txt, ind, s3, B, row0,
                                                                                       want_logits=True)
                lse_all = ops.ssl_clip_loss_fwd_raw(img, txt, ind, s3, G, 0)[0][..., 0].contiguous()
                out['dimg'], out['dtxt'] = ops.ssl_clip_loss_bwd_raw(img, txt, ind, lse_all, s3, up, 3.0 / (2 * G), B, row0)
            out['lse_all'] = lse_all
            res[f'{kind} B={B} G={G} E={E} row0={row0} {name}'] = {k: v.cpu() for k, v in out.items()}


def _criteria(res):
    from lavila_amd import loss as L
    # (B, E): matrix-core forward, VALU forward twice; the margin kernels take E in {64, 128, 256, 512}
    contrastive, margin = ((32, 256), (5, 24), (33, 768)), ((32, 256), (5, 64), (33, 512))
    for crit_name in ('CLIPLoss', 'SSLCLIPLoss', 'MaxMarginRankingLoss', 'AdaptiveMaxMarginRankingLoss'):
        for seed, (B, E) in enumerate(margin if 'Margin' in crit_name else contrastive):
            for name, dt in DTYPES.items():
                img, txt, ind = _embeddings(B, E, 2000 + seed, dt)
                img.requires_grad_(True), txt.requires_grad_(True)
                scale = torch.tensor(14.285714, device='cuda', requires_grad=True)
                outputs = {'image_embed': img, 'text_embed': txt, 'logit_scale': scale}
                crit = getattr(L, crit_name)().cuda()
                if crit_name == 'SSLCLIPLoss':
                    out = crit(outputs, ind)
                elif crit_name == 'AdaptiveMaxMarginRankingLoss':
                    out = crit(outputs, torch.rand(B, generator=torch.Generator().manual_seed(seed)).cuda())
                else:
                    out = crit(outputs)
                (out['loss'] * 0.7).backward()
                got = {k: v.detach().cpu() for k, v in out.items()}
                got.update({'d_' + k: t.grad.cpu() for k, t in (('img', img), ('txt', txt), ('scale', scale))
                            if t.grad is not None})
                if crit_name == 'SSLCLIPLoss':
                    got['d_scale_pseudo'] = crit.logit_scale_pseudo.grad.cpu()
                res[f'{crit_name} B={B} E={E} {name}'] = got


def run(path):
    res = {}
    _kernels(res)
    _criteria(res)
    torch.cuda.synchronize()
    torch.save(res, path)
    print(f'{len(res)} cases, {sum(len(v) for v in res.values())} tensors -> {path}')


def compare(path_a, path_b):
    a, b = torch.load(path_a), torch.load(path_b)
    bad = []
    if list(a) != list(b):
        bad.append(f'case lists differ: {sorted(set(a) ^ set(b))}')
    for name in a:
        if name not in b:
            continue
        x, y = a[name], b[name]
        diffs = [f'tensor names {sorted(set(x) ^ set(y))}'] if set(x) != set(y) else []
        diffs += [k for k in x if k in y and not torch.equal(x[k], y[k])]
        if diffs:
            bad.append(f'{name}: ' + ', '.join(diffs))
    print(f'{path_a} vs {path_b}: {len(a)} cases, {sum(len(v) for v in a.values())} tensors, {len(bad)} cases differ')
    for line in bad:
        print('  DIFFERS', line)
    return not bad


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == 'run':
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == 'compare':
        sys.exit(0 if compare(sys.argv[2], sys.argv[3]) else 1)
    else:
        sys.exit(__doc__)
