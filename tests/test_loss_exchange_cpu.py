"""CPU (-m "not gpu"): what the contrastive and ranking losses put on the wire, on 2 gloo ranks.

The value tests (test_distributed_cpu.py, test_margin_loss_cpu.py) pass float32 embeddings and check results; a change of
the wire dtype for bf16 embeddings, a second gather or a backward collective would pass them all. Here
`torch.distributed.all_gather_into_tensor` itself is wrapped with a recorder and every loss runs forward and backward on
float32, bfloat16 and mixed embeddings with B = 3, E = 8; the recorded (shape, dtype) lists per phase must equal the
plan of lavila_amd/loss.py:

  criterion (W = 2)                             gather 1              gather 2            backward
  CLIPLoss, global loss (vissl / gather path)   [B, 2E]   dt          [1, 2B+3] f32       none
  CLIPLoss(local_loss, gather_with_grad)        [B, 2E]   dt          [1, 2B+3] f32       none
  CLIPLoss(local_loss)                          [B, 2E]   dt          none                none
  SSLCLIPLoss                                   [B, 2E+1] f32         [1, 2B+7] f32       none
  MaxMarginRankingLoss                          [B, 2E]   dt          [1, 1]    f32       none
  AdaptiveMaxMarginRankingLoss                  [B, 2E+1] f32         [1, 1]    f32       none

dt = the embeddings' common dtype when both agree and it is float32 or bfloat16, float32 otherwise. One rank records
nothing. The kernel hooks are stubs that return tensors of the kernels' shapes: only the exchange is under test.
"""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

B, E = 3, 8
F32, BF16 = 'torch.float32', 'torch.bfloat16'
DTYPES = {'f32': (torch.float32, torch.float32, F32), 'bf16': (torch.bfloat16, torch.bfloat16, BF16),
          'mixed': (torch.float32, torch.bfloat16, F32)}          # image dtype, text dtype, dt
CASES = ['clip_vissl', 'clip_gather', 'clip_local_grad', 'clip_local', 'ssl', 'margin', 'adaptive']


def expected(case, dt):
    rows, rows_extra = ((B, 2 * E), dt), ((B, 2 * E + 1), F32)
    return {'clip_vissl': [rows, ((1, 2 * B + 3), F32)], 'clip_gather': [rows, ((1, 2 * B + 3), F32)],
            'clip_local_grad': [rows, ((1, 2 * B + 3), F32)], 'clip_local': [rows],
            'ssl': [rows_extra, ((1, 2 * B + 7), F32)], 'margin': [rows, ((1, 1), F32)],
            'adaptive': [rows_extra, ((1, 1), F32)]}[case]


def _criterion(case, rank, world):
    from lavila.models import loss as L

    def clip_fwd(img_all, txt_all, scale, b, row0):
        return torch.ones(2, b, 4), torch.zeros(2, b, dtype=torch.int32)

    def clip_bwd(img_all, txt_all, lse_all, scale, upstream, coef, b, row0, rows_only=False):
        return torch.ones(b, img_all.shape[1]), torch.ones(b, img_all.shape[1])

    def ssl_fwd(img_all, txt_all, ind_all, scales3, b, row0):
        return torch.ones(2, b, 8), torch.zeros(2, b, dtype=torch.int32)

    def ssl_bwd(img_all, txt_all, ind_all, lse_all, scales3, upstream, coef, b, row0):
        return torch.ones(b, img_all.shape[1]), torch.ones(b, img_all.shape[1])

    def margin_prepare(img_all, txt_all, weight_all, margin):
        return torch.ones(7, img_all.shape[0])

    def margin_fwd(img_all, txt_all, prep, b, row0, with_diag):
        return torch.ones(2, b), torch.zeros(2, b, dtype=torch.int32)

    def margin_bwd(img_all, txt_all, prep, upstream, coef, b, row0):
        return torch.ones(b, img_all.shape[1]), torch.ones(b, img_all.shape[1])

    if case.startswith('clip'):
        kw = {'clip_vissl': dict(use_vissl=True), 'clip_gather': dict(),
              'clip_local_grad': dict(local_loss=True, gather_with_grad=True), 'clip_local': dict(local_loss=True)}[case]
        crit = L.CLIPLoss(rank=rank, world_size=world, **kw)
        crit._slab_forward, crit._slab_backward = clip_fwd, clip_bwd
    elif case == 'ssl':
        crit = L.SSLCLIPLoss(use_vissl=True, rank=rank, world_size=world)
        crit._slab_forward, crit._slab_backward = ssl_fwd, ssl_bwd
    else:
        crit = (L.AdaptiveMaxMarginRankingLoss if case == 'adaptive' else L.MaxMarginRankingLoss)()
        crit._slab_prepare, crit._slab_forward, crit._slab_backward = margin_prepare, margin_fwd, margin_bwd
    return crit


def record_all(rank, world):
    """{(case, dtype name): (forward gathers, backward gathers)} of this process, each a list of (shape, dtype)."""
    calls = []
    real = dist.all_gather_into_tensor

    def recorder(output, input, *a, **k):
        calls.append((tuple(input.shape), str(input.dtype)))
        return real(output, input, *a, **k)

    dist.all_gather_into_tensor = recorder
    res = {}
    try:
        for case in CASES:
            for name, (idt, tdt, _) in DTYPES.items():
                g = torch.Generator().manual_seed(7 + rank)
                img = torch.randn(B, E, generator=g).to(idt).requires_grad_(True)
                txt = torch.randn(B, E, generator=g).to(tdt).requires_grad_(True)
                outputs = {'image_embed': img, 'text_embed': txt, 'logit_scale': torch.tensor(10.0, requires_grad=True)}
                crit = _criterion(case, rank, world)
                del calls[:]
                if case == 'ssl':
                    out = crit(outputs, torch.tensor([1, 0, 1]))
                elif case == 'adaptive':
                    out = crit(outputs, torch.rand(B, generator=g))
                else:
                    out = crit(outputs)
                fwd = list(calls)
                del calls[:]
                out['loss'].backward()
                assert img.grad.dtype == idt and txt.grad.dtype == tdt
                res[(case, name)] = (fwd, list(calls))
    finally:
        dist.all_gather_into_tensor = real
    return res


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    q.put((rank, record_all(rank, world)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope='module')
def two_ranks():
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, 29883, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
    return [res for _, res in got]


@pytest.mark.parametrize('name', list(DTYPES))
@pytest.mark.parametrize('case', CASES)
def test_two_ranks_gather_what_the_plan_says(two_ranks, case, name):
    for rank, res in enumerate(two_ranks):
        fwd, bwd = res[(case, name)]
        print(f'rank {rank} {case} {name}: forward {fwd} backward {bwd}')
        assert fwd == expected(case, DTYPES[name][2])
        assert bwd == []


def test_one_rank_gathers_nothing():
    for key, (fwd, bwd) in record_all(0, 1).items():
        assert fwd == [] and bwd == [], key
