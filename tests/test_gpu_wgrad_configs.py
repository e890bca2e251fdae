"""GPU (-m gpu): every tile configuration of lvl_linear_wgrad (13 instantiations of csrc/wgrad_kernel.h, each with and
without dbias) on every schedule. The rows of wgrad_cases.CASES -- per configuration a one-chunk plan at the device's CU
count and a multi-split, multi-chunk plan at 8 CUs (test_wgrad_plan_cpu.py: each reaches the configuration it names) --
run static, dynamic and with late workgroups (the tile-mates take the late workgroup's chunks across chunk boundaries),
with and without dbias, at row counts M, M + 1 and M + 31:

  * small-integer operands (dy sparse in -2..2, x in -2..2: every sum far below 2^24): dW and dbias equal the float64
    result bit for bit on every schedule, a second launch on the same counter block included;
  * random bf16 operands against float64 of the same rounded operands, within the bound of
    test_gpu_gemm_tails.py::test_linear_wgrad_tail_rows_on_every_schedule (2^-12 |dy|^T |x| + 1e-6; dbias: 2^-12 sum |dy| +
    1e-6); two static launches bit-identical. No bit equality between schedules on random data: a workgroup that
    finishes early may take a tile-mate's chunk and the f32 summation order then follows the timing (csrc/wgrad_mfma.hip);
  * guards on every launch: rows >= M of dy and x are NaN / Inf, dW / dbias / the workspace start as NaN, the floats
    behind lvl_workspace_floats come back untouched, the counter block is zero again after the launch.
"""
import pytest
import torch

import wgrad_cases as W
from helpers import launch_config, sched_block, wgrad_launch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
WS_GUARD = 4096


def _lib():
    from lavila_amd import _cabi as C
    return C.lib()


def _schedules(lib, p):
    """(name, schedule, late_mod) of a plan: static, dynamic, and dynamic with each late setting the plan allows"""
    return [('static', 'static', 0), ('dynamic', 'dynamic', 0)] + \
        [(f'late{m}', 'late', m) for m in W.late_mods(lib, p)]


def _integers(M, N, K, g):
    dy = (torch.randint(-2, 3, (M, N), device=DEV, generator=g) * (torch.rand(M, N, device=DEV, generator=g) < 0.05)).bfloat16()
    x = torch.randint(-2, 3, (M, K), device=DEV, generator=g).bfloat16()
    return dy, x


def _run_case(lib, c, p):
    """one table row: every remainder x schedule x dbias, integers and random data"""
    ran = set()
    for rem in W.REMAINDERS:
        M = c.M + rem
        g = torch.Generator(device=DEV).manual_seed(1000 * c.cfg + rem)
        dyi, xi = _integers(M, c.N, c.K, g)
        wanti, wantbi = dyi.double().t() @ xi.double(), dyi.double().sum(0)
        assert float(wanti.abs().max()) > 0 and float(dyi.double().abs().t().matmul(xi.double().abs()).max()) < 2 ** 24
        dy = torch.randn(M, c.N, device=DEV, generator=g).bfloat16()
        x = torch.randn(M, c.K, device=DEV, generator=g).bfloat16()
        ref = dy.double().t() @ x.double()
        bound = 2.0 ** -12 * (dy.double().abs().t() @ x.double().abs()) + 1e-6
        refb = dy.double().sum(0)
        boundb = 2.0 ** -12 * dy.double().abs().sum(0) + 1e-6
        for name, sched, late in _schedules(lib, p):
            with launch_config([lib], c.cus, late):
                assert W.plan(lib, M, c.N, c.K) == p, (c, M)
                for want_db in (False, True):
                    key = (W.case_id(c), M, name, want_db)
                    blk = sched_block(sched, W.COUNTER_WORDS)
                    dw, db = wgrad_launch(lib, dyi, xi, want_db, sched, guard=True, blk=blk, ws_guard=WS_GUARD)
                    assert torch.equal(dw.double(), wanti), key
                    if want_db:
                        assert torch.equal(db.double(), wantbi), key
                    if blk is not None:       # the launch left its counters at zero: the same block serves the next one
                        dw2, db2 = wgrad_launch(lib, dyi, xi, want_db, sched, guard=True, blk=blk, ws_guard=WS_GUARD)
                        assert torch.equal(dw2.double(), wanti), key
                        if want_db:
                            assert torch.equal(db2.double(), wantbi), key
                    dw, db = wgrad_launch(lib, dy, x, want_db, sched, guard=True, ws_guard=WS_GUARD)
                    assert ((dw.double() - ref).abs() <= bound).all(), key
                    if want_db:
                        assert ((db.double() - refb).abs() <= boundb).all(), key
                    if sched == 'static':
                        dw2, db2 = wgrad_launch(lib, dy, x, want_db, sched, guard=True, ws_guard=WS_GUARD)
                        assert torch.equal(dw2, dw) and (not want_db or torch.equal(db2, db)), key
                    ran.add(name)
    return ran


@pytest.mark.parametrize('cfg', range(len(W.CFGS)))
def test_wgrad_configuration_on_every_schedule(cfg):
    lib = _lib()
    rows = [c for c in W.CASES if c.cfg == cfg]
    assert {c.kind for c in rows} == {'one', 'multi'}
    late = set()
    for c in rows:
        with W.compute_units(lib, c.cus):
            p = W.plan(lib, c.M, c.N, c.K)
        assert p is not None and p['cfg'] == cfg, (c, p)
        assert (W.chunks(p) == 1) if c.kind == 'one' else (p['S'] >= 2 and W.chunks(p) >= 3), (c, p)
        ran = _run_case(lib, c, p)
        assert {'static', 'dynamic'} <= ran
        if c.kind == 'multi':
            late |= ran
    assert 'late1024' in late, late          # the multi-split rows always run with block 1 late


# (N, K, M, compute units): the decoder's and the towers' own widths, one launch per schedule, integers only
REAL_SHAPES = ((4800, 1600, 3103, 0),        # 150 tiles of 320 x 160 at S = 1: 150 pairs, not a multiple of 8
               (6400, 1600, 9216, 0),        # cfg 11 (256 x 320 tiles), S = 2, 3 chunks per unit
               (1024, 4096, 25000, 0))       # cfg 5 on all compute units


@pytest.mark.parametrize('N,K,M,cus', REAL_SHAPES)
def test_wgrad_real_shapes_exact_on_integers(N, K, M, cus):
    lib = _lib()
    with W.compute_units(lib, cus):
        p = W.plan(lib, M, N, K)
    assert p is not None
    if (N, K) == (4800, 1600):
        assert (p['cfg'], p['ntiles'] * p['S']) == (8, 150), p
    if (N, K) == (6400, 1600):
        assert (p['cfg'], p['S'], W.chunks(p)) == (11, 2, 3), p
    if (N, K) == (1024, 4096):
        assert p['cfg'] == 5 and p['ntiles'] * p['S'] > 128, p
    g = torch.Generator(device=DEV).manual_seed(N + K)
    dyi, xi = _integers(M, N, K, g)
    wanti, wantbi = dyi.double().t() @ xi.double(), dyi.double().sum(0)
    for name, sched, late in _schedules(lib, p):
        with launch_config([lib], cus, late):
            want_db = name == 'static'       # dbias rides on the static plan only (the dbias instantiations never claim)
            dw, db = wgrad_launch(lib, dyi, xi, want_db, sched, guard=True, ws_guard=WS_GUARD)
            assert torch.equal(dw.double(), wanti), (N, K, M, name)
            if want_db:
                assert torch.equal(db.double(), wantbi), (N, K, M, name)
