"""GPU (-m gpu): the exact-GELU epilogues of lvl_linear_tn -- 6 LVL_EPI_BIAS_GELU, 7 LVL_EPI_GELU_BWD (bf16 and f32-class),
8 LVL_EPI_BIAS_GELU_DERIV (bf16) -- through the C ABI.

Shapes (M, N, K): (300, 512, 192) one full and one 44-row tail tile, two column tiles, 3 K blocks (static schedule, and with a
counter block); (1, 256, 64) one row, one K block; (513, 256, 128). Outputs sit in sentinel-guarded buffers, inputs in
NaN/Inf-padded ones.

  * EXACT-u operands (gelu_tn_cases.exact_u_data: u = k / 8, |u| <= 7, exact in bf16 and in the f32 accumulation): what the
    epilogues write equals, BIT FOR BIT, what lvl_act_fwd / lvl_act_bwd (LVL_ACT_GELU_ERF) compute from the same numbers --
    the one definition in csrc/gelu_erf.h. Epilogue 6: aux_out == u, y == lvl_act_fwd(aux_out). Epilogue 8: y == epilogue 6's
    y (the rounded u IS u here), aux_out == lvl_act_bwd(u, 1). Epilogue 7: y == lvl_act_bwd(aux_in, acc) evaluated in float32
    (bf16: rounded once), the column sums at the bars gemm_tn_cases.check_random_vs_float64 holds epilogue 2 to, and
    unchanged when the rows behind M of the inputs go from zeros to NaN / Inf.
  * the same outputs against float64: |delta| <= 2^-8 |ref| + 2^-18 for y of 6 and 8 and aux_out of 8. The absolute term
    covers the float32 cancellation of 1 + erf below u = -4, where a float32 and a float64 evaluation round to different
    bf16 values (26 of the 129 grid points k / 8 on the CPU) -- an ulp count would be the wrong bar. A float32 evaluation of
    the same expressions on the CPU stays within 2^-8 |ref| + 2^-20 on this grid (worst ratios 0.84 and 0.93): the device's
    erff has a factor of 4.
  * random operands (gemm_tn_cases.case_data) at the float64 bars of the QuickGELU twins 1, 2 and 4.
  * refusals: epilogue 8 in f32-class mode, epilogues 6-8 on the ragged entry.
  * the store-count audit (GM_AUDIT build of csrc/gemm_tn_gelu.hip, as tests/test_gpu_gemm_tails.py's of gemm_tn_mfma.hip): the vmcnt allowance behind an epilogue never
    exceeds the stores the wave issued. (300, 512, 192) has four tiles and a launch at least eight workgroups' room: every
    workgroup runs ONE tile and writes no record (a record belongs to a tile boundary), so that shape is run for its outputs
    and the same N, K with 2092 rows (eight full tile rows and the 44-row tail, 18 tiles on 8 compute units) gives the
    records, non-zero allowances among them."""
import pytest
import torch

import gelu_tn_cases as G
from gemm_tn_cases import DEV, case_data
from gemm_tn_cases import same as _same

pytestmark = pytest.mark.gpu

KERN = {k[0]: k for k in G.GELU_KERNELS}


def _configs(shape):
    return ('static', 'dynamic') if shape == G.SHAPES[0] else ('static',)


def _within(name, got, ref, rel, ab):
    err, bound = (got.double() - ref).abs(), rel * ref.abs() + ab
    worst = (err / bound).max().item()
    print(f'[gelu epilogues] {name}: worst |delta| / (2^{torch.log2(torch.tensor(rel)).item():.0f} |ref| + '
          f'2^{torch.log2(torch.tensor(ab)).item():.0f}) = {worst:.3f}')
    assert bool((err <= bound).all()), (name, worst)


@pytest.mark.parametrize('shape', G.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_forward_epilogues_share_the_bits_of_lvl_act(shape):
    from lavila_amd import _cabi as C
    lib = C.lib()
    M, N, K = shape
    d = G.exact_u_data(M, N, K, seed=M + N + K)
    u64 = d['u64']
    for sched in _configs(shape):
        o6 = G.tn(lib, KERN['gelu'], d, sched, guard=True)
        o8 = G.tn(lib, KERN['gelu_deriv'], d, sched, guard=True)
        f6 = G.tn(lib, KERN['f32_gelu'], d, sched, guard=True)
        # epilogue 6, bf16: the kept pre-activation is u, and y is what lvl_act_fwd rebuilds from it
        assert torch.equal(o6['aux_out'].double(), u64), sched
        up, _ = G.pad8(o6['aux_out'])
        assert torch.equal(o6['y'], G.act_fwd(up)[:M]), (sched, 'bf16 epilogue 6: y != lvl_act_fwd(aux_out)')
        # ... f32-class: float32 u and y, unrounded
        assert f6['aux_out'].dtype == torch.float32 and torch.equal(f6['aux_out'].double(), u64), sched
        fp, _ = G.pad8(f6['aux_out'])
        assert torch.equal(f6['y'], G.act_fwd(fp)[:M]), (sched, 'f32-class epilogue 6: y != lvl_act_fwd(aux_out)')
        # epilogue 8: the unrounded u equals the rounded one on these operands
        assert torch.equal(o8['y'], o6['y']), (sched, 'epilogue 8: y != epilogue 6\'s y')
        assert torch.equal(o8['aux_out'], G.act_bwd(up, torch.ones_like(up))[:M]), (sched, 'epilogue 8: aux_out != lvl_act_bwd(u, 1)')
        # against float64
        _within(f'{shape} {sched} epilogue 6 y', o6['y'], G.gelu64(u64), 2.0 ** -8, 2.0 ** -18)
        _within(f'{shape} {sched} epilogue 8 y', o8['y'], G.gelu64(u64), 2.0 ** -8, 2.0 ** -18)
        _within(f'{shape} {sched} epilogue 8 aux_out', o8['aux_out'], G.gelu_grad64(u64), 2.0 ** -8, 2.0 ** -18)
        assert float(o8['aux_out'].float().min()) >= -0.13 and float(o8['aux_out'].float().max()) <= 1.13
    if M > 1:
        assert float(u64.min()) < -4 and float(u64.max()) > 4          # the grid reaches the cancellation range


@pytest.mark.parametrize('shape', G.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_backward_epilogue_shares_the_bits_of_lvl_act_bwd(shape):
    from lavila_amd import _cabi as C
    lib = C.lib()
    M, N, K = shape
    d = G.exact_u_data(M, N, K, seed=2 * (M + N + K))
    acc = d['acc']
    accp, _ = G.pad8(acc.float())
    for sched in _configs(shape):
        o7 = G.tn(lib, KERN['gelu_bwd'], d, sched, guard=True)
        f7 = G.tn(lib, KERN['f32_gelu_bwd'], d, sched, guard=True)
        # bf16: acc * gelu'(aux_in) in float32, rounded once
        ub, _ = G.pad8(d['u'].float())
        want = G.act_bwd(ub, accp)[:M]
        assert torch.equal(o7['y'], want.bfloat16()), (sched, 'bf16 epilogue 7: y != bf16(lvl_act_bwd(aux_in, acc) in f32)')
        uf, _ = G.pad8(d['f32_u'])
        wantf = G.act_bwd(uf, accp)[:M]
        assert torch.equal(f7['y'], wantf), (sched, 'f32-class epilogue 7: y != lvl_act_bwd(aux_in, acc)')
        # column sums against float64, as check_random_vs_float64 holds epilogue 2
        xd, wd = d['x'].double(), d['w'].double()
        eps = 2.0 ** -14 * (xd.abs() @ wd.abs().t()) + 1e-6
        G.check_bwd_vs_float64('gelu_bwd', o7, acc, G.gelu_grad64(d['u'].double()), eps)
        ref = acc * G.gelu_grad64(d['f32_u'].double())
        torch.testing.assert_close(f7['colsum'].double(), ref.sum(0), atol=1e-3 * M ** 0.5, rtol=1e-4)
        assert torch.isfinite(o7['colsum']).all() and torch.isfinite(f7['colsum']).all()
        # rows behind M stay out of the sums: zeros there or NaN / Inf, the same bits
        for kern, got in ((KERN['gelu_bwd'], o7), (KERN['f32_gelu_bwd'], f7)):
            zero = G.tn(lib, kern, d, sched, guard=True, pad='zero')
            assert torch.equal(zero['colsum'], got['colsum']) and torch.equal(zero['y'], got['y']), (kern[0], sched)


@pytest.mark.parametrize('shape', G.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_random_operands_vs_float64(shape):
    from lavila_amd import _cabi as C
    lib = C.lib()
    M, N, K = shape
    d = case_data(N, M, 31 * M + N + K, K, K)
    for kern in G.GELU_KERNELS:
        base = G.tn(lib, kern, d, 'static', guard=False)
        G.check_random_vs_float64(kern, base, d)
        for sched in _configs(shape):
            assert _same(G.tn(lib, kern, d, sched, guard=True), base), (kern[0], sched)


def test_refusals():
    from lavila_amd import _cabi as C
    lib = C.lib()
    M, N, K = 256, 256, 64
    x3 = torch.zeros(M, 3 * K, dtype=torch.bfloat16, device=DEV)
    w3 = torch.zeros(N, 3 * K, dtype=torch.bfloat16, device=DEV)
    b = torch.zeros(N, device=DEV)
    y, a = (torch.zeros(M, N, device=DEV) for _ in range(2))
    rc = lib.lvl_linear_tn(C.ptr(x3), C.ptr(w3), C.ptr(b), C.ptr(y), C.ptr(a), None, None, None, None, M, N, 3 * K,
                           C.EPI_BIAS_GELU_DERIV, C.LVL_F32, C.stream_ptr())
    assert rc == -38 and 'bf16 epilogue' in lib.lvl_last_error().decode()            # LVL_ENOSYS, as epilogues 4 and 5
    for epi in (C.EPI_BIAS_QUICKGELU_DERIV, C.EPI_MUL_AUX_COLSUM):
        assert lib.lvl_linear_tn(C.ptr(x3), C.ptr(w3), C.ptr(b), C.ptr(y), C.ptr(a), C.ptr(a), C.ptr(b), C.ptr(y), None, M, N,
                                 3 * K, epi, C.LVL_F32, C.stream_ptr()) == -38
    assert lib.lvl_linear_tn(C.ptr(x3), C.ptr(w3), C.ptr(b), C.ptr(y), C.ptr(a), None, None, None, None, M, N, 3 * K, 9,
                             C.LVL_F32, C.stream_ptr()) == -22                       # LVL_EINVAL: unknown
    xb, yb = x3[:, :K].contiguous(), torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    wb = w3[:, :K].contiguous()
    for epi in (C.EPI_BIAS_GELU, C.EPI_GELU_BWD, C.EPI_BIAS_GELU_DERIV):
        rc = lib.lvl_linear_tn_ragged(C.ptr(xb), C.ptr(wb), C.ptr(b), C.ptr(yb), None, M, N, K, epi, C.LVL_BF16, C.stream_ptr())
        assert rc == -38 and 'LVL_EPI_BIAS only' in lib.lvl_last_error().decode(), epi
    rc = lib.lvl_linear_tn_ragged(C.ptr(xb), C.ptr(wb), C.ptr(b), C.ptr(yb), None, M, N, K, 9, C.LVL_BF16, C.stream_ptr())
    assert rc == -22 and 'unknown epilogue' in lib.lvl_last_error().decode()
    # the bf16 entry wants aux_out for 6 and 8, aux_in + colsum + workspace for 7
    for epi in (C.EPI_BIAS_GELU, C.EPI_GELU_BWD, C.EPI_BIAS_GELU_DERIV):
        assert lib.lvl_linear_tn(C.ptr(xb), C.ptr(wb), C.ptr(b), C.ptr(yb), None, None, None, None, None, M, N, K, epi,
                                 C.LVL_BF16, C.stream_ptr()) == -22
    torch.cuda.synchronize()


@pytest.fixture(scope='module')
def audit_lib(tmp_path_factory):
    return G.build_audit_library(tmp_path_factory.mktemp('gm_audit_gelu'))


def test_counted_waits_never_exceed_the_stores_issued(audit_lib):
    from lavila_amd import _cabi as C
    lib = C.lib()
    M0, N, K = G.SHAPES[0]
    allowances = 0
    for M in (M0, 256 * 8 + 44):
        d = case_data(N, M, 77 + M, K, K)
        for kern in G.GELU_KERNELS:
            want = G.tn(lib, kern, d, 'static', guard=False)
            for sched in ('static', 'dynamic'):
                out, r, _ = G.audit_records(audit_lib, kern, d, 8, sched)
                assert _same(out, {k: v for k, v in want.items() if k != 'colsum'}), (kern[0], M, sched)
                nsk, full = G.ns(kern)
                tail = (r[:, 0] + 1) * 256 > M
                assert bool((r[~tail, 2] == full).all()), (kern[0], M, sched, 'full-tile store count')
                assert bool((r[~tail, 3] == nsk).all()) and bool((r[tail, 3] == 0).all())
                viol = int((r[:, 3] > r[:, 2]).sum())
                assert viol == 0, f'{kern[0]}, M = {M}, {sched}: {viol} of {len(r)} records with slack > issued'
                if M != M0:
                    assert len(r) > 0 and bool(tail.any()), (kern[0], sched)
                    if nsk:
                        assert int((r[:, 3] > 0).sum()) > 0, (kern[0], sched, 'no record with a non-zero allowance')
                allowances += int((r[:, 3] > 0).sum())
    assert allowances > 0
