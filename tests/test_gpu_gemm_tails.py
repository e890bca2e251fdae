"""GPU (-m gpu): the persistent TN GEMM (lvl_linear_tn) and the weight-gradient GEMM (lvl_linear_wgrad) on TAIL tiles
(M % 256 != 0), with few compute units and on every tile schedule.

  * a store-count audit of the counted vmcnt waits (csrc/gemm_tn_mfma.hip built with -DGM_AUDIT): the K loop never drains
    at a tile boundary, and the first blocks after an epilogue wait with an allowance for the epilogue's result stores
    still in flight. That is only sound if every wave issued at least that many stores -- which a wave of a tail tile
    whose row groups lie behind M does not. An output comparison cannot see a wrong wait (the unawaited fills have
    usually landed); the audit counts the stores at their issue sites and checks them against the allowance used;
  * a correctness matrix: row remainders at every boundary of the four 32-row groups x two wave halves of a 256-row
    tile, 8 / 16 / all compute units, static / dynamic / dynamic-with-late-workgroups schedules, against float64 and
    exactly on small integers; outputs bit-equal across CU counts and schedules (a tile's arithmetic does not depend on
    who computes it); rows >= M of the outputs never written, rows >= M of the inputs never read.
"""
import pytest
import torch

from gemm_tn_cases import CONFIGS, DEV, LATE_MOD, TN_KERNELS, audit_records, build_audit_library
from gemm_tn_cases import check_integers as _check_integers
from gemm_tn_cases import check_random_vs_float64 as _check_random_vs_float64
from gemm_tn_cases import case_data, int_data
from gemm_tn_cases import ns as _ns
from gemm_tn_cases import rows as _rows
from gemm_tn_cases import same as _same
from gemm_tn_cases import tn as _tn
from helpers import launch_config as _launch_config
from helpers import wgrad_launch as _wgrad

pytestmark = pytest.mark.gpu

# row remainders mod 256: both sides of every 32-row group boundary (a 256-row tile = 2 halves (qm) x 2 waves (wm) x
# 2 groups of 32 rows), one-row and all-but-one-row tails, and the remainder-0 control
REMAINDERS = (0, 1, 31, 32, 33, 64, 65, 96, 127, 128, 129, 192, 224, 255)
# (N, tile rows): at 8 CUs (one workgroup per XCD) XCD 7 walks the whole last tile row, so tail tiles run back to back
# in one workgroup (N = 768: 8 x 3 tiles, 3 per XCD; N = 3072: 4 x 12 tiles, 6 per XCD)
SHAPES = ((768, 8), (3072, 4))
K_BF16 = 320          # 5 K blocks: the fewest the dynamic schedule takes (DYN_MIN_NB)
K_F32 = 128           # f32-class mode: K' = 3 x 128 = 384 (6 K blocks)
# the launch and check helpers, the kernel table (TN_KERNELS), the configurations (CONFIGS: 8 / 16 / all CUs x static /
# dynamic / late) and the GM_AUDIT build live in gemm_tn_cases.py, shared with the K-axis matrix (test_gpu_gemm_kblocks.py)


def _case_data(N, rem):
    """random operands of one (N, remainder) case"""
    return case_data(N, _rows(dict(SHAPES)[N], rem), 1000 * N + rem, K_BF16, K_F32)


def _int_data(N, rem):
    return int_data(N, _rows(dict(SHAPES)[N], rem), 7 * N + rem, K_BF16, K_F32)


@pytest.mark.parametrize('N,rem', [(n, r) for n, _ in SHAPES for r in REMAINDERS])
def test_linear_tn_tail_tiles_vs_float64_on_every_schedule(N, rem):
    """every epilogue of lvl_linear_tn (bf16 0 with and without bias, 1-5; f32-class 0-3) at one row remainder: float64
    bounds on random data, exact on small integers, then bit-equal under 8 / 16 / all CUs x static / dynamic / late
    schedules with NaN/Inf rows behind the inputs and sentinel rows behind the outputs (never read / never written),
    NaN-poisoned column-sum outputs and workspace, and the tile-counter block zero again afterwards"""
    from lavila_amd import _cabi as C
    lib = C.lib()
    d = _case_data(N, rem)
    di = _int_data(N, rem)
    base = {}
    for kern in TN_KERNELS:
        base[kern[0]] = _tn(lib, kern, d, 'static', guard=False)
        _check_random_vs_float64(kern, base[kern[0]], d)
        if kern[1] != 2 and kern[1] != 4:
            _check_integers(kern, _tn(lib, kern, di, 'static', guard=True), di)
    for cus, sched in CONFIGS:
        with _launch_config([lib], cus, LATE_MOD if sched == 'late' else 0):
            for kern in TN_KERNELS:
                got = _tn(lib, kern, d, sched, guard=True)
                assert _same(got, base[kern[0]]), (kern[0], cus, sched)


# --------------------------------------------------------------------------------------------------------------------
# store-count audit of the counted waits (GM_AUDIT build)
# --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def audit_lib(tmp_path_factory):
    return build_audit_library(tmp_path_factory.mktemp('gm_audit'))


@pytest.mark.parametrize('N', [n for n, _ in SHAPES])
def test_counted_waits_never_exceed_the_stores_issued(audit_lib, N):
    """GM_AUDIT: for every wave and tile boundary, the vmcnt allowance the next tile's first K blocks use (`slack`)
    is at most the number of vector-memory stores that wave issued in the finished tile's epilogue (`issued`, counted
    at the issue sites) -- over the whole remainder x CU-count x schedule matrix. Non-vacuity: for every epilogue and
    both schedule kinds some record is a tail tile followed by another tile of the same workgroup in which a wave
    issued fewer stores than the full-tile allowance; full tiles issue exactly the expected count. The audit build
    computes what the product library computes, bit for bit."""
    from lavila_amd import _cabi as C
    lib = C.lib()
    seen = {}                     # (kernel, static?) -> tail records with fewer stores than the allowance
    bad = []
    for rem in REMAINDERS:
        d = _case_data(N, rem)
        M = d['M']
        tiles_m = (M + 255) // 256
        want = {kern[0]: _tn(lib, kern, d, 'static', guard=False) for kern in TN_KERNELS}
        for cus, sched in CONFIGS:
            for kern in TN_KERNELS:
                out, r = audit_records(audit_lib, kern, d, cus, sched)
                assert _same(out, {k: v for k, v in want[kern[0]].items() if k != 'colsum'}), (kern[0], rem, cus, sched)
                ns, full = _ns(kern)
                tail = (r[:, 0] + 1) * 256 > M
                assert bool((r[:, 0] < tiles_m).all()) and bool((r[:, 1] < N // 256).all())
                assert bool((r[~tail, 2] == full).all()), (kern[0], rem, cus, sched, 'full-tile store count')
                assert bool((r[~tail, 3] == ns).all())
                viol = int((r[:, 3] > r[:, 2]).sum())
                if viol:
                    bad.append((kern[0], M, cus, sched, viol, len(r)))
                key = (kern[0], sched == 'static')
                seen[key] = seen.get(key, 0) + int((tail & (r[:, 2] < ns)).sum())
    assert not bad, f'records with slack > issued (kernel, M, cus, schedule, violating, records): {bad}'
    for kern in TN_KERNELS:
        if _ns(kern)[0] > 0:
            for static in (True, False):
                assert seen[(kern[0], static)] > 0, (kern[0], static, 'no back-to-back tail tile with fewer stores')


@pytest.mark.parametrize('epi', [0, 1, 2, 3, 4, 5])
def test_counted_waits_of_the_few_cu_shape(audit_lib, epi):
    """the shape of test_persistent_gemms_exact_with_fewer_compute_units at 8 CUs (M = 9000: remainder 40, N = 768):
    XCD 7's single workgroup runs the last tile row back to back; every epilogue, static and dynamic schedule"""
    from lavila_amd import _cabi as C
    kern = next(k for k in TN_KERNELS if k[1] == epi and not k[2])
    M, N, K = 9000, 768, 768
    g = torch.Generator(device=DEV).manual_seed(9000 + epi)
    d = {'M': M, 'x': torch.randn(M, K, device=DEV, generator=g).bfloat16(),
         'w': (torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).bfloat16(),
         'b': torch.randn(N, device=DEV, generator=g)}
    for k in 'urd':
        d[k] = torch.randn(M, N, device=DEV, generator=g).bfloat16()
    want = _tn(C.lib(), kern, d, 'static', guard=False)
    ns, _ = _ns(kern)
    for sched in ('static', 'dynamic'):
        out, r = audit_records(audit_lib, kern, d, 8, sched)
        assert _same(out, {k: v for k, v in want.items() if k != 'colsum'}), sched
        tail = (r[:, 0] + 1) * 256 > M
        assert int((tail & (r[:, 2] < ns)).sum()) > 0, sched
        viol = int((r[:, 3] > r[:, 2]).sum())
        assert viol == 0, f'epilogue {epi}, {sched}: {viol} of {len(r)} records with slack > issued'


# --------------------------------------------------------------------------------------------------------------------
# lvl_linear_wgrad on the same remainders (the launch harness: helpers.wgrad_launch)
# --------------------------------------------------------------------------------------------------------------------
def test_linear_wgrad_tail_rows_on_every_schedule():
    """lvl_linear_wgrad (dW = dy^T x, with and without dbias) at every remainder of the matrix, 8 / 16 / all CUs x
    static / dynamic / late: rows >= M of dy and x are NaN/Inf and never read; exact on small integers under every
    configuration, within the f32 summation bound of float64 on random data (the row splits, and with them the
    summation order, follow the CU count)"""
    from lavila_amd import _cabi as C
    lib = C.lib()
    N, K = 768, 768
    for rem in REMAINDERS:
        M = 256 * 40 + rem
        g = torch.Generator(device=DEV).manual_seed(rem)
        dy = torch.randn(M, N, device=DEV, generator=g).bfloat16()
        x = torch.randn(M, K, device=DEV, generator=g).bfloat16()
        dyi = (torch.randint(-2, 3, (M, N), device=DEV, generator=g) * (torch.rand(M, N, device=DEV, generator=g) < 0.05)).bfloat16()
        xi = torch.randint(-2, 3, (M, K), device=DEV, generator=g).bfloat16()
        ref = dy.double().t() @ x.double()
        bound = 2.0 ** -12 * (dy.double().abs().t() @ x.double().abs()) + 1e-6
        refb = dy.double().sum(0)
        boundb = 2.0 ** -12 * dy.double().abs().sum(0) + 1e-6
        wanti = dyi.double().t() @ xi.double()
        for cus, sched in CONFIGS:
            with _launch_config([lib], cus, LATE_MOD if sched == 'late' else 0):
                for want_db in (False, True):
                    dw, db = _wgrad(lib, dy, x, want_db, sched, guard=True)
                    assert ((dw.double() - ref).abs() <= bound).all(), (rem, cus, sched, want_db)
                    if want_db:
                        assert ((db.double() - refb).abs() <= boundb).all(), (rem, cus, sched)
                    dw, db = _wgrad(lib, dyi, xi, want_db, sched, guard=True)
                    assert torch.equal(dw.double(), wanti), (rem, cus, sched, want_db)
                    if want_db:
                        assert torch.equal(db.double(), dyi.double().sum(0)), (rem, cus, sched)
