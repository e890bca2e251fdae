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
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

from helpers import guarded_in as _guarded_in
from helpers import launch_config as _launch_config
from helpers import sched_block as _sched_block
from helpers import wgrad_launch as _wgrad

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# row remainders mod 256: both sides of every 32-row group boundary (a 256-row tile = 2 halves (qm) x 2 waves (wm) x
# 2 groups of 32 rows), one-row and all-but-one-row tails, and the remainder-0 control
REMAINDERS = (0, 1, 31, 32, 33, 64, 65, 96, 127, 128, 129, 192, 224, 255)
# (N, tile rows): at 8 CUs (one workgroup per XCD) XCD 7 walks the whole last tile row, so tail tiles run back to back
# in one workgroup (N = 768: 8 x 3 tiles, 3 per XCD; N = 3072: 4 x 12 tiles, 6 per XCD)
SHAPES = ((768, 8), (3072, 4))
K_BF16 = 320          # 5 K blocks: the fewest the dynamic schedule takes (DYN_MIN_NB)
K_F32 = 128           # f32-class mode: K' = 3 x 128 = 384 (6 K blocks)
# (compute units (0 = the device's), schedule). No late workgroups at 8 CUs: there the hook would leave an XCD's single
# workgroup idle for the whole launch and nobody would serve that XCD's tile queue (test_gpu_parity_bf16.py)
CONFIGS = tuple((cus, sched) for cus in (8, 16, 0) for sched in ('static', 'dynamic', 'late')
                if not (cus == 8 and sched == 'late'))
LATE_MOD = 3
SENT16, SENT32 = 0x7FA5, 0x7FA5A5A5     # sentinel bit patterns of the output guard rows (NaN payloads nobody writes)


def _rows(tiles, rem):
    return 256 * (tiles - 1) + rem if rem else 256 * tiles


def _qg(u):
    return u * torch.sigmoid(1.702 * u)


def _qg_grad(u):
    s = torch.sigmoid(1.702 * u)
    return s * (1 + 1.702 * u * (1 - s))


def _guarded_out(M, N, dtype):
    """an (M + 256)-row output buffer pre-filled with the sentinel bit pattern"""
    buf = torch.empty(M + 256, N, dtype=dtype, device=DEV)
    if dtype == torch.bfloat16:
        buf.view(torch.int16).fill_(SENT16)
    else:
        buf.view(torch.int32).fill_(SENT32)
    return buf


def _untouched(buf, M):
    if buf.dtype == torch.bfloat16:
        return bool((buf[M:].view(torch.int16) == SENT16).all())
    return bool((buf[M:].view(torch.int32) == SENT32).all())


# the kernels of the matrix: (name, epilogue, f32-class, with bias, aux_in)
TN_KERNELS = (('bias', 0, False, True, None), ('nobias', 0, False, False, None), ('gelu', 1, False, True, None),
              ('gelu_bwd', 2, False, False, 'u'), ('residual', 3, False, True, 'r'), ('gelu_deriv', 4, False, True, None),
              ('mul_aux', 5, False, False, 'd'),
              ('f32_bias', 0, True, True, None), ('f32_gelu', 1, True, True, None), ('f32_gelu_bwd', 2, True, False, 'u'),
              ('f32_residual', 3, True, True, 'r'))


def _tn(lib, kern, data, sched, guard, audit=None):
    """one lvl_linear_tn launch (or lvl_linear_tn_audit with `audit`, the record buffer) -> dict of outputs. guard: the
    inputs are the first M rows of NaN/Inf-padded buffers, the outputs of sentinel-filled ones (checked here), and the
    column-sum outputs start as NaN."""
    from lavila_amd import _cabi as C
    name, epi, f32, with_bias, aux = kern
    x, w = (data['x3'], data['w3']) if f32 else (data['x'], data['w'])
    bias = data['b'] if with_bias else None
    aux_in = data[('f32_' if f32 else '') + aux] if aux else None
    M, K = x.shape
    N = w.shape[0]
    odt = torch.float32 if f32 else torch.bfloat16
    if guard:
        x = _guarded_in(x)
        aux_in = _guarded_in(aux_in) if aux_in is not None else None
    ybuf = _guarded_out(M, N, odt) if guard else torch.empty(M, N, dtype=odt, device=DEV)
    abuf = None
    if epi in (1, 4):
        abuf = _guarded_out(M, N, odt) if guard else torch.empty(M, N, dtype=odt, device=DEV)
    colsum = ws = None
    P = 2 * ((M + 255) // 256)
    if epi in (2, 5):
        colsum = torch.full((N,), float('nan'), device=DEV)
        ws = C.workspace('linear_tn', M, N, DEV).fill_(float('nan'))
    blk = _sched_block(sched)
    dtype = C.LVL_F32 if f32 else C.LVL_BF16
    if audit is None:
        C.check(lib.lvl_linear_tn(C.ptr(x), C.ptr(w), C.ptr(bias), C.ptr(ybuf), C.ptr(abuf), C.ptr(aux_in), C.ptr(colsum),
                                  C.ptr(ws), C.ptr(blk), M, N, K, epi, dtype, C.stream_ptr()), 'lvl_linear_tn')
    else:
        assert lib.lvl_linear_tn_audit(C.ptr(x), C.ptr(w), C.ptr(bias), C.ptr(ybuf), C.ptr(abuf), C.ptr(aux_in),
                                       C.ptr(audit), C.ptr(blk), M, N, K, epi, dtype, C.stream_ptr()) == 0
    out = {'y': ybuf[:M]}
    if abuf is not None:
        out['aux_out'] = abuf[:M]
    if epi in (2, 5):
        out['part'] = (audit if audit is not None else ws)[:P * N]
        if audit is None:
            out['colsum'] = colsum
    if guard:
        assert _untouched(ybuf, M), (name, 'y rows >= M written')
        assert abuf is None or _untouched(abuf, M), (name, 'aux_out rows >= M written')
    if blk is not None:
        torch.cuda.synchronize()
        assert int(blk.abs().sum()) == 0, (name, blk.tolist())
    return out


def _case_data(N, rem):
    """random and small-integer operands of one (N, remainder) case, device generators only"""
    from lavila_amd import ops
    M = _rows(dict(SHAPES)[N], rem)
    g = torch.Generator(device=DEV).manual_seed(1000 * N + rem)
    d = {'M': M}
    d['x'] = torch.randn(M, K_BF16, device=DEV, generator=g).bfloat16()
    d['w'] = (torch.randn(N, K_BF16, device=DEV, generator=g) * K_BF16 ** -0.5).bfloat16()
    d['b'] = torch.randn(N, device=DEV, generator=g)
    d['u'] = torch.randn(M, N, device=DEV, generator=g).bfloat16()          # pre-activation rows (epilogue 2)
    d['r'] = torch.randn(M, N, device=DEV, generator=g).bfloat16()          # residual rows (epilogue 3)
    d['d'] = (torch.rand(M, N, device=DEV, generator=g) * 1.2 - 0.1).bfloat16()     # derivative rows (epilogue 5)
    xf = torch.randn(M, K_F32, device=DEV, generator=g)
    wf = torch.randn(N, K_F32, device=DEV, generator=g) * K_F32 ** -0.5
    d['xf'], d['wf'] = xf, wf
    d['x3'], d['w3'] = ops.split3(xf, 0), ops.split3(wf, 1)
    d['f32_u'] = torch.randn(M, N, device=DEV, generator=g)
    d['f32_r'] = torch.randn(M, N, device=DEV, generator=g)
    return d


def _int_data(N, rem):
    from lavila_amd import ops
    M = _rows(dict(SHAPES)[N], rem)
    g = torch.Generator(device=DEV).manual_seed(7 * N + rem)
    ri = lambda lo, hi, shape: torch.randint(lo, hi, shape, device=DEV, generator=g).float()
    d = {'M': M}
    xi = ri(-2, 3, (M, K_BF16))
    wi = ri(-1, 2, (N, K_BF16)) * (torch.rand(N, K_BF16, device=DEV, generator=g) < 0.08)
    d['x'], d['w'], d['b'] = xi.bfloat16(), wi.bfloat16(), ri(-8, 9, (N,))
    d['r'] = ri(-8, 9, (M, N)).bfloat16()
    d['d'] = ri(-2, 3, (M, N)).bfloat16()
    d['acc'] = xi.double() @ wi.double().t()
    xf = ri(-300, 301, (M, K_F32))                 # |x| > 256: non-zero low term images
    wf = ri(-3, 4, (N, K_F32))
    d['x3'], d['w3'] = ops.split3(xf, 0), ops.split3(wf, 1)
    d['f32_r'] = ri(-1000, 1001, (M, N))
    d['f32_acc'] = xf.double() @ wf.double().t()
    return d


def _check_random_vs_float64(kern, out, d):
    """float64 reference of one kernel on the random operands: one bf16 rounding (2^-8 relative, with margin) plus the
    f32 accumulation (2^-14 |x| |w|); f32-class mode: 3 2^-17 |x| |w| (test_gpu_f32_class.py)"""
    name, epi, f32, with_bias, aux = kern
    M = d['M']
    y = out['y'].double()
    b = d['b'].double() if with_bias else 0.0
    if f32:
        xd, wd = d['xf'].double(), d['wf'].double()
        acc = xd @ wd.t()
        bound = 3 * 2.0 ** -17 * (xd.abs() @ wd.abs().t()) + 1e-6
        if epi == 0:
            assert ((y - (acc + b)).abs() <= bound).all(), name
        elif epi == 1:
            u = acc + b
            assert ((out['aux_out'].double() - u).abs() <= bound).all(), name
            assert ((y - _qg(u)).abs() <= 1.5 * bound + 2e-6 * _qg(u).abs()).all(), name
        elif epi == 3:
            ref = acc + b + d['f32_r'].double()
            assert ((y - ref).abs() <= bound + 2e-7 * ref.abs()).all(), name
        else:
            ref = acc * _qg_grad(d['f32_u'].double())
            assert ((y - ref).abs() <= 1.6 * bound + 2e-6 * ref.abs()).all(), name
            torch.testing.assert_close(out['colsum'].double(), ref.sum(0), atol=1e-3 * M ** 0.5, rtol=1e-4)
        return
    xd, wd = d['x'].double(), d['w'].double()
    acc = xd @ wd.t()
    eps = 2.0 ** -14 * (xd.abs() @ wd.abs().t()) + 1e-6
    if epi == 0 or epi == 3:
        ref = acc + b + (d['r'].double() if epi == 3 else 0.0)
        assert ((y - ref).abs() <= 2.0 ** -8 * ref.abs() + eps).all(), name
    elif epi == 1:
        u = out['aux_out'].double()
        assert ((u - (acc + b)).abs() <= 2.0 ** -8 * (acc + b).abs() + eps).all(), name
        assert ((y - _qg(u)).abs() <= 2.0 ** -8 * _qg(u).abs() + 1e-5).all(), name      # the activation sees bf16(u)
    elif epi == 4:
        u = acc + b
        assert ((y - _qg(u)).abs() <= 2.0 ** -8 * _qg(u).abs() + 1.2 * eps + 1e-5).all(), name
        dd = out['aux_out'].double()
        assert ((dd - _qg_grad(u)).abs() <= 2.0 ** -8 * _qg_grad(u).abs() + 1.2 * eps + 1e-5).all(), name
    else:
        a = _qg_grad(d['u'].double()) if epi == 2 else d['d'].double()
        ref = acc * a
        err = 1.2 * eps * a.abs() + 1e-5 * acc.abs()
        assert ((y - ref).abs() <= 2.0 ** -8 * ref.abs() + err).all(), name
        # column sums (of the unrounded f32 products): a row dropped, doubled or taken from behind M would exceed this
        cs, want = out['colsum'].double(), ref.sum(0)
        assert ((cs - want).abs() <= 2.0 ** -12 * ref.abs().sum(0) + err.sum(0) + 1e-4).all(), name
    for v in out.values():
        assert torch.isfinite(v.float()).all(), name


def _check_integers(kern, out, d):
    """small-integer operands: every product and sum is exact -> equality (column sums included)"""
    name, epi, f32, with_bias, aux = kern
    b = d['b'].double() if with_bias else 0.0
    acc = d['f32_acc' if f32 else 'acc']
    if epi == 0:
        assert torch.equal(out['y'].double(), acc + b), name
    elif epi == 1:
        assert torch.equal(out['aux_out'].double(), acc + b), name
    elif epi == 3:
        want = acc + b + d['f32_r' if f32 else 'r'].double()
        assert torch.equal(out['y'].double(), want), name
    elif epi == 5:
        want = acc * d['d'].double()
        assert want.abs().max() < 256
        assert torch.equal(out['y'].double(), want), name
        assert torch.equal(out['colsum'].double(), want.sum(0)), name       # integers < 2^24: exact in any order


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


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
def build_audit_library(out_dir):
    """gemm_tn_mfma.hip with -DGM_AUDIT plus the host stub (tools/probes/trace_stub.hip) -> a shared library"""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.fail('hipcc not found: the GM_AUDIT build of gemm_tn_mfma.hip cannot be made')
    from lavila_amd.build import EXTRA_FLAGS
    so = os.path.join(str(out_dir), 'libgemm_audit.so')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-Wl,-Bsymbolic', '-DGM_AUDIT',
                    *EXTRA_FLAGS['gemm_tn_mfma.hip'], os.path.join(ROOT, 'lavila_amd', 'csrc', 'gemm_tn_mfma.hip'),
                    os.path.join(ROOT, 'tools', 'probes', 'trace_stub.hip'), '-o', so], check=True, timeout=900)
    lib = ctypes.CDLL(so)
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.lvl_linear_tn_audit.restype = I
    lib.lvl_linear_tn_audit.argtypes = [P] * 8 + [ctypes.c_int64, I, I, I, I, P]
    for fn in ('lvl_set_compute_units', 'lvl_debug_late_workgroups'):
        getattr(lib, fn).restype = I
        getattr(lib, fn).argtypes = [I]
    lib.lvl_linear_tn_audit_cap.restype = I
    return lib


@pytest.fixture(scope='module')
def audit_lib(tmp_path_factory):
    return build_audit_library(tmp_path_factory.mktemp('gm_audit'))


def _ns(kern):
    """the vmcnt allowance of the first blocks after a full tile's epilogue, and the stores a wave issues there"""
    name, epi, f32, with_bias, aux = kern
    if f32:
        return 0, 4 * 2 * 4 * (2 if epi == 1 else 1) + (1 if epi == 2 else 0)
    return (32 if epi in (1, 4) else 16), 4 * 4 * (2 if epi in (1, 4) else 1) + (1 if epi in (2, 5) else 0)


def audit_records(alib, kern, d, cus, sched):
    """one audited launch under a launch configuration -> (outputs, records [R, 4] int64 on the CPU: tm, tn of the
    finished tile, stores the wave issued in its epilogue, allowance of the next tile's first blocks)"""
    cap = alib.lvl_linear_tn_audit_cap()
    M, N = d['M'], d['w'].shape[0]
    grid = torch.cuda.get_device_properties(0).multi_processor_count     # room for the largest grid a launch can have
    slab = 2 * ((M + 255) // 256) * N if kern[1] in (2, 5) else 0
    buf = torch.zeros(slab + grid * 8 * (1 + cap) * 4, dtype=torch.float32, device=DEV)
    with _launch_config([alib], cus, LATE_MOD if sched == 'late' else 0):
        out = _tn(alib, kern, d, sched, guard=True, audit=buf)
    torch.cuda.synchronize()
    rec = buf[slab:].view(torch.int32).view(grid * 8, 1 + cap, 4)
    n = rec[:, 0, 0].long()
    assert int(n.max()) <= cap, 'audit records overflow'
    keep = torch.arange(cap, device=DEV)[None, :] < n[:, None]
    return out, rec[:, 1:][keep].long().cpu()


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
