"""Launch and check helpers for the exact-GELU epilogues of lvl_linear_tn (6 LVL_EPI_BIAS_GELU, 7 LVL_EPI_GELU_BWD,
8 LVL_EPI_BIAS_GELU_DERIV; tests/test_gpu_gemm_gelu_epilogues.py): the kernel table, one guarded launch (gemm_tn_cases.tn
hard-codes which epilogues have aux_out / colsum, so this module has its own; the operand builders and guards are that
module's), operands whose pre-activation is exact in bf16, lvl_act_fwd / lvl_act_bwd launches, and the float64 checks of
gemm_tn_cases.check_random_vs_float64 restated for the GELU. A plain module: no tests, no fixtures."""
import ctypes
import math
import os
import shutil
import subprocess

import pytest
import torch

from gemm_tn_cases import DEV, ROOT, _guarded_out, _untouched
from helpers import guarded_in as _guarded_in
from helpers import launch_config as _launch_config
from helpers import sched_block as _sched_block

# (name, epilogue, f32-class, with bias, aux_in), as gemm_tn_cases.TN_KERNELS
GELU_KERNELS = (('gelu', 6, False, True, None), ('gelu_bwd', 7, False, False, 'u'), ('gelu_deriv', 8, False, True, None),
                ('f32_gelu', 6, True, True, None), ('f32_gelu_bwd', 7, True, False, 'u'))
TWO_OUT, COLSUM = (6, 8), (7,)
SHAPES = ((300, 512, 192), (1, 256, 64), (513, 256, 128))        # (M, N, K); f32-class: K' = 3 K


def gelu64(u):
    return 0.5 * u * (1 + torch.erf(u / math.sqrt(2)))


def gelu_grad64(u):
    return 0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)


def tn(lib, kern, data, sched, guard, audit=None, pad=None):
    """one lvl_linear_tn launch (or lvl_linear_tn_audit with `audit`, the record buffer) of an epilogue 6 / 7 / 8 kernel ->
    dict of outputs. guard: the inputs are the first M rows of NaN/Inf-padded buffers (pad='zero': zero-padded), the outputs
    of sentinel-filled ones (checked here), and the column-sum outputs and workspace start as NaN."""
    from lavila_amd import _cabi as C
    name, epi, f32, with_bias, aux = kern
    x, w = (data['x3'], data['w3']) if f32 else (data['x'], data['w'])
    bias = data['b'] if with_bias else None
    aux_in = data[('f32_' if f32 else '') + aux] if aux else None
    M, K = x.shape
    N = w.shape[0]
    odt = torch.float32 if f32 else torch.bfloat16
    if guard:
        if pad == 'zero':
            zp = lambda t: torch.cat([t, torch.zeros(256, t.shape[1], dtype=t.dtype, device=DEV)])[:M]
            x, aux_in = zp(x), (zp(aux_in) if aux_in is not None else None)
        else:
            x = _guarded_in(x)
            aux_in = _guarded_in(aux_in) if aux_in is not None else None
    ybuf = _guarded_out(M, N, odt) if guard else torch.empty(M, N, dtype=odt, device=DEV)
    abuf = None
    if epi in TWO_OUT:
        abuf = _guarded_out(M, N, odt) if guard else torch.empty(M, N, dtype=odt, device=DEV)
    colsum = ws = None
    P = 2 * ((M + 255) // 256)
    if epi in COLSUM:
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
    if epi in COLSUM:
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


def exact_u_data(M, N, K, seed, nnz=12):
    """Operands whose pre-activation u = x . w^T + b is a multiple of 1/8 with |u| <= 7: x in {-2 .. 2}, w with `nnz`
    entries of +-1/8 per row (|acc| <= nnz / 4 = 3), b multiples of 1/8 in [-4, 4]. Every product and sum is exact in
    float32 and u = k / 8, |k| <= 56, is exact in bf16 (8 significant bits). Both modes: the float32 operands of the
    f32-class mode are the same numbers (their low term images are zero)."""
    from lavila_amd import ops
    g = torch.Generator(device=DEV).manual_seed(seed)
    ri = lambda lo, hi, shape: torch.randint(lo, hi, shape, device=DEV, generator=g).float()
    x = ri(-2, 3, (M, K))
    cols = torch.rand(N, K, device=DEV, generator=g).argsort(1)[:, :nnz]
    w = torch.zeros(N, K, device=DEV).scatter_(1, cols, (2 * ri(0, 2, (N, nnz)) - 1) / 8)
    b = ri(-32, 33, (N,)) / 8
    acc = x.double() @ w.double().t()
    u = acc + b.double()
    assert float(u.abs().max()) <= 8 and torch.equal(u * 8, (u * 8).round())
    assert torch.equal(u.bfloat16().double(), u) and torch.equal(acc.float().double(), acc)
    d = {'M': M, 'x': x.bfloat16(), 'w': w.bfloat16(), 'b': b, 'acc': acc, 'u64': u,
         'x3': ops.split3(x, 0), 'w3': ops.split3(w, 1)}
    d['f32_u'] = 3 * torch.randn(M, N, device=DEV, generator=g)             # pre-activation rows of epilogue 7
    d['u'] = d['f32_u'].bfloat16()
    return d


def act_fwd(u):
    """lvl_act_fwd(u, LVL_ACT_GELU_ERF)"""
    from lavila_amd import _cabi as C
    a = torch.full_like(u, float('nan'))
    C.check(C.lib().lvl_act_fwd(C.ptr(u), C.ptr(a), u.numel(), C.ACT_GELU_ERF, C.dtype_code(u), C.stream_ptr()), 'lvl_act_fwd')
    return a


def act_bwd(u, da):
    """lvl_act_bwd(u, da, LVL_ACT_GELU_ERF) = da * gelu'(u)"""
    from lavila_amd import _cabi as C
    assert u.dtype == da.dtype and u.shape == da.shape
    du = torch.full_like(u, float('nan'))
    C.check(C.lib().lvl_act_bwd(C.ptr(u), C.ptr(da), C.ptr(du), u.numel(), C.ACT_GELU_ERF, C.dtype_code(u), C.stream_ptr()),
            'lvl_act_bwd')
    return du


def pad8(t):
    """[M, N] -> a contiguous tensor with M rounded up to 8 rows (lvl_act_* take n % 8 == 0), and M"""
    M = t.shape[0]
    return torch.cat([t, t.new_zeros((-M) % 8, t.shape[1])]).contiguous(), M


def check_random_vs_float64(kern, out, d, colsum=True):
    """gemm_tn_cases.check_random_vs_float64's bars for epilogues 1, 2, 4 (bf16) and 1, 2 (f32-class), applied to their
    GELU twins 6, 7, 8: one bf16 rounding (2^-8 relative, with margin) plus the f32 accumulation (2^-14 |x| |w|);
    f32-class mode: 3 2^-17 |x| |w|. colsum=False: a window of rows of a larger call (its column sums are checked elsewhere)."""
    name, epi, f32, with_bias, aux = kern
    M = d['M']
    y = out['y'].double()
    b = d['b'].double() if with_bias else 0.0
    if f32:
        xd, wd = d['xf'].double(), d['wf'].double()
        acc = xd @ wd.t()
        bound = 3 * 2.0 ** -17 * (xd.abs() @ wd.abs().t()) + 1e-6
        if epi == 6:
            u = acc + b
            assert ((out['aux_out'].double() - u).abs() <= bound).all(), name
            assert ((y - gelu64(u)).abs() <= 1.5 * bound + 2e-6 * gelu64(u).abs()).all(), name
        else:
            ref = acc * gelu_grad64(d['f32_u'].double())
            assert ((y - ref).abs() <= 1.6 * bound + 2e-6 * ref.abs()).all(), name
            if colsum:
                torch.testing.assert_close(out['colsum'].double(), ref.sum(0), atol=1e-3 * M ** 0.5, rtol=1e-4)
    else:
        xd, wd = d['x'].double(), d['w'].double()
        acc = xd @ wd.t()
        eps = 2.0 ** -14 * (xd.abs() @ wd.abs().t()) + 1e-6
        if epi == 6:
            u = out['aux_out'].double()
            assert ((u - (acc + b)).abs() <= 2.0 ** -8 * (acc + b).abs() + eps).all(), name
            assert ((y - gelu64(u)).abs() <= 2.0 ** -8 * gelu64(u).abs() + 1e-5).all(), name       # the activation sees bf16(u)
        elif epi == 8:
            u = acc + b
            assert ((y - gelu64(u)).abs() <= 2.0 ** -8 * gelu64(u).abs() + 1.2 * eps + 1e-5).all(), name
            dd = out['aux_out'].double()
            assert ((dd - gelu_grad64(u)).abs() <= 2.0 ** -8 * gelu_grad64(u).abs() + 1.2 * eps + 1e-5).all(), name
        else:
            check_bwd_vs_float64(name, out, acc, gelu_grad64(d['u'].double()), eps, colsum)
    for v in out.values():
        assert torch.isfinite(v.float()).all(), name


def check_bwd_vs_float64(name, out, acc, a, eps, colsum=True):
    """bf16 epilogue 7 as check_random_vs_float64 holds epilogue 2: y = acc * a rounded once, the column sums of the
    unrounded f32 products (a row dropped, doubled or taken from behind M would exceed this)."""
    ref = acc * a
    err = 1.2 * eps * a.abs() + 1e-5 * acc.abs()
    assert ((out['y'].double() - ref).abs() <= 2.0 ** -8 * ref.abs() + err).all(), name
    if colsum:
        cs, want = out['colsum'].double(), ref.sum(0)
        assert ((cs - want).abs() <= 2.0 ** -12 * ref.abs().sum(0) + err.sum(0) + 1e-4).all(), name


def ns(kern):
    """the vmcnt allowance of the first blocks after a full tile's epilogue, and the stores a wave issues there"""
    name, epi, f32, with_bias, aux = kern
    if f32:
        return 0, 4 * 2 * 4 * (2 if epi == 6 else 1) + (1 if epi == 7 else 0)
    return (32 if epi in TWO_OUT else 16), 4 * 4 * (2 if epi in TWO_OUT else 1) + (1 if epi == 7 else 0)


def audit_records(alib, kern, d, cus, sched):
    """gemm_tn_cases.audit_run for the GELU kernels -> (outputs, records [R, 4] int64 on the CPU: tm, tn of the finished
    tile, stores the wave issued in its epilogue, allowance of the next tile's first blocks)"""
    cap = alib.lvl_linear_tn_audit_cap()
    M, N = d['M'], d['w'].shape[0]
    grid = torch.cuda.get_device_properties(0).multi_processor_count
    slab = 2 * ((M + 255) // 256) * N if kern[1] in COLSUM else 0
    buf = torch.zeros(slab + grid * 8 * (1 + cap) * 4, dtype=torch.float32, device=DEV)
    with _launch_config([alib], cus, 0):
        out = tn(alib, kern, d, sched, guard=True, audit=buf)
    torch.cuda.synchronize()
    rec = buf[slab:].view(torch.int32).view(grid * 8, 1 + cap, 4)
    n = rec[:, 0, 0].long()
    assert int(n.max()) <= cap, 'audit records overflow'
    keep = torch.arange(cap, device=DEV)[None, :] < n[:, None]
    return out, rec[:, 1:][keep].long().cpu(), rec[:, 0].long().cpu()


_AUDIT_LIB = []           # one build per process


def build_audit_library(out_dir):
    """csrc/gemm_tn_gelu.hip (the translation unit of epilogues 6-8) with -DGM_AUDIT plus the host stub
    (tools/probes/trace_stub.hip) -> a shared library with gemm_tn_cases.build_audit_library's entry points"""
    if _AUDIT_LIB:
        return _AUDIT_LIB[0]
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.fail('hipcc not found: the GM_AUDIT build of gemm_tn_gelu.hip cannot be made')
    from lavila_amd.build import EXTRA_FLAGS
    so = os.path.join(str(out_dir), 'libgemm_gelu_audit.so')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-Wl,-Bsymbolic', '-DGM_AUDIT',
                    *EXTRA_FLAGS['gemm_tn_gelu.hip'], os.path.join(ROOT, 'lavila_amd', 'csrc', 'gemm_tn_gelu.hip'),
                    os.path.join(ROOT, 'tools', 'probes', 'trace_stub.hip'), '-o', so], check=True, timeout=900)
    lib = ctypes.CDLL(so)
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.lvl_linear_tn_audit.restype = I
    lib.lvl_linear_tn_audit.argtypes = [P] * 8 + [ctypes.c_int64, I, I, I, I, P]
    for fn in ('lvl_set_compute_units', 'lvl_debug_late_workgroups'):
        getattr(lib, fn).restype = I
        getattr(lib, fn).argtypes = [I]
    lib.lvl_linear_tn_audit_cap.restype = I
    _AUDIT_LIB.append(lib)
    return lib
