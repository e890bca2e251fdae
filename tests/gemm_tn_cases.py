"""Launch and check helpers of the lvl_linear_tn matrices (test_gpu_gemm_tails.py: the M axis, test_gpu_gemm_kblocks.py:
the K axis): the kernel table, one guarded launch, operand builders (K is an argument), the float64 and exact-integer
checkers, and the GM_AUDIT build of csrc/gemm_tn_mfma.hip with its record readers. A plain module: no tests, no fixtures."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

from helpers import guarded_in as _guarded_in
from helpers import launch_config as _launch_config
from helpers import sched_block as _sched_block

DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (compute units (0 = the device's), schedule). No late workgroups at 8 CUs: there the hook would leave an XCD's single
# workgroup idle for the whole launch and nobody would serve that XCD's tile queue (test_gpu_parity_bf16.py)
CONFIGS = tuple((cus, sched) for cus in (8, 16, 0) for sched in ('static', 'dynamic', 'late')
                if not (cus == 8 and sched == 'late'))
LATE_MOD = 3
SENT16, SENT32 = 0x7FA5, 0x7FA5A5A5     # sentinel bit patterns of the output guard rows (NaN payloads nobody writes)
DYN_MIN_NB = 5                          # fewest K blocks per tile the dynamic schedule takes (csrc/gemm_tn_mfma.hip)


def rows(tiles, rem):
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


def tn(lib, kern, data, sched, guard, audit=None):
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


def case_data(N, M, seed, k_bf16, k_f32):
    """random operands of one (N, M) case, device generators only. k_bf16 / k_f32: the contraction widths of the bf16
    kernels and of the f32-class ones (K' = 3 k_f32); None leaves that mode's tensors out."""
    from lavila_amd import ops
    g = torch.Generator(device=DEV).manual_seed(seed)
    d = {'M': M}
    if k_bf16 is not None:
        d['x'] = torch.randn(M, k_bf16, device=DEV, generator=g).bfloat16()
        d['w'] = (torch.randn(N, k_bf16, device=DEV, generator=g) * k_bf16 ** -0.5).bfloat16()
    d['b'] = torch.randn(N, device=DEV, generator=g)
    if k_bf16 is not None:
        d['u'] = torch.randn(M, N, device=DEV, generator=g).bfloat16()          # pre-activation rows (epilogue 2)
        d['r'] = torch.randn(M, N, device=DEV, generator=g).bfloat16()          # residual rows (epilogue 3)
        d['d'] = (torch.rand(M, N, device=DEV, generator=g) * 1.2 - 0.1).bfloat16()     # derivative rows (epilogue 5)
    if k_f32 is not None:
        xf = torch.randn(M, k_f32, device=DEV, generator=g)
        wf = torch.randn(N, k_f32, device=DEV, generator=g) * k_f32 ** -0.5
        d['xf'], d['wf'] = xf, wf
        d['x3'], d['w3'] = ops.split3(xf, 0), ops.split3(wf, 1)
        d['f32_u'] = torch.randn(M, N, device=DEV, generator=g)
        d['f32_r'] = torch.randn(M, N, device=DEV, generator=g)
    return d


def int_data(N, M, seed, k_bf16, k_f32):
    """small-integer operands of one (N, M) case (both modes)"""
    from lavila_amd import ops
    g = torch.Generator(device=DEV).manual_seed(seed)
    ri = lambda lo, hi, shape: torch.randint(lo, hi, shape, device=DEV, generator=g).float()
    d = {'M': M}
    xi = ri(-2, 3, (M, k_bf16))
    wi = ri(-1, 2, (N, k_bf16)) * (torch.rand(N, k_bf16, device=DEV, generator=g) < 0.08)
    d['x'], d['w'], d['b'] = xi.bfloat16(), wi.bfloat16(), ri(-8, 9, (N,))
    d['r'] = ri(-8, 9, (M, N)).bfloat16()
    d['d'] = ri(-2, 3, (M, N)).bfloat16()
    d['acc'] = xi.double() @ wi.double().t()
    xf = ri(-300, 301, (M, k_f32))                 # |x| > 256: non-zero low term images
    wf = ri(-3, 4, (N, k_f32))
    d['x3'], d['w3'] = ops.split3(xf, 0), ops.split3(wf, 1)
    d['f32_r'] = ri(-1000, 1001, (M, N))
    d['f32_acc'] = xf.double() @ wf.double().t()
    return d


def check_random_vs_float64(kern, out, d, colsum=True):
    """float64 reference of one kernel on the random operands: one bf16 rounding (2^-8 relative, with margin) plus the
    f32 accumulation (2^-14 |x| |w|); f32-class mode: 3 2^-17 |x| |w| (test_gpu_f32_class.py). colsum=False: `out` and `d`
    are a window of rows of a larger call; its column sums (over all rows) are checked elsewhere
    (test_gpu_large_operands.py)."""
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
            if colsum:
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
        if colsum:
            cs, want = out['colsum'].double(), ref.sum(0)
            assert ((cs - want).abs() <= 2.0 ** -12 * ref.abs().sum(0) + err.sum(0) + 1e-4).all(), name
    for v in out.values():
        assert torch.isfinite(v.float()).all(), name


def check_integers(kern, out, d):
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


def same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


# --------------------------------------------------------------------------------------------------------------------
# the GM_AUDIT build
# --------------------------------------------------------------------------------------------------------------------
_AUDIT_LIB = []           # one build per process: both test modules' fixtures share it


def build_audit_library(out_dir):
    """gemm_tn_mfma.hip with -DGM_AUDIT plus the host stub (tools/probes/trace_stub.hip) -> a shared library"""
    if _AUDIT_LIB:
        return _AUDIT_LIB[0]
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
    _AUDIT_LIB.append(lib)
    return lib


def ns(kern):
    """the vmcnt allowance of the first blocks after a full tile's epilogue, and the stores a wave issues there"""
    name, epi, f32, with_bias, aux = kern
    if f32:
        return 0, 4 * 2 * 4 * (2 if epi == 1 else 1) + (1 if epi == 2 else 0)
    return (32 if epi in (1, 4) else 16), 4 * 4 * (2 if epi in (1, 4) else 1) + (1 if epi in (2, 5) else 0)


def audit_run(alib, kern, d, cus, sched):
    """one audited launch under a launch configuration -> (outputs, records [R, 4] int64 on the CPU: tm, tn of the
    finished tile, stores the wave issued in its epilogue, allowance of the next tile's first blocks; headers
    [grid * 8, 4] int64 on the CPU, row = workgroup * 8 + wave: records, fill-order violations, code of the first one,
    tightest margin (0x7fffffff: the wave made no check; all zero: the workgroup was not launched or had no tile))"""
    cap = alib.lvl_linear_tn_audit_cap()
    M, N = d['M'], (d['w'] if 'w' in d else d['w3']).shape[0]
    grid = torch.cuda.get_device_properties(0).multi_processor_count     # room for the largest grid a launch can have
    slab = 2 * ((M + 255) // 256) * N if kern[1] in (2, 5) else 0
    buf = torch.zeros(slab + grid * 8 * (1 + cap) * 4, dtype=torch.float32, device=DEV)
    with _launch_config([alib], cus, LATE_MOD if sched == 'late' else 0):
        out = tn(alib, kern, d, sched, guard=True, audit=buf)
    torch.cuda.synchronize()
    rec = buf[slab:].view(torch.int32).view(grid * 8, 1 + cap, 4)
    n = rec[:, 0, 0].long()
    assert int(n.max()) <= cap, 'audit records overflow'
    keep = torch.arange(cap, device=DEV)[None, :] < n[:, None]
    return out, rec[:, 1:][keep].long().cpu(), rec[:, 0].long().cpu()


def audit_records(alib, kern, d, cus, sched):
    """audit_run without the headers"""
    return audit_run(alib, kern, d, cus, sched)[:2]


CHECK_NAMES = ('opening barrier: X0 of block 0', 'opening barrier: W0 of block 0', 'barrier in front of P0: W1(j)',
               'barrier in front of P1: X1(j)', 'barrier in front of P2: X0(j+1)', 'barrier in front of P3: W0(j+1)',
               'init_acc: bias image', 'publish: tile-counter reply', "epilogue's re-read: X0 of the next tile",
               "epilogue's re-read: W0 of the next tile")


def decode_violation(code):
    """the first-violation code of a wave's audit header -> text"""
    chk, kb, ti = (code >> 24) & 15, (code >> 12) & 4095, code & 4095
    what = CHECK_NAMES[chk] if chk < len(CHECK_NAMES) else f'check {chk}'
    return f'{what}, tile ordinal {ti}, K block {kb} (= nb: in or behind the epilogue)'


# --------------------------------------------------------------------------------------------------------------------
# the K-axis matrix (test_gpu_gemm_kblocks.py, test_gemm_kblocks_cpu.py)
# --------------------------------------------------------------------------------------------------------------------
# row remainders: both sides of a 32-row group (33), of the second wave half (129), the one-row and all-but-one-row tails
KB_REMAINDERS = (0, 1, 33, 129, 255)
# N -> (tile rows, remainders). Both shapes have 48 tiles: at 8 CUs every workgroup walks 6 consecutive tiles (N = 768: two
# tile rows with tn cycling 0, 1, 2 -- consecutive tiles use different bias images and the ring of four images wraps), at
# 16 CUs 3 tiles, at all CUs one tile (the single-tile prologue and the past-the-end re-read). N = 256: tiles_n = 1.
KB_SHAPES = {768: (16, KB_REMAINDERS), 256: (48, (33,))}
# (mode, K): K blocks per tile nb = K / 64 = 1 .. 8 for the bf16 kernels; f32-class mode K' = 3 K: nb = 3 (the smallest
# legal one) and 9 (nb = 6 is test_gpu_gemm_tails.py's)
KB_MODES = tuple(('bf16', 64 * nb) for nb in range(1, 9)) + (('f32', 64), ('f32', 192))
KB_CASES = tuple((mode, K, N, rem) for mode, K in KB_MODES for N, (_, rems) in KB_SHAPES.items() for rem in rems)


def kb_blocks(mode, K):
    """K blocks per tile"""
    return K // 64 if mode == 'bf16' else 3 * K // 64


def kb_rows(N, rem):
    return rows(KB_SHAPES[N][0], rem)


def kb_kernels(mode):
    return tuple(k for k in TN_KERNELS if k[2] == (mode == 'f32'))


def kb_configs(mode, K):
    """below DYN_MIN_NB the launch takes the static schedule whatever it is handed: static at 8 / 16 / all CUs, and one call
    with a counter block ('dynamic' at all CUs: the result must equal the static one, the block must stay zero)"""
    if kb_blocks(mode, K) >= DYN_MIN_NB:
        return CONFIGS
    return ((8, 'static'), (16, 'static'), (0, 'static'), (0, 'dynamic'))


def static_walk(ntiles, cus):
    """the static tile walk of gemm_tn_kernel restated: tiles (N-fastest order) of every workgroup, in the order it runs
    them. The grid is min(tiles, CUs) rounded down to whole XCD rounds; workgroup b works on XCD b % 8's contiguous range
    [xstart, xstart + cnt) at stride wpx = workgroups per XCD."""
    grid = min(ntiles, cus)
    if grid >= 8:
        grid -= grid % 8
    nx = 8 if grid >= 8 else 1
    wpx = grid // nx
    tq, tr = divmod(ntiles, nx)
    walks = []
    for bid in range(grid):
        xcd = bid % nx
        cnt = tq + (1 if xcd < tr else 0)
        xstart = xcd * (tq + 1) if xcd < tr else tr * (tq + 1) + (xcd - tr) * tq
        walks.append([xstart + t for t in range(bid // nx, cnt, wpx)])
    return walks


def split3_host(x, role):
    """lvl_split_bf16x3 in torch: float32 [R, C] -> bf16 [R, 3C] term images (h, h, l) (role 0) or (h, l, h) (role 1)"""
    h = x.bfloat16()
    lo = (x - h.float()).bfloat16()
    return torch.cat((h, h, lo) if role == 0 else (h, lo, h), 1)


def kblock_int_data(N, M, seed, mode, K, device):
    """small-integer operands in which EVERY K block counts: dropping or repeating any block of 64 contraction elements
    changes every output element, because every block's contribution x[:, blk] . w[:, blk]^T is non-zero by construction.
      bf16: marker columns 64 b hold +-1 in x and in w; everywhere else x is EVEN (-2 / 0 / 2) and w the usual sparse +-1:
            a block contributes (+-1) + (an even number): odd;
      f32-class (the operands are the term images [xh | xh | xl], [wh | wl | wh] of float32 matrices, K' = 3 K): marker
            columns hold +-257 = 256 + 1 in x and in w (both term images non-zero), everywhere else |x| <= 300 and w sparse
            in -3 .. 3 (no low image). A block of xh . wh holds 65536 against at most 63 * 300 * 3 from the other columns, a
            block of xh . wl exactly +-256, a block of xl . wh 256 against at most 63 * 3. The reference is the float64
            product OF THE IMAGES (the kernel never forms xl . wl).
    All sums stay integers below 2^8 (bf16 results) / 2^24 (float32 results): exact in any order."""
    g = torch.Generator(device=device).manual_seed(seed)
    ri = lambda lo, hi, shape: torch.randint(lo, hi, shape, device=device, generator=g).float()
    sparse = lambda shape: (torch.rand(shape, device=device, generator=g) < 0.08).float()
    cols = torch.arange(0, K, 64, device=device)
    d = {'M': M, 'b': ri(-8, 9, (N,))}
    if mode == 'bf16':
        xi = 2 * ri(-1, 2, (M, K))
        wi = ri(-1, 2, (N, K)) * sparse((N, K))
        xi[:, cols] = 2 * ri(0, 2, (M, len(cols))) - 1
        wi[:, cols] = 2 * ri(0, 2, (N, len(cols))) - 1
        d['x'], d['w'] = xi.bfloat16(), wi.bfloat16()
        d['r'] = ri(-8, 9, (M, N)).bfloat16()
        d['d'] = ((2 * ri(0, 2, (M, N)) - 1) * ri(1, 3, (M, N))).bfloat16()        # -2, -1, 1, 2: never hides a product
        d['acc'] = d['x'].double() @ d['w'].double().t()
    else:
        xf = ri(-300, 301, (M, K))
        wf = ri(-3, 4, (N, K)) * sparse((N, K))
        xf[:, cols] = 257 * (2 * ri(0, 2, (M, len(cols))) - 1)
        wf[:, cols] = 257 * (2 * ri(0, 2, (N, len(cols))) - 1)
        d['xf'], d['wf'] = xf, wf
        d['x3'], d['w3'] = split3_host(xf, 0), split3_host(wf, 1)
        d['f32_r'] = ri(-1000, 1001, (M, N))
        d['f32_acc'] = d['x3'].double() @ d['w3'].double().t()
    return d


def check_every_block_counts(d, mode, share=0.9):
    """the conditions on kblock_int_data's operands, on the reference alone: the results are exactly representable, and
    for more than one K block the reference with block b REMOVED, and with block b counted TWICE, differs from the true
    one in at least `share` of the output elements, for every b. (Integers: removing / repeating block b is subtracting /
    adding its own product, exactly.)"""
    xop, wop, acc = (d['x'], d['w'], d['acc']) if mode == 'bf16' else (d['x3'], d['w3'], d['f32_acc'])
    room = float(acc.abs().max() + d['b'].abs().max())
    if mode == 'bf16':
        assert room + float(d['r'].abs().max()) < 256, room                # epilogues 0, 1, 3: bf16 holds integers < 256
        assert float((acc * d['d'].double()).abs().max()) < 256            # epilogue 5
        assert bool((d['d'] != 0).all())
    else:
        assert room + float(d['f32_r'].abs().max()) < 2 ** 24, room
    nb = xop.shape[1] // 64
    total = torch.zeros_like(acc)
    worst = 1.0
    for b in range(nb):
        part = xop[:, 64 * b:64 * b + 64].double() @ wop[:, 64 * b:64 * b + 64].double().t()
        total += part
        if nb > 1:
            removed, twice = acc - part, acc + part
            worst = min(worst, int((removed != acc).sum()) / acc.numel(), int((twice != acc).sum()) / acc.numel())
    assert torch.equal(total, acc)                  # the blocks are the whole contraction
    assert worst >= share, (mode, nb, worst)
    return worst
