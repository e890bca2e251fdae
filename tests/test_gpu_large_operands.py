"""GPU (-m gpu): the kernels on operands past 2 GiB (B31), 4 GiB (B32) and 2^31 elements (E31).

A 32-bit offset that wraps gives plausible finite numbers, not NaNs, so every case (tests/large_operand_cases.py; its
arithmetic is checked on the CPU by test_large_operand_cases_cpu.py) is held by references that no aliased, dropped or
doubled row survives, without a float64 copy of a multi-GiB tensor:

  * WINDOWS against float64, computed on the device from slices of the same inputs: the first tile / rows, 512 rows
    straddling every boundary the operand crosses, the last partial tile / row. The bounds are the ones the existing case
    modules hold the kernel to (gemm_tn_cases, gelu_tn_cases, rowops_reference, caption_loss_reference.bounds): no new ones;
  * CHUNK EQUALITY, bit for bit: an output that is local to a row equals what the same entry point gives on row chunks that
    each stay below B31 (GEMM chunks cut at multiples of 256 rows) -- every element of the large call, compared on the device;
  * EXACT REDUCTIONS: outputs that sum over all rows (dW, dbias, column sums) on small-integer inputs whose sums stay below
    2^24, with marked rows on both sides of every boundary and at the end; the reference is the float64 sum in row chunks.

Inputs are generated on the device in chunks, comparisons run on the device, tensors are dropped at the end of each test.
"""
import ctypes
import math

import pytest
import torch

import gelu_tn_cases as G
import gemm_tn_cases as T
import large_operand_cases as L
import rowops_reference as R
from helpers import sched_block, wgrad_launch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF = torch.bfloat16
NAN = float('nan')
ENOSYS = -38


@pytest.fixture(scope='module', autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def _C():
    from lavila_amd import _cabi as C
    return C


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _row_step(cols, elems=1 << 26):
    return max(1, elems // cols)


def _randn(rows, cols, seed, dtype, scale=1.0, shift=0.0):
    """scale * N(0, 1) + shift in `dtype`, generated on the device in chunks (no float32 copy of the whole tensor)"""
    out = torch.empty(rows, cols, dtype=dtype, device=DEV)
    g, step = _gen(seed), _row_step(cols)
    for r0 in range(0, rows, step):
        n = min(step, rows - r0)
        out[r0:r0 + n] = torch.randn(n, cols, generator=g, device=DEV) * scale + shift
    return out


def _randint(rows, cols, seed, lo, hi, dtype, keep=None):
    """integers in [lo, hi) (times a Bernoulli(keep) mask) in `dtype`, in chunks"""
    out = torch.empty(rows, cols, dtype=dtype, device=DEV)
    g, step = _gen(seed), _row_step(cols)
    for r0 in range(0, rows, step):
        n = min(step, rows - r0)
        v = torch.randint(lo, hi, (n, cols), generator=g, device=DEV, dtype=torch.int8)
        if keep is not None:
            v = v * (torch.rand(n, cols, generator=g, device=DEV) < keep)
        out[r0:r0 + n] = v
    return out


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _chunks(rows, step):
    return [(r, min(r + step, rows)) for r in range(0, rows, step)]


def _windows(case, rows, half=256):
    """[r0, r1): the first rows, 2 * half rows straddling every boundary the case's operands cross, the last rows"""
    wins = {(0, min(half, rows)), (max(rows - half, 0), rows)}
    for op in case.operands:
        for b in op.crosses:
            r = L.first_row_beyond(op, b)
            wins.add((max(r - half, 0), min(r + half, rows)))
    return sorted(wins)


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if not torch.equal(a, b):
        bits = torch.int16 if a.element_size() == 2 else torch.int32
        bad = (a.view(bits) != b.view(bits)).nonzero()
        raise AssertionError(f'{what}: {bad.shape[0]} elements differ, first at {bad[0].tolist()}')


# ==== lvl_linear_tn / lvl_linear_tn_ragged ==================================================================================
def _kern(epi, f32):
    """the (name, epilogue, f32-class, with bias, aux_in) row of the existing kernel tables"""
    for k in T.TN_KERNELS + G.GELU_KERNELS:
        if k[1] == epi and k[2] == f32 and k[3] == (epi not in L.COLSUM):
            return k
    raise KeyError((epi, f32))


def _tn_call(epi, f32, x, w, bias, aux_in, sched='static', ragged=False):
    """one launch with NaN-prefilled outputs, column sums and workspace -> dict of outputs"""
    C = _C()
    M, K = x.shape
    N = w.shape[0]
    odt = torch.float32 if f32 else BF
    y = _nan(M, N, dtype=odt)
    aux_out = _nan(M, N, dtype=odt) if epi in L.AUX_OUT else None
    colsum = ws = None
    if epi in L.COLSUM:
        colsum = _nan(N)
        ws = C.workspace('linear_tn', M, N, DEV).fill_(NAN)
    blk = sched_block(sched)
    code = C.LVL_F32 if f32 else C.LVL_BF16
    if ragged:
        rc = C.lib().lvl_linear_tn_ragged(C.ptr(x), C.ptr(w), C.ptr(bias), C.ptr(y), C.ptr(blk), M, N, K, epi, code,
                                          C.stream_ptr())
    else:
        rc = C.lib().lvl_linear_tn(C.ptr(x), C.ptr(w), C.ptr(bias), C.ptr(y), C.ptr(aux_out), C.ptr(aux_in), C.ptr(colsum),
                                   C.ptr(ws), C.ptr(blk), M, N, K, epi, code, C.stream_ptr())
    C.check(rc, 'lvl_linear_tn')
    if blk is not None:
        torch.cuda.synchronize()
        assert int(blk.abs().sum()) == 0, blk.tolist()
    out = {'y': y}
    if aux_out is not None:
        out['aux_out'] = aux_out
    if colsum is not None:
        out['colsum'] = colsum
    return out


def _tn_check(case, epi, data, ragged=False):
    """One large call (dynamic schedule where the kernel takes one) held by windows against float64, by bit equality with
    chunk calls (static schedule) and -- column-sum epilogues -- by the float64 column sums over all rows."""
    f32 = case.shape['f32']
    kern = _kern(epi, f32)
    x, w = (data['x3'], data['w3']) if f32 else (data['x'], data['w'])
    bias = data['b'] if kern[3] else None
    aux_key = (('f32_' if f32 else '') + kern[4]) if kern[4] else None
    aux_in = data[aux_key] if aux_key else None
    M = x.shape[0]
    big = _tn_call(epi, f32, x, w, bias, aux_in, 'dynamic', ragged)
    check = G.check_random_vs_float64 if epi >= 6 else T.check_random_vs_float64
    for r0, r1 in L.tn_windows(case):
        d = {'M': r1 - r0, 'b': data['b']}
        if f32:
            d.update(xf=data['xf'][r0:r1], wf=data['wf'])
        else:
            d.update(x=x[r0:r1], w=w)
        if aux_key:
            d[aux_key] = aux_in[r0:r1]
        check(kern, {k: v[r0:r1] for k, v in big.items() if k != 'colsum'}, d, colsum=False)
    for r0, r1 in _chunks(M, L.tn_chunk(case)):
        part = _tn_call(epi, f32, x[r0:r1], w, bias, aux_in[r0:r1] if aux_in is not None else None, 'static', ragged)
        for k in ('y', 'aux_out'):
            if k in big:
                _same(big[k][r0:r1], part[k], f'{case.name} epilogue {epi}: {k} rows {r0}..{r1} differ from the chunk call')
    if epi in L.COLSUM:
        _tn_colsum_check(kern, big['colsum'], data, aux_in, M)


def _tn_colsum_check(kern, colsum, data, aux_in, M):
    """the column-sum bars of gemm_tn_cases.check_random_vs_float64 / gelu_tn_cases.check_bwd_vs_float64 (bf16:
    2^-12 sum |ref| + sum err + 1e-4 with err = 1.2 eps |a| + 1e-5 |acc|, eps = 2^-14 |x| |w| + 1e-6; f32-class: atol
    1e-3 sqrt(M), rtol 1e-4), with the float64 sums accumulated over row chunks"""
    name, epi, f32, _, _ = kern
    N = colsum.shape[0]
    x, w = (data['xf'], data['wf']) if f32 else (data['x'], data['w'])
    wd = w.double()
    s, sa, se = (torch.zeros(N, dtype=torch.float64, device=DEV) for _ in range(3))
    for r0, r1 in _chunks(M, 1 << 14):
        xd = x[r0:r1].double()
        acc = xd @ wd.t()
        u = aux_in[r0:r1].double()
        a = u if epi == 5 else (T._qg_grad(u) if epi == 2 else G.gelu_grad64(u))
        ref = acc * a
        s += ref.sum(0)
        if not f32:
            eps = 2.0 ** -14 * (xd.abs() @ wd.abs().t()) + 1e-6
            sa += ref.abs().sum(0)
            se += (1.2 * eps * a.abs() + 1e-5 * acc.abs()).sum(0)
    if f32:
        torch.testing.assert_close(colsum.double(), s, atol=1e-3 * M ** 0.5, rtol=1e-4)
    else:
        assert ((colsum.double() - s).abs() <= 2.0 ** -12 * sa + se + 1e-4).all(), name


def _tn_data(case, seed, aux=()):
    s = case.shape
    M, N, K = s['M'], s['N'], s['K']
    d = {'M': M, 'b': torch.randn(N, generator=_gen(seed + 2), device=DEV)}
    if s['f32']:
        from lavila_amd import ops
        K0 = K // 3
        d['xf'] = _randn(M, K0, seed, torch.float32)
        d['wf'] = _randn(N, K0, seed + 1, torch.float32, scale=K0 ** -0.5)
        d['x3'], d['w3'] = ops.split3(d['xf'], 0), ops.split3(d['wf'], 1)
    else:
        d['x'] = _randn(M, K, seed, BF)
        d['w'] = _randn(N, K, seed + 1, BF, scale=K ** -0.5)
    odt = torch.float32 if s['f32'] else BF
    pre = 'f32_' if s['f32'] else ''
    if 'u' in aux:                      # pre-activation rows (epilogues 2, 7) and residual rows (3): the same tensor
        d[pre + 'u'] = d[pre + 'r'] = _randn(M, N, seed + 3, odt)
    if 'd' in aux:                      # stored derivative rows (epilogue 5), in [-0.1, 1.1] as gemm_tn_cases.case_data's
        d['d'] = torch.empty(M, N, dtype=BF, device=DEV).uniform_(-0.1, 1.1, generator=_gen(seed + 4))
    return d


_X_CASES = [c for c in L.TN_CASES if c.operands[0].name == 'x' and 'ragged' not in c.entry]


@pytest.mark.parametrize('case', _X_CASES, ids=lambda c: c.name)
def test_linear_tn_x_operand_past_2gib_and_up_to_the_4gib_limit(case):
    """The X operand past B31 (per-lane DMA offsets above 2^31), one row below B32 (the largest M the entry takes at
    K = 4096) and at the largest M of K = 4160, where the tail tile's rows behind M have offsets that wrap past 2^32
    (`xrel + f_xrow` before the clamp): those rows are never stored and never summed."""
    data = _tn_data(case, 31, aux=('u',) if 3 in case.shape['epilogues'] else ())
    for epi in case.shape['epilogues']:
        _tn_check(case, epi, data)
    del data


@pytest.fixture(scope='module')
def y_bf16_data():
    case = next(c for c in L.TN_CASES if c.name == 'y_past_b32')
    data = _tn_data(case, 32, aux=('u', 'd'))
    yield case, data
    data.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize('epi', L.BF16_EPILOGUES)
def test_linear_tn_outputs_past_4gib_bf16(y_bf16_data, epi):
    """y / aux_out / aux_in of more than 4 GiB and 2^31 elements behind a small X: every bf16 epilogue; the column-sum
    epilogues' sums over all rows"""
    case, data = y_bf16_data
    _tn_check(case, epi, data)


@pytest.fixture(scope='module')
def y_f32_data():
    case = next(c for c in L.TN_CASES if c.name == 'y_f32_past_b32')
    data = _tn_data(case, 33, aux=('u',))
    yield case, data
    data.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize('epi', L.F32_EPILOGUES)
def test_linear_tn_outputs_past_4gib_f32_class(y_f32_data, epi):
    """the f32-class mode: float32 y / aux of more than 4 GiB, every epilogue the mode accepts"""
    case, data = y_f32_data
    _tn_check(case, epi, data)


def test_linear_tn_integer_column_sums_past_4gib():
    """LVL_EPI_MUL_AUX_COLSUM on small integers at the y_past_b32 shape: y and its column sums over all 2^19 + 293 rows are
    exact (|y| < 256, every column's sum of |y| below 2^24), so a row dropped, doubled or read from an aliased place
    changes a sum by an integer."""
    case = next(c for c in L.TN_CASES if c.name == 'y_past_b32')
    M, N, K = (case.shape[k] for k in 'MNK')
    x = _randint(M, K, 41, -2, 3, BF)
    w = _randint(N, K, 42, -1, 2, BF, keep=0.08)
    dd = _randint(M, N, 43, -2, 3, BF)
    for r in L.marked_rows(case):               # marked rows: no zero in x or in the multiplier
        x[r] = (2 * torch.randint(0, 2, (K,), generator=_gen(r), device=DEV) - 1).to(BF)
        dd[r] = (2 * torch.randint(0, 2, (N,), generator=_gen(r + 1), device=DEV) - 1).to(BF) * 2
    out = _tn_call(5, False, x, w, None, dd, 'static')
    wd = w.double()
    want = torch.zeros(N, dtype=torch.float64, device=DEV)
    room = torch.zeros(N, dtype=torch.float64, device=DEV)
    for r0, r1 in _chunks(M, 1 << 14):
        ref = (x[r0:r1].double() @ wd.t()) * dd[r0:r1].double()
        assert float(ref.abs().max()) < 256
        assert torch.equal(out['y'][r0:r1].double(), ref), (r0, r1)
        want += ref.sum(0)
        room += ref.abs().sum(0)
    assert float(room.max()) < R.MAX_EXACT and float((room > 0).double().mean()) > 0.9
    assert torch.equal(out['colsum'].double(), want), (out['colsum'].double() - want).abs().max().item()


@pytest.mark.parametrize('case', [c for c in L.TN_CASES if 'ragged' in c.entry], ids=lambda c: c.name)
def test_linear_tn_ragged_past_the_boundaries(case):
    """N = 320: the persistent kernel on the full column tile (output stride 320) and the edge kernel on the 64 columns
    behind it, with y past B32 / E31 and with X past B31"""
    data = _tn_data(case, 34)
    _tn_check(case, 0, data, ragged=True)
    del data


def test_linear_tn_refuses_a_4gib_operand_without_touching_anything():
    """M * K * 2 == 2^32 exactly (one row more than x_below_b32): LVL_ENOSYS from both entries, the outputs, the column
    sums and the tile-counter block as they were"""
    C = _C()
    M, N, K = (L.TN_REFUSED[k] for k in 'MNK')
    x = torch.empty(M, K, dtype=BF, device=DEV)
    w = torch.zeros(N, K, dtype=BF, device=DEV)
    y = torch.empty(4096, N, dtype=BF, device=DEV)          # never written: no need for M rows
    y.view(torch.int16).fill_(T.SENT16)
    blk = sched_block('dynamic')
    for epi in (0, 3):
        rc = C.lib().lvl_linear_tn(C.ptr(x), C.ptr(w), None, C.ptr(y), None, C.ptr(y), None, None, C.ptr(blk), M, N, K, epi,
                                   C.LVL_BF16, C.stream_ptr())
        assert rc == ENOSYS and b'4 GiB' in C.lib().lvl_last_error(), rc
    rc = C.lib().lvl_linear_tn_ragged(C.ptr(x), C.ptr(w), None, C.ptr(y), C.ptr(blk), M, N + 64, K, 0, C.LVL_BF16,
                                      C.stream_ptr())
    assert rc == ENOSYS and b'4 GiB' in C.lib().lvl_last_error(), rc
    rc = C.lib().lvl_linear_tn(C.ptr(x), C.ptr(w), None, C.ptr(y), None, None, None, None, None, 1, 1 << 25, 64, 0,
                                   C.LVL_BF16, C.stream_ptr())          # the weight operand at 4 GiB
    assert rc == ENOSYS, rc
    torch.cuda.synchronize()
    assert bool((y.view(torch.int16) == T.SENT16).all()) and int(blk.abs().sum()) == 0


# ==== lvl_linear_wgrad ======================================================================================================
@pytest.mark.parametrize('case', L.WGRAD_CASES, ids=lambda c: c.name)
def test_linear_wgrad_exact_past_4gib(case):
    """dy and x of more than 4 GiB and 2^31 elements each, one shape per tile family, with and without dbias, static and
    dynamic schedule: small integers (dy sparse, so that every sum of |dy x| stays below 2^24) make dW and dbias exact in
    any summation order; marked rows without a zero sit on both sides of every boundary and at both ends. M runs far
    enough past the 4 GiB row that a row split STARTS behind it (see large_operand_cases._wgrad)."""
    from wgrad_cases import plan
    C = _C()
    M, N, K = (case.shape[k] for k in 'MNK')
    p = plan(C.lib(), M, N, K)           # the kernel forms a full row offset where a split starts: one starts beyond B32
    assert (p['S'] - 1) * p['base'] * 32 >= L.first_row_beyond(case.operands[0], 'B32'), p
    dy = _randint(M, N, 51, -2, 3, BF, keep=0.05)
    x = _randint(M, K, 52, -2, 3, BF)
    for r in L.marked_rows(case):
        dy[r] = (2 * torch.randint(0, 2, (N,), generator=_gen(r), device=DEV) - 1).to(BF)
        x[r] = ((2 * torch.randint(0, 2, (K,), generator=_gen(r + 1), device=DEV) - 1) *
                torch.randint(1, 3, (K,), generator=_gen(r + 2), device=DEV)).to(BF)
    want = torch.zeros(N, K, dtype=torch.float64, device=DEV)
    wantb = torch.zeros(N, dtype=torch.float64, device=DEV)
    nnz = torch.zeros(N, dtype=torch.float64, device=DEV)
    for r0, r1 in _chunks(M, 1 << 18):
        dyd = dy[r0:r1].double()
        want += dyd.t() @ x[r0:r1].double()
        wantb += dyd.sum(0)
        nnz += (dyd != 0).sum(0)
        del dyd
    assert 4 * float(nnz.max()) < R.MAX_EXACT           # |dy x| <= 4: every partial sum of every order is exact
    assert bool((want != 0).any(1).all())
    for want_db in (False, True):
        for sched in ('static', 'dynamic'):
            dw, db = wgrad_launch(C.lib(), dy, x, want_db, sched, guard=False)
            diff = (dw.double() - want).abs()
            assert torch.equal(dw.double(), want), (case.name, want_db, sched, int((diff != 0).sum()), diff.max().item())
            if want_db:
                assert torch.equal(db.double(), wantb), (case.name, sched, (db.double() - wantb).abs().max().item())
    del dy, x


# ==== element-wise row kernels ==============================================================================================
ROW_CHUNK = 1 << 17           # rows of a chunk call: 2^17 x 4096 bf16 = 1 GiB


def _rows_windows(case):
    return _windows(case, case.shape['rows'])


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _within(name, got, want, bound):
    """rowops: |got - want| <= 2 x the model bound (test_gpu_rowops_at_scale._within)"""
    err = (got.double() - want).abs()
    ok = err <= 2 * bound
    assert bool(ok.all()), f'{name}: {int((~ok).sum())} elements beyond 2x the model bound, first at {(~ok).nonzero()[0].tolist()}'


def _gelu_fwd(u, b):
    C = _C()
    a = _nan(*u.shape, dtype=u.dtype)
    C.check(C.lib().lvl_bias_quickgelu_fwd(_p(u), _p(b), _p(a), u.shape[0], u.shape[1], C.dtype_code(u), C.stream_ptr()),
            'lvl_bias_quickgelu_fwd')
    return a


def _gelu_bwd(da, u, b, want_db=True):
    C = _C()
    rows, cols = u.shape
    du = _nan(rows, cols, dtype=u.dtype)
    dbias = _nan(cols) if want_db else None
    ws = _nan(int(C.lib().lvl_workspace_floats(b'bias_quickgelu_bwd', rows, cols))) if want_db else None
    C.check(C.lib().lvl_bias_quickgelu_bwd(_p(da), _p(u), _p(b), _p(du), _p(dbias), _p(ws), rows, cols, C.dtype_code(u),
                                           C.stream_ptr()), 'lvl_bias_quickgelu_bwd')
    return du, dbias


@pytest.mark.parametrize('case', L.ROWS_CASES, ids=lambda c: c.name)
def test_bias_quickgelu_past_2_31_elements(case):
    """lvl_bias_quickgelu_fwd / _bwd on more than 2^31 bf16 elements: windows against float64 (rowops_reference's model
    bounds), chunk equality of a and du, dbias against the float64 sum of the kernel's own du (its f32 accumulation bound),
    and marked rows: with da zero except one marked row per column, dbias equals the kernel's own du of that row bit for
    bit and no other du is non-zero."""
    rows, cols = case.shape['rows'], case.shape['cols']
    u = _randn(rows, cols, 61, BF, scale=2.0)
    da = _randn(rows, cols, 62, BF)
    b = 0.5 * torch.randn(cols, generator=_gen(63), device=DEV)
    a = _gelu_fwd(u, b)
    du, dbias = _gelu_bwd(da, u, b)
    for r0, r1 in _rows_windows(case):
        a64, f64 = R.gelu_ref(u[r0:r1], b)
        ea, ef = R.gelu_bounds(u[r0:r1], b, BF)
        _within('a', a[r0:r1], a64, ea)
        _within('du', du[r0:r1], da[r0:r1].double() * f64, R.gelu_du_bound(da[r0:r1], f64, ef, BF))
    sb, ab = (torch.zeros(cols, dtype=torch.float64, device=DEV) for _ in range(2))
    for r0, r1 in _chunks(rows, ROW_CHUNK):
        _same(a[r0:r1], _gelu_fwd(u[r0:r1], b), f'a rows {r0}..{r1}')
        _same(du[r0:r1], _gelu_bwd(da[r0:r1], u[r0:r1], b, False)[0], f'du rows {r0}..{r1}')
        sb += du[r0:r1].double().sum(0)
        ab += du[r0:r1].double().abs().sum(0)
    _within('dbias', dbias, sb, R.gelu_bwd_depth(rows) * R.U * ab)
    del a, du
    mk = L.marked_rows(case)
    cidx = torch.arange(cols, device=DEV)
    mcol = torch.tensor(mk, device=DEV)[cidx % len(mk)]
    dam = torch.zeros(rows, cols, dtype=BF, device=DEV)
    dam[mcol, cidx] = da[mcol, cidx]
    dum, dbm = _gelu_bwd(dam, u, b)
    nonzero = sum(int((dum[r0:r1] != 0).sum()) for r0, r1 in _chunks(rows, ROW_CHUNK))
    own = dum[mcol, cidx]
    assert nonzero == int((own != 0).sum()) > cols // 2, 'an unmarked du is not exactly 0'
    bad = (dbm != own.float()).nonzero().flatten().tolist()
    assert not bad, f'marked dbias != own du of the marked row at columns {bad[:8]} (rows {mcol[bad[:8]].tolist()})'
    del u, da, dam, dum


def _act(entry, act, u, da=None):
    C = _C()
    n = u.numel()
    if entry == 'inplace':
        out = u.clone()
        C.check(C.lib().lvl_act_inplace(_p(out), n, act, C.dtype_code(u), C.stream_ptr()), 'lvl_act_inplace')
        return out
    out = _nan(*u.shape, dtype=u.dtype)
    if entry == 'fwd':
        C.check(C.lib().lvl_act_fwd(_p(u), _p(out), n, act, C.dtype_code(u), C.stream_ptr()), 'lvl_act_fwd')
    else:
        C.check(C.lib().lvl_act_bwd(_p(u), _p(da), _p(out), n, act, C.dtype_code(u), C.stream_ptr()), 'lvl_act_bwd')
    return out


def _ratio(got, want):
    """test_gpu_narrator_train._ratio / test_gpu_keymask_attention: max |got - want| / max |want|, held to 2^-7"""
    return ((got.double() - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize('case', L.ROWS_CASES, ids=lambda c: c.name)
def test_activations_past_2_31_elements(case):
    """lvl_act_fwd / _bwd / _inplace (gelu_new, relu^2, erf GELU) and lvl_quickgelu_apply on more than 2^31 bf16 elements:
    chunk equality of every element (which is what holds the large call), the in-place form equal to the out-of-place
    one, and windows against float64 that tie the chunk results to the function. The window bars are restated literals:
    activations max |err| <= 2^-7 max |reference| over the window (test_gpu_narrator_train.test_activation_derivatives and
    test_gpu_keymask_attention's erf-GELU test: their `_ratio`; relative to the window's largest value, so it says little
    about small elements -- those are held by the chunk equality); lvl_quickgelu_apply |err| <= 2^-8 |reference| + 1e-30
    elementwise (test_gpu_selective_recompute.test_quickgelu_apply_whole_tensor_equals_row_slices)."""
    from oracle import oracle as O
    C = _C()
    rows, cols = case.shape['rows'], case.shape['cols']
    u = _randn(rows, cols, 71, BF, scale=3.0)
    da = _randn(rows, cols, 72, BF)
    f64 = {C.ACT_GELU_NEW: O.gelu_new, C.ACT_SQRELU: O.sq_relu, C.ACT_GELU_ERF: G.gelu64}
    for act in (C.ACT_GELU_NEW, C.ACT_SQRELU, C.ACT_GELU_ERF):
        a = _act('fwd', act, u)
        du = _act('bwd', act, u, da)
        _same(a, _act('inplace', act, u), f'act {act}: in place != out of place')
        for r0, r1 in _rows_windows(case):
            u64 = u[r0:r1].double().requires_grad_(True)
            a64 = f64[act](u64)
            a64.backward(da[r0:r1].double())
            assert max(_ratio(a[r0:r1], a64.detach()), _ratio(du[r0:r1], u64.grad)) <= 2.0 ** -7, (act, r0)
        for r0, r1 in _chunks(rows, ROW_CHUNK):
            _same(a[r0:r1], _act('fwd', act, u[r0:r1]), f'act {act} fwd rows {r0}..{r1}')
            _same(du[r0:r1], _act('bwd', act, u[r0:r1], da[r0:r1]), f'act {act} bwd rows {r0}..{r1}')
        del a, du
    del da

    def qg(t):
        out = _nan(*t.shape, dtype=t.dtype)
        C.check(C.lib().lvl_quickgelu_apply(_p(t), _p(out), t.shape[0], t.shape[1], C.dtype_code(t), C.stream_ptr()),
                'lvl_quickgelu_apply')
        return out

    a = qg(u)
    for r0, r1 in _rows_windows(case):
        ud = u[r0:r1].double()
        want = ud * torch.sigmoid(1.702 * ud)
        assert bool(((a[r0:r1].double() - want).abs() <= 2.0 ** -8 * want.abs() + 1e-30).all()), r0
    for r0, r1 in _chunks(rows, ROW_CHUNK):
        _same(a[r0:r1], qg(u[r0:r1]), f'quickgelu_apply rows {r0}..{r1}')
    del a, u


@pytest.mark.parametrize('case', L.ROWS_CASES, ids=lambda c: c.name)
def test_dropout_apply_past_2_31_elements(case):
    """lvl_dropout_apply: element e of the flat tensor is kept iff lvl_dropout_mask says so for index e (a 64-bit Philox
    counter), and a kept element is one float32 product rounded once -- every element, against masks drawn in chunks; in
    place equals out of place. The reference mask comes from the same library (lvl_dropout_mask shares the Philox code of
    dropout.h): what this test holds is the element INDEX each value is paired with; the mask itself is held against the
    numpy restatement by test_gpu_decoder_dropout.test_dropout_mask_equals_restatement, also at element 2^34."""
    C = _C()
    rows, cols = case.shape['rows'], case.shape['cols']
    n, seed, site, p = rows * cols, 0x1234567890ABCDEF, 3, 0.25
    x = _randn(rows, cols, 81, BF)
    out = _nan(rows, cols, dtype=BF)
    C.check(C.lib().lvl_dropout_apply(_p(x), _p(out), n, seed, site, p, C.LVL_BF16, C.stream_ptr()), 'lvl_dropout_apply')
    scale = torch.tensor(1.0, device=DEV) / (torch.tensor(1.0, device=DEV) - torch.tensor(p, device=DEV))
    xf, of = x.view(-1), out.view(-1)
    kept = 0
    for e0 in range(0, n, 1 << 28):
        m = min(1 << 28, n - e0)
        mask = torch.full((m,), 77, dtype=torch.uint8, device=DEV)
        C.check(C.lib().lvl_dropout_mask(_p(mask), m, e0, seed, site, p, C.stream_ptr()), 'lvl_dropout_mask')
        assert int(mask.max()) <= 1
        want = torch.where(mask.bool(), (scale * xf[e0:e0 + m].float()).to(BF), torch.zeros((), dtype=BF, device=DEV))
        _same(of[e0:e0 + m], want, f'dropout_apply elements {e0}..{e0 + m}')
        kept += int(mask.sum())
    assert abs(kept / n - (1 - p)) < 1e-3
    C.check(C.lib().lvl_dropout_apply(_p(x), _p(x), n, seed, site, p, C.LVL_BF16, C.stream_ptr()), 'lvl_dropout_apply')
    _same(x, out, 'in place != out of place')
    del x, out


# ==== LayerNorm family ======================================================================================================
def _ln_fwd(x, x2, b, gamma, beta, eps, keep):
    C = _C()
    rows, cols = x.shape
    y = _nan(rows, cols, dtype=x.dtype)
    s = _nan(rows, cols, dtype=x.dtype) if keep else None
    mean, rstd = _nan(rows), _nan(rows)
    C.check(C.lib().lvl_layernorm_fwd(_p(x), _p(x2), _p(b), _p(gamma), _p(beta), _p(s), _p(y), _p(mean), _p(rstd), rows, cols,
                                      eps, C.dtype_code(x), C.stream_ptr()), 'lvl_layernorm_fwd')
    return y, s, mean, rstd


def _ln_bwd(dy, x, gamma, mean, rstd, dadd):
    C = _C()
    rows, cols = x.shape
    dx = _nan(rows, cols, dtype=x.dtype)
    dgamma, dbeta, dxsum = _nan(cols), _nan(cols), _nan(cols)
    ws = _nan(int(C.lib().lvl_workspace_floats(b'layernorm_bwd', rows, cols)))
    C.check(C.lib().lvl_layernorm_bwd(_p(dy), _p(x), None, None, _p(gamma), _p(mean), _p(rstd), _p(dadd), _p(dx), None,
                                      _p(dgamma), _p(dbeta), _p(dxsum), _p(ws), rows, cols, C.dtype_code(x), C.stream_ptr()),
            'lvl_layernorm_bwd')
    return dx, dgamma, dbeta, dxsum


def _ln_cases():
    out = []
    for case in L.LN_CASES:
        for e in case.shape['dtypes']:
            out.append(pytest.param(case, torch.float32 if e == L.F32 else BF, id=f'{case.name}-{"f32" if e == L.F32 else "bf16"}'))
    return out


@pytest.mark.parametrize('case,dt', _ln_cases())
def test_layernorm_family_past_the_boundaries(case, dt):
    """lvl_layernorm_fwd / _apply / _bwd, the _mixed pair (float32 cases) and lvl_droppath_add_layernorm_fwd / _bwd on row
    tensors past B32 (float32, 4096 columns) and past B31 (bf16; float32 at 768 columns).
    Forward: y, the kept sum s, mean, rstd by windows against float64 (s bit-exact against the f32 restatement) and chunk
    equality; lvl_layernorm_apply from s, and from (x, x2, bias) for a forward that kept no sum, rebuilds y to the bit; the stochastic-depth forward with
    scale 1 gives s, h, mean, rstd to the bit, with scales 0 / 2 per sample it equals its own chunk calls.
    Backward (integer dy): dx by windows and chunk equality, dbeta exact, dgamma / dxsum within the f32 accumulation
    bounds of test_gpu_rowops_at_scale over all rows; the stochastic-depth backward with scale 1 gives ds, dgamma, dbeta to
    the bit, dysum within rows 2^-24 sum |dy| (test_gpu_drop_path). The mixed entries equal the float32 ones to the bit."""
    C = _C()
    rows, cols, rps = case.shape['rows'], case.shape['cols'], case.shape['rows_per_sample']
    f32 = dt == torch.float32
    eps = 1e-6
    step = (1 << 28) // cols // (4 * rps) * (4 * rps)      # rows of a chunk call: whole samples (4 n of them: the slices of
                                                           # mean / rstd / scale stay 16-byte aligned), at most 2^30 bytes
    x = _randn(rows, cols, 91, dt, scale=2.0, shift=0.5)
    x2b = _randn(rows, cols, 92, BF)                       # the branch: bf16 values in either dtype (the mixed entries take bf16)
    x2 = x2b.float() if f32 else x2b
    g = _gen(93)
    b = 0.1 * torch.randn(cols, generator=g, device=DEV)
    gamma = 1 + 0.2 * torch.randn(cols, generator=g, device=DEV)
    beta = 0.1 * torch.randn(cols, generator=g, device=DEV)
    y, s, mean, rstd = _ln_fwd(x, x2, b, gamma, beta, eps, True)
    for r0, r1 in _windows(case, rows, half=128):
        want_s = R.ln_sum_f32(x[r0:r1].cpu(), x2[r0:r1].cpu(), b.cpu()).to(dt).to(DEV)
        _same(s[r0:r1], want_s, f's rows {r0}..{r1} not bit-exact')
        s64 = want_s.double()
        y64, mu64, rs64 = R.ln_fwd_ref(s64, gamma, beta, eps)
        ey, emu, ers = R.ln_fwd_bounds(s64, s64.abs(), 0, gamma, beta, eps, cols, dt)
        _within('y', y[r0:r1], y64, ey)
        _within('mean', mean[r0:r1], mu64, emu)
        _within('rstd', rstd[r0:r1], rs64, ers)
    for r0, r1 in _chunks(rows, step):
        part = _ln_fwd(x[r0:r1], x2[r0:r1], b, gamma, beta, eps, True)
        for name, big, small in zip(('y', 's', 'mean', 'rstd'), (y, s, mean, rstd), part):
            _same(big[r0:r1], small, f'layernorm_fwd {name} rows {r0}..{r1}')
        del part
    # lvl_layernorm_apply: from the kept sum it rebuilds y; from (x, x2, bias) the y of a forward that kept no sum (whose
    # statistics are those of the unrounded sum)
    def apply(a0, a1, a2, mu, rs):
        out = _nan(rows, cols, dtype=dt)
        C.check(C.lib().lvl_layernorm_apply(_p(a0), _p(a1), _p(a2), _p(gamma), _p(beta), _p(mu), _p(rs), _p(out), rows, cols,
                                            C.dtype_code(x), C.stream_ptr()), 'lvl_layernorm_apply')
        return out

    _same(apply(s, None, None, mean, rstd), y, 'layernorm_apply(s) != layernorm_fwd')
    y0, _, mean0, rstd0 = _ln_fwd(x, x2, b, gamma, beta, eps, False)
    _same(apply(x, x2, b, mean0, rstd0), y0, 'layernorm_apply(x, x2, bias) != layernorm_fwd without s_out')
    del y0
    if f32:         # the mixed forward: float32 stream, bf16 branch, bf16 rows out
        ym, sm = _nan(rows, cols, dtype=BF), _nan(rows, cols)
        mm, rm = _nan(rows), _nan(rows)
        C.check(C.lib().lvl_layernorm_fwd_mixed(_p(x), _p(x2b), _p(b), _p(gamma), _p(beta), _p(sm), _p(ym), _p(mm), _p(rm),
                                                rows, cols, eps, 0, C.stream_ptr()), 'lvl_layernorm_fwd_mixed')
        _same(sm, s, 'fwd_mixed s')
        _same(mm, mean, 'fwd_mixed mean')
        _same(rm, rstd, 'fwd_mixed rstd')
        for r0, r1 in _chunks(rows, step):
            _same(ym[r0:r1], y[r0:r1].to(BF), f'fwd_mixed y rows {r0}..{r1}')
        del ym, sm
    # stochastic depth, forward: res = x, y = x2, ybias = b
    nsamp = rows // rps

    def dp_fwd(res, yy, scale):
        n = res.shape[0]
        so, ho = _nan(n, cols, dtype=dt), _nan(n, cols, dtype=dt)
        mo, ro = _nan(n), _nan(n)
        C.check(C.lib().lvl_droppath_add_layernorm_fwd(_p(res), _p(yy), _p(b), _p(scale), _p(gamma), _p(beta), _p(so), _p(ho),
                                                       _p(mo), _p(ro), n, rps, cols, eps, C.dtype_code(res), C.stream_ptr()),
                'lvl_droppath_add_layernorm_fwd')
        return so, ho, mo, ro

    one = torch.ones(nsamp, device=DEV)
    for name, big, small in zip(('s', 'h', 'mean', 'rstd'), (s, y, mean, rstd), dp_fwd(x, x2, one)):
        _same(small, big, f'droppath fwd at scale 1: {name}')
    del small
    scale = 2.0 * torch.randint(0, 2, (nsamp,), generator=g, device=DEV).float()
    assert 0 < int((scale == 0).sum()) < nsamp
    dp = dp_fwd(x, x2, scale)
    dropped = (scale == 0).repeat_interleave(rps)
    for r0, r1 in _chunks(rows, step):
        part = dp_fwd(x[r0:r1], x2[r0:r1], scale[r0 // rps:r1 // rps])
        for name, big, small in zip(('s', 'h', 'mean', 'rstd'), dp, part):
            _same(big[r0:r1], small, f'droppath fwd {name} rows {r0}..{r1}')
        _same(dp[0][r0:r1][dropped[r0:r1]], x[r0:r1][dropped[r0:r1]], 'a dropped sample: s != res')
        del part
    del dp, x, x2, x2b, y

    # ---- backward on the kept sum ----
    dyb = _randint(rows, cols, 94, -8, 9, BF)
    dy = dyb.float() if f32 else dyb
    dadd = _randn(rows, cols, 95, dt)
    dx, dgamma, dbeta, dxsum = _ln_bwd(dy, s, gamma, mean, rstd, dadd)
    R.ln_bwd_check(lambda name, got, want, bound, what='': _within(name + what, got, want, bound), f' [{case.name} {dt}]',
                   dt, (dx, None, dgamma, dbeta, dxsum), dy, s, None, None, gamma, mean, rstd, dadd, False)
    want = torch.zeros(cols, dtype=torch.float64, device=DEV)
    for r0, r1 in _chunks(rows, step):
        want += dy[r0:r1].double().sum(0)
        _same(dx[r0:r1], _ln_bwd(dy[r0:r1], s[r0:r1], gamma, mean[r0:r1], rstd[r0:r1], dadd[r0:r1])[0],
              f'layernorm_bwd dx rows {r0}..{r1}')
    assert torch.equal(dbeta.double(), want), 'integer dbeta not exact'
    ws = _nan(int(C.lib().lvl_workspace_floats(b'layernorm_bwd', rows, cols)))
    if f32:
        dxm, dx2 = _nan(rows, cols), _nan(rows, cols, dtype=BF)
        dgm, dbm, dsm = _nan(cols), _nan(cols), _nan(cols)
        C.check(C.lib().lvl_layernorm_bwd_mixed(_p(dyb), _p(s), None, None, _p(gamma), _p(mean), _p(rstd), _p(dadd), _p(dxm),
                                                _p(dx2), _p(dgm), _p(dbm), _p(dsm), _p(ws), rows, cols, 0, C.stream_ptr()),
                'lvl_layernorm_bwd_mixed')
        _same(dxm, dx, 'bwd_mixed dx')
        for name, a_, b_ in (('dgamma', dgm, dgamma), ('dbeta', dbm, dbeta), ('dxsum', dsm, dxsum)):
            _same(a_, b_, f'bwd_mixed {name}')
        for r0, r1 in _chunks(rows, step):
            _same(dx2[r0:r1], dx[r0:r1].to(BF), f'bwd_mixed dx2 rows {r0}..{r1}')
        del dxm, dx2
    # stochastic depth, backward at scale 1: ds, dgamma, dbeta of lvl_layernorm_bwd to the bit, dy = ds
    ds, dyo = _nan(rows, cols, dtype=dt), _nan(rows, cols, dtype=dt)
    dg2, db2, dys = _nan(cols), _nan(cols), _nan(cols)
    ws2 = _nan(int(C.lib().lvl_workspace_floats(b'droppath_add_layernorm_bwd', rows, cols)))
    C.check(C.lib().lvl_droppath_add_layernorm_bwd(_p(dy), _p(s), _p(gamma), _p(mean), _p(rstd), _p(one), _p(dadd), _p(ds),
                                                   _p(dyo), _p(dg2), _p(db2), _p(dys), _p(ws2), rows, rps, cols,
                                                   C.dtype_code(s), C.stream_ptr()), 'lvl_droppath_add_layernorm_bwd')
    _same(ds, dx, 'droppath bwd ds')
    _same(dyo, dx, 'droppath bwd dy at scale 1')
    _same(dg2, dgamma, 'droppath bwd dgamma')
    _same(db2, dbeta, 'droppath bwd dbeta')
    sum64, abs64 = (torch.zeros(cols, dtype=torch.float64, device=DEV) for _ in range(2))
    for r0, r1 in _chunks(rows, step):
        sum64 += dyo[r0:r1].double().sum(0)
        abs64 += dyo[r0:r1].double().abs().sum(0)
    assert bool(((dys.double() - sum64).abs() <= rows * 2.0 ** -24 * abs64).all()), 'dysum beyond the f32 accumulation bound'
    # ... and with per-sample scales: dy = c * ds, sample by sample, equal to its chunk calls
    C.check(C.lib().lvl_droppath_add_layernorm_bwd(_p(dy), _p(s), _p(gamma), _p(mean), _p(rstd), _p(scale), _p(dadd), _p(ds),
                                                   _p(dyo), _p(dg2), _p(db2), _p(dys), _p(ws2), rows, rps, cols,
                                                   C.dtype_code(s), C.stream_ptr()), 'lvl_droppath_add_layernorm_bwd')
    _same(ds, dx, 'droppath bwd ds (scaled)')
    for r0, r1 in _chunks(rows, step):
        c = scale.repeat_interleave(rps)[r0:r1, None]
        _same(dyo[r0:r1], (c * dx[r0:r1].float()).to(dt), f'droppath bwd dy rows {r0}..{r1}')


# ==== vocabulary cross-entropy ==============================================================================================
@pytest.mark.parametrize('case', L.XENT_CASES, ids=lambda c: c.name)
def test_token_xent_past_the_boundaries(case):
    """float32 logits [rows, 50257] past B31 / B32: the per-row results and the gradient rows by windows against float64
    (caption_loss_reference.check_rows: its derived bounds) and by bit equality with chunk calls; the reduction against
    caption_loss_reference.reduce3 of the kernel's own per-row results within the bars of
    test_gpu_caption_loss.test_rows_past_the_grid_cap."""
    import caption_loss_reference as CR
    from lavila_amd import ops
    rows, V, Tc = case.shape['rows'], case.shape['vocab'], case.shape['T']
    pad = 0
    x = _randn(rows, V, 101, torch.float32, scale=3.0).clamp_(-16, 16)
    lab = torch.randint(0, V, (rows,), generator=_gen(102), device=DEV)
    lab[::3] = pad
    up = torch.tensor([1.7], device=DEV)
    coef = 0.37
    lse, nll, pred, correct, counted = ops.token_xent_fwd_raw(x, lab, pad, out=tuple(
        CR.nan_like((rows,), k) for k in (torch.float32, torch.float32, torch.int32, torch.int32, torch.int32)))
    grad = ops.token_xent_bwd_raw(x, lab, lse, up, coef, pad, out=CR.nan_like((rows, CR.padded(V)), torch.float32))
    for r0, r1 in _windows(case, rows, half=8):
        CR.check_rows(x[r0:r1], lab[r0:r1], pad, f'{case.name} rows {r0}..{r1}', coef=coef, upstream=1.7)
    step = 1 << 12                                        # 4096 rows of 50257 float32: 0.8 GB
    for r0, r1 in _chunks(rows, step):
        part = ops.token_xent_fwd_raw(x[r0:r1], lab[r0:r1], pad)
        for name, big, small in zip(('lse', 'nll', 'pred', 'correct', 'counted'), (lse, nll, pred, correct, counted), part):
            _same(big[r0:r1], small, f'token_xent_fwd {name} rows {r0}..{r1}')
        _same(grad[r0:r1], ops.token_xent_bwd_raw(x[r0:r1], lab[r0:r1], lse[r0:r1], up, coef, pad),
              f'token_xent_bwd rows {r0}..{r1}')
    B = rows // Tc
    res = ops.token_xent_reduce_raw(nll, correct, counted, B, Tc, out=CR.nan_like((3,), torch.float32)).cpu().double()
    want = CR.reduce3(nll.cpu(), correct.cpu(), counted.cpu(), B, Tc)
    n_add = Tc + math.ceil(B / 256) + 6 + 4 + 2
    assert abs(res[0] - want[0]) <= n_add * CR.EPS * want[0].abs()
    assert abs(res[1] - want[1]) <= 4 * CR.EPS * want[1]
    per_caption = (nll.cpu().double().reshape(B, Tc).sum(1) / counted.cpu().reshape(B, Tc).sum(1)).abs().max().item()
    assert abs(res[2] - want[2]) <= ((Tc + 1) * CR.EPS * per_caption + 4 * CR.EPS + n_add * CR.EPS) * want[2]
    del x, grad


# ==== gathers ===============================================================================================================
def _gather_case(name):
    return next(c for c in L.GATHER_CASES if c.name == name)


@pytest.mark.parametrize('frame_major', [False, True], ids=['bcfhw', 'bfchw'])
@pytest.mark.parametrize('P', [16, 14])
def test_patchify_video_past_2gib(P, frame_major):
    """a float32 clip batch of more than 2 GiB, both layouts, P = 16 and 14, bf16 patches: equal to torch's own gather
    (oracle.patchify) on the device"""
    from oracle import oracle as O
    C = _C()
    s = _gather_case('patchify').shape
    B, Ch, F, H = s['B'], s['C'], s['F'], s['H']
    video = _randn(B, (F * Ch if frame_major else Ch * F) * H * H, 111 + P, torch.float32)
    video = video.view(B, F, Ch, H, H) if frame_major else video.view(B, Ch, F, H, H)
    assert video.numel() * 4 > L.B31
    N = (H // P) ** 2
    out = torch.full((B + 1, F * N, Ch * P * P), -1536.0, dtype=BF, device=DEV)
    C.check(C.lib().lvl_patchify(_p(video), _p(out), B, Ch, F, H, H, P, int(frame_major), C.LVL_BF16, C.stream_ptr()),
            'lvl_patchify')
    assert bool((out[B] == -1536.0).all()), 'a patch row behind the last clip was written'
    for b0, b1 in _chunks(B, 128):
        v = video[b0:b1]
        want = O.patchify(v.permute(0, 2, 1, 3, 4) if frame_major else v, P).to(BF)
        _same(out[b0:b1], want, f'patchify clips {b0}..{b1}')
    del video, out


def test_embed_tokens_past_2gib(dt=torch.float32):
    """token assembly forward (float32: x past B31) against the f32 restatement pe + (pos + temporal) on the device, one
    rounding; backward on integer dx: d pos_embed, d temporal_embed, d cls_token exact"""
    C = _C()
    s = _gather_case('embed_tokens').shape
    B, F, N, D = s['B'], s['F'], s['N'], s['D']
    pe = _randn(B, F * N * D, 121, dt).view(B, F * N, D)
    g = _gen(122)
    cls, pos, tem = (0.5 * torch.randn(*sh, generator=g, device=DEV) for sh in ((D,), (N + 1, D), (8, D)))
    x = torch.full((B + 1, 1 + F * N, D), -1536.0, dtype=dt, device=DEV)
    C.check(C.lib().lvl_embed_tokens_fwd(_p(pe), _p(cls), _p(pos), _p(tem), _p(x), B, F, N, D, C.dtype_code(pe),
                                         C.stream_ptr()), 'lvl_embed_tokens_fwd')
    assert bool((x[B] == -1536.0).all()), 'a token behind the last clip was written'
    add = (pos[1:][None] + tem[:F, None]).reshape(1, F * N, D)
    for b0, b1 in _chunks(B, 64):
        assert torch.equal(x[b0:b1, 0].float(), (cls + pos[0]).to(dt).float().expand(b1 - b0, D)), (b0, 'cls')
        _same(x[b0:b1, 1:], (pe[b0:b1].float() + add).to(dt), f'embed_tokens clips {b0}..{b1}')
    del pe
    dx = _randint(B, (1 + F * N) * D, 123, -8, 9, dt).view(B, 1 + F * N, D)
    dpos, dtem = _nan(N + 1, D), _nan(8, D)
    ws = _nan(int(C.lib().lvl_embed_tokens_bwd_ws(F, N, D)))
    C.check(C.lib().lvl_embed_tokens_bwd(_p(dx), _p(dpos), _p(dtem), _p(ws), B, F, N, D, 8, C.dtype_code(dx), C.stream_ptr()),
            'lvl_embed_tokens_bwd')
    tot = torch.zeros(1 + F * N, D, dtype=torch.float64, device=DEV)
    for b0, b1 in _chunks(B, 64):
        tot += dx[b0:b1].double().sum(0)
    body = tot[1:].reshape(F, N, D)
    assert torch.equal(dpos[0].double(), tot[0]), 'd cls_token'
    assert torch.equal(dpos[1:].double(), body.sum(0)), 'd pos_embed'
    assert torch.equal(dtem[:F].double(), body.sum(1)), 'd temporal_embed'
    assert torch.equal(dtem[F:], torch.zeros_like(dtem[F:]))
    del dx, x


def test_text_embed_past_2gib():
    """lvl_text_embed_fwd with a float32 x past B31 against table[tokens] + pos on the device; lvl_text_embed_bwd on
    integer dx rows against torch's own index_add_ (exact in any order)"""
    C = _C()
    s = _gather_case('text_embed').shape
    B, Lc, W, V = s['B'], s['L'], s['W'], s['V']
    g = _gen(131)
    tokens = torch.randint(0, V, (B, Lc), generator=g, device=DEV)
    table = torch.randn(V, W, generator=g, device=DEV)
    pos = torch.randn(Lc, W, generator=g, device=DEV)
    x = _nan(B, Lc, W)
    assert x.numel() * 4 > L.B31
    C.check(C.lib().lvl_text_embed_fwd(_p(tokens), Lc, _p(table), _p(pos), _p(x), B, Lc, W, V, C.LVL_F32, C.stream_ptr()),
            'lvl_text_embed_fwd')
    for b0, b1 in _chunks(B, 1024):
        _same(x[b0:b1], table[tokens[b0:b1]] + pos, f'text_embed_fwd captions {b0}..{b1}')
    del x
    dx = _randint(B * Lc, W, 132, -8, 9, torch.float32)
    dtable, dpos = _nan(V, W), _nan(Lc, W)
    ws = torch.empty(int(C.lib().lvl_text_embed_bwd_ws(B, Lc, V)), dtype=torch.int32, device=DEV)
    C.check(C.lib().lvl_text_embed_bwd(_p(dx), _p(tokens), Lc, _p(dtable), _p(dpos), _p(ws), B, Lc, W, V, Lc, C.LVL_F32,
                                       C.stream_ptr()), 'lvl_text_embed_bwd')
    want = torch.zeros(V, W, dtype=torch.float64, device=DEV)
    wantp = torch.zeros(Lc, W, dtype=torch.float64, device=DEV)
    flat = tokens.reshape(-1)
    for r0, r1 in _chunks(B * Lc, Lc * 1024):
        d = dx[r0:r1].double()
        want.index_add_(0, flat[r0:r1], d)
        wantp += d.reshape(-1, Lc, W).sum(0)
    assert torch.equal(dtable.double(), want), 'd token_embedding'
    assert torch.equal(dpos.double(), wantp), 'd positional_embedding'
    del dx


# ==== attention on replicated exact problems ================================================================================
def _replicated(p_tensor, Rn, dt, scale=None, cols=None):
    """[B0, ...] float64 -> [Rn * B0, ...] in dt on the device, replica r times scale[r] (in the last-dim slice `cols`)"""
    t = p_tensor.to(DEV, dt).repeat(Rn, *([1] * (p_tensor.dim() - 1)))
    if scale is not None:
        v = t.view(Rn, *p_tensor.shape)
        sc = scale.to(dt).view(Rn, *([1] * p_tensor.dim()))
        if cols is None:
            v.mul_(sc)
        else:
            v[..., cols] *= sc
    return t


def _replicas_exact(name, got, want, scale, dt, slack):
    """got [Rn, B0, ...] against want [B0, ...] x scale [Rn], in replica chunks, with the bars of
    test_gpu_attention_ties._assert_exact: bf16 bit for bit where the reference is non-zero, float32 within 2^-20 relative;
    where it is zero |got| <= attention_problems.ZERO_SLACK (scaled like the replica)"""
    want = want.to(DEV)
    sc = scale.view(-1, *([1] * want.dim()))
    for r0, r1 in _chunks(got.shape[0], 256):
        g = got[r0:r1].double()
        w = want[None] * sc[r0:r1]
        nz = w != 0
        wrong = (g != w) if dt == BF else ((g - w).abs() > 2.0 ** -20 * w.abs())
        bad = (nz & wrong) | (~nz & (g.abs() > slack * sc[r0:r1].abs()))
        if bool(bad.any()):
            i = bad.nonzero()[0].tolist()
            raise AssertionError(f'{name}: {int(bad.sum())} values wrong, first at replica {r0 + i[0]}, {i[1:]}: '
                                 f'got {g[tuple(i)].item()!r}, want {w[tuple(i)].item()!r}')


def _colsum64(t, width):
    """float64 column sums and column sums of magnitudes of t viewed as [-1, width], in chunks"""
    t2 = t.reshape(-1, width)
    s, a = (torch.zeros(width, dtype=torch.float64, device=DEV) for _ in range(2))
    for r0, r1 in _chunks(t2.shape[0], _row_step(width, 1 << 25)):
        d = t2[r0:r1].double()
        s += d.sum(0)
        a += d.abs().sum(0)
    return s, a


@pytest.mark.parametrize('case', L.ATTN_CASES, ids=lambda c: c.name)
def test_attention_qkv_past_4gib(case):
    """qkv (cls-only: kv) of more than 4 GiB -- bf16: also more than 2^31 elements; float32: the same bytes at half the
    batch -- for the four divided-attention families, the causal text kernels and the cls-only kernels: one exact
    tied-softmax problem (attention_problems) replicated on the device, replica r with v and dout scaled by signs and powers
    of two from a hash of r. Every expected value scales exactly (out with v, dv with dout, dq and dk with both), so out and
    the gradients of EVERY replica are held to the bars of test_gpu_attention_ties._assert_exact and a sample read or written
    at an aliased place shows; lse equals ln(m) in every replica. No call may reach the shape-generic kernels.
    The qkv-bias gradient (divided: lvl_divided_attn_bwd_bias, causal: lvl_qkv_bias_grad): k third exactly 0; q and v thirds
    against the float64 column sums of the kernel's own dq (checked element by element above) and of dout, within the
    column-sum bound of rowops_reference, depth x 2^-24 x sum |terms|, where depth = colsum_depth of the row pass
    (kBiasGradRowBlocks row blocks) or, where the backward kernel itself writes per-workgroup sums of its float32 dq
    accumulators, of at most T terms per workgroup over at most (workspace / D - kColsumMid) partial rows; those accumulators
    differ from the stored dq by at most Problem.noise (the builder's bound on a float32 kernel's P), summed over the rows.
    The divided kernels also run once WITHOUT a bias (lvl_divided_attn_bwd): the same dqkv to the bit."""
    import attention_problems as AP
    from lavila_amd import ops
    C = _C()
    s = case.shape
    B, B0, F, N, H, mode = (s[k] for k in ('B', 'B0', 'F', 'N', 'H', 'mode'))
    dt = BF if s['esize'] == L.BF16 else torch.float32
    flat = mode in ('causal', 'cls')
    T, D, Rn = (N if flat else 1 + F * N), 64 * H, B // B0
    p = AP.make(mode, (B0, N, H) if flat else (B0, F, N, H), 0)
    sc = torch.tensor([L.replica_scales(r) for r in range(Rn)], dtype=torch.float64, device=DEV)      # [Rn, 2]: c_v, c_dout
    cv, co = sc[:, 0], sc[:, 1]
    C.lib().lvl_debug_generic_attention_calls(1)
    if mode == 'cls':
        q_ref, kv_ref, out_ref, dq_ref, dkv_ref = p.as_cls()
        q = _replicated(q_ref.contiguous(), Rn, dt).requires_grad_(True)
        kv = _replicated(kv_ref.contiguous(), Rn, dt, cv, slice(D, 2 * D))
        assert kv.numel() * kv.element_size() > L.B32 and (dt != BF or kv.numel() > L.E31)
        kv.requires_grad_(True)
        dout = _replicated(p.dout[:, 0].contiguous(), Rn, dt, co)
        out = ops.cls_attention(q, kv, H)
        out.backward(dout)
        lse = torch.empty(B, H, dtype=torch.float32, device=DEV)
        C.check(C.lib().lvl_cls_attn_fwd(C.ptr(q.detach()), C.ptr(kv.detach()), C.ptr(torch.empty_like(out)), C.ptr(lse), B, T,
                                         H, C.dtype_code(kv), C.stream_ptr()), 'lvl_cls_attn_fwd')
        tag = case.name
        _replicas_exact(f'{tag} out', out.detach().view(Rn, B0, D), out_ref, cv, dt, AP.ZERO_SLACK)
        _replicas_exact(f'{tag} dq', q.grad.view(Rn, B0, D), dq_ref, cv * co, dt, AP.ZERO_SLACK)
        g = kv.grad.view(Rn, B0, T, 2 * D)
        _replicas_exact(f'{tag} dk', g[..., :D], dkv_ref[..., :D], cv * co, dt, AP.ZERO_SLACK)
        _replicas_exact(f'{tag} dv', g[..., D:], dkv_ref[..., D:], co, dt, AP.ZERO_SLACK)
        err = (lse.double().view(Rn, B0, H) - p.lse[:, :, 0].to(DEV)[None]).abs().max().item()
        assert err <= 1e-6, f'lse differs from ln(m) by {err}'
        return
    x = _replicated(p.qkv, Rn, dt, cv, slice(2 * D, 3 * D))
    dout = _replicated(p.dout, Rn, dt, co)
    assert x.numel() * x.element_size() > L.B32 and (dt != BF or x.numel() > L.E31)
    x.requires_grad_(True)
    bias = torch.zeros(3 * D, device=DEV, requires_grad=True)
    out = ops.causal_attention(x, H, bias=bias) if flat else ops.divided_attention(x, F, N, H, mode, bias=bias)
    out.backward(dout)
    if flat:
        lse = torch.empty(B, H, T, dtype=torch.float32, device=DEV)
        C.check(C.lib().lvl_causal_attn_fwd(C.ptr(x.detach()), C.ptr(torch.empty_like(out)), C.ptr(lse), B, T, H,
                                            C.dtype_code(x), C.stream_ptr()), 'lvl_causal_attn_fwd')
    else:
        _, lse = ops.divided_attn_fwd_raw(x.detach(), F, N, H, {'space': 0, 'time': 1}[mode])
    torch.cuda.synchronize()
    assert C.lib().lvl_debug_generic_attention_calls(1) == 0
    tag = case.name
    g = x.grad.view(Rn, B0, T, 3 * D)
    _replicas_exact(f'{tag} out', out.detach().view(Rn, B0, T, D), p.out, cv, dt, AP.ZERO_SLACK)
    _replicas_exact(f'{tag} dq', g[..., :D], p.dqkv[..., :D], cv * co, dt, AP.ZERO_SLACK)
    _replicas_exact(f'{tag} dk', g[..., D:2 * D], p.dqkv[..., D:2 * D], cv * co, dt, AP.ZERO_SLACK)
    _replicas_exact(f'{tag} dv', g[..., 2 * D:], p.dqkv[..., 2 * D:], co, dt, AP.ZERO_SLACK)
    err = (lse.double().view(Rn, B0, H, T) - p.lse.to(DEV)[None]).abs().max().item()
    assert err <= 1e-6, f'lse differs from ln(m) by {err}'
    # ---- the bias gradient ----
    db = bias.grad.double()
    assert torch.count_nonzero(db[D:2 * D]) == 0, 'd(bias) k third must be exactly 0'
    rows = B * T
    gy = min(rows, R.QKV_BIAS_ROW_BLOCKS)
    depth = R.colsum_depth(-(-rows // gy), gy)                     # the row pass over dqkv / dout (qkv_bias_partial_kernel)
    depth_q = depth
    if not flat:                                                   # the rider: per-workgroup sums written by the backward itself
        n2 = int(C.lib().lvl_divided_attn_bwd_bias_ws(B, F, N, H, {'space': 0, 'time': 1}[mode], C.dtype_code(x)))
        depth_q = max(depth, R.colsum_depth(T, max(n2 // D - R.COLSUM_MID, 1)))
    sum_q = torch.zeros(D, dtype=torch.float64, device=DEV)
    abs_q = torch.zeros(D, dtype=torch.float64, device=DEV)
    for r0, r1 in _chunks(Rn, 256):
        d = g[r0:r1, ..., :D].double()
        sum_q += d.sum((0, 1, 2))
        abs_q += d.abs().sum((0, 1, 2))
    noise = p.noise[..., :D].sum((0, 1)).to(DEV) * float((cv * co).abs().sum())
    sum_v, abs_v = _colsum64(dout, D)
    eq, ev = (db[:D] - sum_q).abs(), (db[2 * D:] - sum_v).abs()
    bq, bv = depth_q * R.U * abs_q + noise, depth * R.U * abs_v
    print(f'[{tag}] d(bias) q third: worst err / bound {float((eq / bq.clamp_min(1e-300)).max()):.3g} (depth {depth_q}, '
          f'noise share {float((noise / bq.clamp_min(1e-300)).max()):.3g}); v third: {float((ev / bv.clamp_min(1e-300)).max()):.3g}')
    assert bool((eq <= bq).all()), 'd(bias) q third beyond the column-sum bound'
    assert bool((ev <= bv).all()), 'd(bias) v third beyond the column-sum bound'
    if not flat:                                                   # lvl_divided_attn_bwd: the call without a bias
        grad = x.grad
        x.grad = None
        del g
        ops.divided_attention(x, F, N, H, mode).backward(dout)
        _same(x.grad, grad, f'{tag}: dqkv without a bias differs from dqkv with one')
    del x, dout, out


# ==== host routing: the fused MLP on both sides of the _tn_ok gate ==========================================================
def _sparse_signs(rows, cols, nnz, seed):
    """[rows, cols] float32 with exactly nnz entries of +-1 per row"""
    g = _gen(seed)
    idx = torch.rand(rows, cols, generator=g, device=DEV).argsort(1)[:, :nnz]
    return torch.zeros(rows, cols, device=DEV).scatter_(1, idx, (2 * torch.randint(0, 2, (rows, nnz), generator=g, device=DEV) - 1).float())


@pytest.mark.parametrize('side', ['below_gate', 'at_gate'])
def test_fused_mlp_routing_at_the_tn_gate(side):
    """ops.mlp_quickgelu, forward and backward, bf16, 768 -> 3072 -> 768, through ops' own routing: one 256-row tile below
    the _tn_ok gate (698 795 rows: lvl_linear_tn's fused epilogues and lvl_linear_wgrad, under forbid_library_gemm) and at
    the gate (699 051 rows: the hidden tensors pass 2^31 elements, so the GEMMs go to the library -- shown by
    forbid_library_gemm raising -- while lvl_bias_quickgelu_fwd / _bwd and lvl_linear_wgrad run on them).
    EXACT on every element of both routings: x in {-2..2}, two +-1 per row of W1 and b1 = 16 put every pre-activation at an
    integer in [12, 20], where sigmoid(1.702 u) is 1 in float32 (e^-20.4 < 2^-24, in either sigmoid expression), so the
    activation is u and its derivative 1; four +-1 per row of W2 and a sparse dy in {-2..2} keep y, dx below 256 (exact in
    bf16) and every sum of dW1, dW2, db1 below 2^24 (exact in float32 in any order). The reference is float64 in row chunks;
    rows just in front of 2^31 elements of the hidden tensor and the last row (which straddles it) carry no zero in x / dy."""
    import contextlib
    from lavila_amd import ops
    from lavila_amd.guards import forbid_library_gemm
    C = _C()
    rows = L.MLP_ROWS[side]
    d, h = L.MLP_WIDTHS
    fused = side == 'below_gate'
    x = _randint(rows, d, 141, -2, 3, BF)
    dy = _randint(rows, d, 142, -2, 3, BF, keep=0.05)
    for r in (0, L.E31 // h - 1, L.E31 // h, rows - 1):
        r = min(r, rows - 1)
        x[r] = (2 * torch.randint(0, 2, (d,), generator=_gen(r), device=DEV) - 1).to(BF)
        dy[r] = (2 * torch.randint(0, 2, (d,), generator=_gen(r + 1), device=DEV) - 1).to(BF)
    w1 = _sparse_signs(h, d, 2, 143).requires_grad_(True)
    w2 = _sparse_signs(d, h, 4, 144).requires_grad_(True)
    b1 = torch.full((h,), 16.0, device=DEV, requires_grad=True)
    x.requires_grad_(True)
    assert ops._mlp_fused_ok(x, w1, b1, w2) is fused
    calls = {}
    lib = C.lib()
    real = {n: getattr(lib, n) for n in ('lvl_bias_quickgelu_fwd', 'lvl_bias_quickgelu_bwd', 'lvl_linear_wgrad', 'lvl_linear_tn')}

    def spy(n):
        def f(*a):
            calls[n] = calls.get(n, 0) + 1
            return real[n](*a)
        return f
    try:
        for n in real:
            setattr(lib, n, spy(n))
        if not fused:
            with pytest.raises(AssertionError, match='library GEMM'), forbid_library_gemm(), torch.no_grad():
                ops.mlp_quickgelu(x.detach(), w1, b1, w2)
            calls.clear()
        with forbid_library_gemm() if fused else contextlib.nullcontext():
            y = ops.mlp_quickgelu(x, w1, b1, w2)
            y.backward(dy)
        torch.cuda.synchronize()
    finally:
        for n in real:
            setattr(lib, n, real[n])
    if fused:
        assert calls == {'lvl_linear_tn': 4, 'lvl_linear_wgrad': 2}, calls
    else:
        assert calls == {'lvl_bias_quickgelu_fwd': 1, 'lvl_bias_quickgelu_bwd': 1, 'lvl_linear_wgrad': 2}, calls
    w1d, w2d = w1.detach().double(), w2.detach().double()
    dw1, dw2 = (torch.zeros_like(t) for t in (w1d, w2d))
    db1 = torch.zeros(h, dtype=torch.float64, device=DEV)
    room1, room2 = torch.zeros_like(w1d), torch.zeros_like(w2d)
    xg = x.grad
    for r0, r1 in _chunks(rows, 1 << 15):
        xd, dyd = x.detach()[r0:r1].double(), dy[r0:r1].double()
        u = xd @ w1d.t() + 16.0
        assert 12 <= float(u.min()) and float(u.max()) <= 20
        yd = u @ w2d.t()
        du = dyd @ w2d
        dxd = du @ w1d
        assert float(yd.abs().max()) < 256 and float(dxd.abs().max()) < 256 and float(du.abs().max()) < 256
        assert torch.equal(y.detach()[r0:r1].double(), yd), (side, 'y', r0)
        assert torch.equal(xg[r0:r1].double(), dxd), (side, 'dx', r0)
        dw2 += dyd.t() @ u
        dw1 += du.t() @ xd
        db1 += du.sum(0)
        room2 += dyd.abs().t() @ u.abs()
        room1 += du.abs().t() @ xd.abs()
    assert float(room1.max()) < R.MAX_EXACT and float(room2.max()) < R.MAX_EXACT and float(du.abs().max()) > 0
    assert torch.equal(w2.grad.double(), dw2), (side, 'dW2', (w2.grad.double() - dw2).abs().max().item())
    assert torch.equal(w1.grad.double(), dw1), (side, 'dW1', (w1.grad.double() - dw1).abs().max().item())
    assert torch.equal(b1.grad.double(), db1), (side, 'db1', (b1.grad.double() - db1).abs().max().item())
    del x, dy, y
