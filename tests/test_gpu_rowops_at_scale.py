"""GPU (-m gpu): the HBM-bound row kernels past their grid caps, against float64.

Every row kernel caps its grid and walks rows with a grid stride; LayerNorm also prefetches the next row of its chain,
bias+QuickGELU and the qkv bias partials unroll the row loop by 4. The unit tests in test_gpu_kernels.py stay below the
caps, so the code that runs past them -- the code of every benched step -- is covered here, at row counts taken from
the caps (rowops_reference.py mirrors them; test_rowops_reference_cpu.py checks the mirror against the sources).

  * every kernel is compared with a torch float64 restatement (rowops_reference.py) within a bound from an error model
    written beside it; asserts use 2x the first-order bound;
  * column sums are also checked EXACTLY: integer fingerprints (dy / da / dq in [-8, 8], sums < 2^24) and marked rows
    (LayerNorm: marked row k carries +-2^-k, so a dropped or doubled row flips bit k of dbeta and is named; one marked
    row alone makes dgamma, dxsum, dbias bit-exact);
  * every output buffer is prefilled (NaN, or a sentinel behind the last row), every workspace is NaN-filled and every
    input has NaN rows behind its last row: an unwritten output, a slab row the kernel did not write or a row read past
    the end shows as a NaN or a changed sentinel.
"""
import ctypes
import math

import pytest
import torch

import rowops_reference as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = (torch.bfloat16, torch.float32)
PAD = 3                              # guard rows behind every input (NaN) and output (sentinel)
SENT = -1536.0                       # exact in bf16 and f32; no kernel writes it here
COL_SWEEP = (8, 128, 264, 512, 768, 1024, 1032, 1280, 1536, 1600, 2048, 3072, 4096)
WORST = {}                           # output -> (max |err| / bound, max |err|), printed at the end (pytest -s)


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    if WORST:
        print('\n[rowops] output: max |err| / (2 x model bound), max |err|')
        for k in sorted(WORST):
            print(f'[rowops] {k:34s} {WORST[k][0]:.3g}  {WORST[k][1]:.3g}')


def _lib():
    from lavila_amd import _cabi as C
    return C


def _p(t):
    if t is None:
        return None
    if t.numel() == 0:       # an empty view of a padded buffer: its (non-null) start, as the C ABI requires one
        return ctypes.c_void_p(t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size())
    return ctypes.c_void_p(t.data_ptr())


def _call(rc, what):
    _lib().check(rc, what)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), dtype=dtype, device=DEV)


def _padded(x):
    """x [rows, ...] in a buffer with PAD NaN rows behind it (the view handed to the kernel starts at the buffer)."""
    buf = _nan(x.shape[0] + PAD, *x.shape[1:], dtype=x.dtype)
    buf[:x.shape[0]] = x
    return buf[:x.shape[0]]


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _chunks(rows, cols):
    step = max(1, (1 << 25) // max(cols, 1))
    return [(r, min(r + step, rows)) for r in range(0, rows, step)]


def _within(name, got, want, bound, what=''):
    """|got - want| <= 2 bound elementwise (float64); records the worst ratio."""
    err = (got.double() - want).abs()
    ok = err <= 2 * bound
    if not bool(ok.all()):
        bad = (~ok).nonzero()[0].tolist()
        raise AssertionError(f'{name}{what}: {int((~ok).sum())} elements beyond 2x the model bound; first at {bad}: '
                             f'got {got[tuple(bad)].item()!r} want {want[tuple(bad)].item()!r} '
                             f'bound {2 * bound[tuple(bad)].item():.3g}')
    ratio = (err / (2 * bound).clamp_min(1e-300)).max().item() if err.numel() else 0.0
    w = WORST.get(name, (0.0, 0.0))
    WORST[name] = (max(w[0], ratio), max(w[1], err.max().item() if err.numel() else 0.0))


# ==== LayerNorm forward ====================================================================================================
FWD_PATHS = {            # name -> (x2, bias, keep_sum)
    'plain': (False, False, False),            # exact width: ln_fwd_exact_kernel<X2 = false>; else ln_fwd_kernel
    'x2_bias': (True, True, False),            # exact: ln_fwd_exact_kernel<true, true>
    'x2': (True, False, False),                # exact: ln_fwd_exact_kernel<true, false>
    'keep_sum': (True, True, True),            # ln_fwd_kernel<X2 = true> with s_out at every width
}


def _ln_inputs(rows, cols, dt, x2f, biasf, seed, low_var=True):
    """Random rows x ~ 2 N(0, 1) + 0.5, x2 ~ N(0, 1), bias ~ 0.1 N(0, 1); with low_var, rows r % 8 == 3 are constant
    (var = 0 up to the bias's bf16 remainder) and rows r % 8 == 6 have std 1e-3 (var ~ eps): an eps in the wrong place
    makes rstd inf (constant rows) or moves it by 30 %, an n - 1 divisor moves rstd by 1 / (2 cols)."""
    g = _gen(seed)
    x = 2 * torch.randn(rows, cols, generator=g, device=DEV) + 0.5
    x2 = torch.randn(rows, cols, generator=g, device=DEV) if x2f else None
    b = 0.1 * torch.randn(cols, generator=g, device=DEV) if biasf else None
    if low_var and rows:
        const = torch.tensor([0.75, -3.0, 0.0, 1.5, 12.0], device=DEV)
        r3 = torch.arange(3, max(rows, 3), 8, device=DEV)
        r6 = torch.arange(6, max(rows, 6), 8, device=DEV)
        c = const[r3 % 5][:, None].expand(-1, cols)
        small = 1e-3 * torch.randn(r6.numel(), cols, generator=g, device=DEV)
        if x2f:      # x = -bias, x2 = the low-variance row: (x + x2) + bias
            nb = (-b if b is not None else torch.zeros(cols, device=DEV)).to(dt).float()
            x[r3], x[r6] = nb, nb
            x2[r3], x2[r6] = c, small
        else:
            x[r3], x[r6] = c, small
    return (x.to(dt), x2.to(dt) if x2 is not None else None, b)


def _ln_fwd_case(path, dt, rows, cols, seed):
    C = _lib()
    x2f, biasf, keep = FWD_PATHS[path]
    eps = 1e-5 if seed % 2 else 1e-6
    x, x2, b = _ln_inputs(rows, cols, dt, x2f, biasf, seed)
    g = _gen(seed + 1)
    gamma = 1 + 0.2 * torch.randn(cols, generator=g, device=DEV)
    beta = 0.1 * torch.randn(cols, generator=g, device=DEV)
    x, x2 = _padded(x), (_padded(x2) if x2 is not None else None)
    y = torch.full((rows + PAD, cols), SENT, dtype=dt, device=DEV)
    s = torch.full((rows + PAD, cols), SENT, dtype=dt, device=DEV) if keep else None
    mean = torch.full((rows + PAD,), SENT, device=DEV)
    rstd = torch.full((rows + PAD,), SENT, device=DEV)
    _call(C.lib().lvl_layernorm_fwd(_p(x), _p(x2), _p(b), _p(gamma), _p(beta), _p(s), _p(y), _p(mean), _p(rstd), rows,
                                    cols, eps, C.dtype_code(x), C.stream_ptr()), 'lvl_layernorm_fwd')
    tag = f' [{path} {str(dt)[6:]} rows={rows} cols={cols}]'
    for name, t in (('y', y), ('s', s), ('mean', mean), ('rstd', rstd)):
        if t is not None:
            assert bool((t[rows:] == SENT).all()), f'{name}: a row behind the last one was written{tag}'
    n_add = (1 if x2f else 0) + (1 if biasf else 0)
    for r0, r1 in _chunks(rows, cols):
        if keep:     # the stored sum: bit-exact against the CPU f32 restatement (x + x2) + bias, rounded once
            want_s = R.ln_sum_f32(x[r0:r1].cpu(), x2[r0:r1].cpu(), b.cpu()).to(dt)
            got_s = s[r0:r1].cpu()
            assert torch.equal(got_s.view(torch.int16 if dt == torch.bfloat16 else torch.int32),
                               want_s.view(torch.int16 if dt == torch.bfloat16 else torch.int32)), f's not bit-exact{tag}'
            s64 = want_s.to(DEV).double()       # the kernel normalises the rounded sum it stored
            absum, na = s64.abs(), 0
        else:
            s64 = R.ln_sum64(x[r0:r1], x2[r0:r1] if x2f else None, b)
            absum = x[r0:r1].double().abs()
            if x2f:
                absum = absum + x2[r0:r1].double().abs()
            if biasf:
                absum = absum + b.double().abs()
            na = n_add
        y64, mu64, rs64 = R.ln_fwd_ref(s64, gamma, beta, eps)
        ey, emu, ers = R.ln_fwd_bounds(s64, absum, na, gamma, beta, eps, cols, dt)
        _within(f'ln_fwd y {str(dt)[6:]}', y[r0:r1], y64, ey, tag)
        _within('ln_fwd mean', mean[r0:r1], mu64, emu, tag)
        _within('ln_fwd rstd', rstd[r0:r1], rs64, ers, tag)


def _fwd_row_cases():
    out = []
    for path in FWD_PATHS:
        for rows in R.cap_sweep(R.ln_fwd_cap_rows(FWD_PATHS[path][0]), bench=True):
            out.append((path, 768, rows))
    for rows in R.cap_sweep(R.ln_fwd_cap_rows(False)):     # the general one-operand kernel (264 = 33 vectors of 8)
        out.append(('plain', 264, rows))
    return out


@pytest.mark.parametrize('dt', DTYPES, ids=str)
@pytest.mark.parametrize('path,cols,rows', _fwd_row_cases())
def test_layernorm_fwd_row_sweep(path, cols, rows, dt):
    _ln_fwd_case(path, dt, rows, cols, seed=rows + cols)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
@pytest.mark.parametrize('cols', COL_SWEEP)
def test_layernorm_fwd_column_sweep(cols, dt):
    """Every LN_DISPATCH arm (W = 8 with idle lanes at 8 columns, the 4096 maximum), one row past the cap."""
    paths = FWD_PATHS if R.ln_exact_width(cols) else ('plain', 'x2_bias', 'keep_sum')
    for path in paths:
        _ln_fwd_case(path, dt, R.ln_fwd_cap_rows(FWD_PATHS[path][0]) + 1, cols, seed=cols + 1)


# ==== LayerNorm backward ===================================================================================================
BWD_VARIANTS = {         # name -> (x2, bias, dadd, want_plain)
    'plain': (False, False, False, False),                 # bf16 exact-width: ln_bwd_exact_kernel<false, false, false>
    'dadd': (False, False, True, False),                   # <false, true, false>
    'x2_bias': (True, True, False, False),                 # <true, false, false>
    'x2_bias_dadd_plain': (True, True, True, True),        # <true, true, true>
    'x2_bias_dadd': (True, True, True, False),             # general kernel at every width
    'dadd_plain': (False, False, True, True),              # general kernel at every width
}


def _ln_bwd_run(dy, x, x2, b, gamma, mean, rstd, dadd, plain):
    """lvl_layernorm_bwd with NaN-prefilled outputs and a NaN workspace (the reduction may read only slab rows written
    by this launch)."""
    C = _lib()
    rows, cols = x.shape
    dt = x.dtype
    dx = _nan(rows, cols, dtype=dt)
    dxp = _nan(rows, cols, dtype=dt) if plain else None
    dgamma, dbeta, dxsum = _nan(cols), _nan(cols), _nan(cols)
    ws = _nan(int(C.lib().lvl_workspace_floats(b'layernorm_bwd', rows, cols)))
    _call(C.lib().lvl_layernorm_bwd(_p(dy), _p(x), _p(x2), _p(b), _p(gamma), _p(mean), _p(rstd), _p(dadd), _p(dx),
                                    _p(dxp), _p(dgamma), _p(dbeta), _p(dxsum), _p(ws), rows, cols, C.dtype_code(x),
                                    C.stream_ptr()), 'lvl_layernorm_bwd')
    return dx, dxp, dgamma, dbeta, dxsum


def _ln_bwd_check(tag, dt, out, dy, x, x2, b, gamma, mean, rstd, dadd, plain):
    """dx, dx_plain elementwise and dgamma / dbeta / dxsum against float64 (rowops_reference.ln_bwd_check)."""
    R.ln_bwd_check(_within, tag, dt, out, dy, x, x2, b, gamma, mean, rstd, dadd, plain)


def _ln_bwd_case(variant, dt, rows, cols, seed, marks=True):
    x2f, biasf, daddf, plain = BWD_VARIANTS[variant]
    x, x2, b = _ln_inputs(rows, cols, dt, x2f, biasf, seed, low_var=False)
    g = _gen(seed + 2)
    gamma = 1 + 0.2 * torch.randn(cols, generator=g, device=DEV)
    s64 = R.ln_sum64(x, x2, b) if rows else None
    if rows:
        _, mu, rs = R.ln_fwd_ref(s64, gamma, torch.zeros_like(gamma), 1e-6)     # f32 stats of a float64 forward
        mean, rstd = _padded(mu.float()), _padded(rs.float())
        del s64, mu, rs
    else:
        mean = rstd = torch.zeros(0, device=DEV)
    x, x2 = _padded(x), (_padded(x2) if x2f else None)
    tag = f' [{variant} {str(dt)[6:]} rows={rows} cols={cols}]'
    args = (x, x2, b, gamma, mean, rstd)

    # 1. integer fingerprint: dy in [-8, 8] (exact in bf16, column sums < 2^24): dbeta bit-exact; everything else vs f64
    dy = _padded(torch.randint(-8, 9, (rows, cols), generator=g, device=DEV).to(dt))
    dadd = _padded(torch.randn(rows, cols, generator=g, device=DEV).to(dt)) if daddf else None
    out = _ln_bwd_run(dy, *args[:3], gamma, mean, rstd, dadd, plain)
    if rows == 0:
        for name, t in zip(('dgamma', 'dbeta', 'dxsum'), out[2:]):
            assert torch.equal(t, torch.zeros_like(t)), f'{name} of zero rows is not exactly 0{tag}'
        return
    _ln_bwd_check(tag, dt, out, dy, x, x2, b, gamma, mean, rstd, dadd, plain)
    want = dy.double().sum(0)
    assert torch.equal(out[3].double(), want), \
        f'integer dbeta not exact{tag}: max diff {(out[3].double() - want).abs().max().item()}'
    if not marks:
        return

    # 2. marked rows: dy = 0 except on the boundary rows; marked row k carries +-2^-k -> dbeta bit-exact, a wrong bit
    # names the row; every unmarked row's dx_plain is exactly 0 and its dx exactly dadd (every row written in place)
    stride = R.ln_bwd_blocks(rows) * R.LN_ROWS_PER_BLOCK
    mk = R.mark_rows(rows, stride, R.LN_BWD_PARTS * R.LN_ROWS_PER_BLOCK)
    mrows = torch.tensor(mk, device=DEV)
    vals = R.mark_values(len(mk), cols, DEV, sign_seed=seed)
    dy = torch.zeros(rows, cols, device=DEV)
    dy[mrows] = vals
    dy = _padded(dy.to(dt))
    out = _ln_bwd_run(dy, x, x2, b, gamma, mean, rstd, dadd, plain)
    want = vals.double().sum(0)
    assert torch.equal(out[3].double(), want), f'marked dbeta: rows {R.decode_marks(out[3], want, mk)} lost or doubled{tag}'
    um = torch.ones(rows, dtype=torch.bool, device=DEV)
    um[mrows] = False
    want_dx = dadd[um] if dadd is not None else torch.zeros_like(dy[um])
    assert torch.equal(out[0][um].float(), want_dx.float()), f'unmarked rows: dx != dadd exactly{tag}'
    if plain:
        assert bool((out[1][um] == 0).all()), f'unmarked rows: dx_plain != 0{tag}'
    _ln_bwd_check(tag + ' marked', dt, out, dy, x, x2, b, gamma, mean, rstd, dadd, plain)

    # 3. one marked row alone: every other row adds exact zeros -> dgamma = fl(dy xhat) of that row (CPU f32 restatement,
    # same mean / rstd), dbeta = dy, dxsum = the kernel's own dx (dx_plain) row, bit for bit
    for m in sorted({rows - 1, min(rows - 1, stride)}):
        dy1 = torch.zeros(rows, cols, dtype=dt, device=DEV)
        dy1[m] = (torch.randn(cols, generator=g, device=DEV)).to(dt)
        dy1 = _padded(dy1)
        da1 = None
        if daddf:
            da1 = torch.zeros(rows, cols, dtype=dt, device=DEV)
            da1[m] = dadd[m]
            da1 = _padded(da1)
        dx, dxp, dgamma, dbeta, dxsum = _ln_bwd_run(dy1, x, x2, b, gamma, mean, rstd, da1, plain)
        s32 = R.ln_sum_f32(x[m].cpu(), x2[m].cpu() if x2f else None, b.cpu() if biasf else None)
        xh = (s32 - mean[m].cpu()) * rstd[m].cpu()
        assert torch.equal(dgamma.cpu(), dy1[m].float().cpu() * xh), f'single mark {m}: dgamma not bit-exact{tag}'
        assert torch.equal(dbeta, dy1[m].float()), f'single mark {m}: dbeta not bit-exact{tag}'
        assert torch.equal(dxsum, (dxp if plain else dx)[m].float()), f'single mark {m}: dxsum != own dx row{tag}'


def _bwd_row_cases():
    out = []
    rows = R.cap_sweep(R.LN_BWD_PARTS * R.LN_ROWS_PER_BLOCK, bench=True)
    for v in ('plain', 'dadd', 'x2_bias', 'x2_bias_dadd_plain'):          # bf16 exact width and the f32 general kernel
        for dt in DTYPES:
            out += [(v, dt, 768, r) for r in rows]
    for v in ('x2_bias_dadd', 'dadd_plain'):                              # other operand combinations
        out += [(v, torch.bfloat16, 768, r) for r in rows]
    for v in ('plain', 'x2_bias_dadd_plain'):                             # not an exact width
        out += [(v, torch.bfloat16, 1032, r) for r in rows]
    return out


@pytest.mark.parametrize('variant,dt,cols,rows', _bwd_row_cases(), ids=str)
def test_layernorm_bwd_row_sweep(variant, dt, cols, rows):
    _ln_bwd_case(variant, dt, rows, cols, seed=3 * rows + cols)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
@pytest.mark.parametrize('cols', COL_SWEEP)
def test_layernorm_bwd_column_sweep(cols, dt):
    for v in ('plain', 'x2_bias_dadd_plain'):
        _ln_bwd_case(v, dt, R.LN_BWD_PARTS * R.LN_ROWS_PER_BLOCK + 1, cols, seed=cols, marks=(cols in (8, 264, 4096)))


@pytest.mark.parametrize('variant', list(BWD_VARIANTS))
def test_layernorm_bwd_zero_rows(variant):
    """rows = 0: dgamma, dbeta, dxsum exactly 0 (one slab of zeros, NaN workspace around it)."""
    for dt in DTYPES:
        _ln_bwd_case(variant, dt, 0, 768, seed=1)


# ==== bias + QuickGELU =====================================================================================================
def _gelu_run(u, b, da):
    C = _lib()
    rows, cols = u.shape
    a = _nan(rows + PAD, cols, dtype=u.dtype)[:rows]        # never a null pointer, also at rows = 0
    _call(C.lib().lvl_bias_quickgelu_fwd(_p(u), _p(b), _p(a), rows, cols, C.dtype_code(u), C.stream_ptr()),
          'lvl_bias_quickgelu_fwd')
    du = _nan(rows + PAD, cols, dtype=u.dtype)[:rows]
    dbias = _nan(cols) if b is not None else None
    ws = _nan(int(C.lib().lvl_workspace_floats(b'bias_quickgelu_bwd', rows, cols))) if b is not None else None
    _call(C.lib().lvl_bias_quickgelu_bwd(_p(da), _p(u), _p(b), _p(du), _p(dbias), _p(ws), rows, cols, C.dtype_code(u),
                                         C.stream_ptr()), 'lvl_bias_quickgelu_bwd')
    return a, du, dbias


@pytest.mark.parametrize('dt', DTYPES, ids=str)
@pytest.mark.parametrize('with_bias', [True, False])
@pytest.mark.parametrize('cols', [8, 768, 1032, 2048, 3072, 4096])
def test_bias_quickgelu_past_the_caps(cols, with_bias, dt):
    """Forward a and backward du against float64 (the bound includes __expf and rcp), dbias against the float64 sum of
    the kernel's own du within the f32 accumulation bound, and the marked-row form: column c has one marked row
    m(c) = marks[c % n] (both sides of each cap, the unroll-group starts, first and last row), so dbias[c] must equal
    the kernel's du[m(c), c] bit for bit and every unmarked du must be exactly 0."""
    tagd = str(dt)[6:]
    for rows in R.gelu_rows(cols):
        tag = f' [{tagd} rows={rows} cols={cols} bias={with_bias}]'
        g = _gen(rows * 7 + cols)
        u = _padded((2 * torch.randn(rows, cols, generator=g, device=DEV)).to(dt))
        b = 0.5 * torch.randn(cols, generator=g, device=DEV) if with_bias else None
        da = _padded(torch.randn(rows, cols, generator=g, device=DEV).to(dt))
        a, du, dbias = _gelu_run(u, b, da)
        sb = torch.zeros(cols, dtype=torch.float64, device=DEV)
        ab = torch.zeros(cols, dtype=torch.float64, device=DEV)
        for r0, r1 in _chunks(rows, cols):
            a64, f64 = R.gelu_ref(u[r0:r1], b)
            ea, ef = R.gelu_bounds(u[r0:r1], b, dt)
            _within(f'gelu a {tagd}', a[r0:r1], a64, ea, tag)
            _within(f'gelu du {tagd}', du[r0:r1], da[r0:r1].double() * f64, R.gelu_du_bound(da[r0:r1], f64, ef, dt), tag)
            sb += du[r0:r1].double().sum(0)
            ab += du[r0:r1].double().abs().sum(0)
        if with_bias:
            _within('gelu dbias', dbias, sb, R.gelu_bwd_depth(rows) * R.U * ab, tag)
        # marked rows (one per column)
        gy = R.gelu_bwd_gy(rows)
        mk = R.mark_rows(rows, gy, R.GELU_BWD_ROW_BLOCKS, limit=64)
        mcol = torch.tensor(mk, device=DEV)[torch.arange(cols, device=DEV) % len(mk)]
        dam = torch.zeros(rows, cols, dtype=dt, device=DEV)
        cidx = torch.arange(cols, device=DEV)
        dam[mcol, cidx] = da[mcol, cidx]
        dam = _padded(dam)
        _, dum, dbm = _gelu_run(u, b, dam)
        marked = torch.zeros(rows, cols, dtype=torch.bool, device=DEV)
        marked[mcol, cidx] = True
        assert bool((dum[~marked] == 0).all()), f'marked: an unmarked du is not exactly 0{tag}'
        _within(f'gelu du {tagd}', dum[mcol, cidx], dam[mcol, cidx].double() * R.gelu_ref(u[mcol, cidx], b)[1],
                R.gelu_du_bound(dam[mcol, cidx], R.gelu_ref(u[mcol, cidx], b)[1], R.gelu_bounds(u[mcol, cidx], b, dt)[1],
                                dt), tag + ' marked')
        if with_bias:
            want = dum[mcol, cidx].float()
            bad = (dbm != want).nonzero().flatten().tolist()
            assert not bad, f'marked dbias != own du of the marked row at columns {bad[:8]} (rows {mcol[bad[:8]].tolist()}){tag}'


def test_bias_quickgelu_zero_rows_give_zero_dbias():
    for dt in DTYPES:
        u = _padded(torch.zeros(0, 768, dtype=dt, device=DEV))
        b = torch.randn(768, device=DEV)
        _, _, dbias = _gelu_run(u, b, u)
        assert torch.equal(dbias, torch.zeros_like(dbias))


# ==== qkv bias gradient ====================================================================================================
QKV_ROWS = sorted(set(R.cap_sweep(R.QKV_BIAS_ROW_BLOCKS)) | set(R.unroll_edges(R.QKV_BIAS_ROW_BLOCKS)) |
                  {4 * 4096 - 1, 4 * 4096, 4 * 4096 + 3})


@pytest.mark.parametrize('dt', DTYPES, ids=str)
@pytest.mark.parametrize('D', [512, 768, 1024, 1032])
def test_qkv_bias_grad_past_the_cap(D, dt):
    """Integer dq and dout rows: the q and v thirds are exact column sums, the k third exactly 0. The k and v thirds of
    dqkv are NaN (never read), so are the workspace and the output before the call."""
    C = _lib()
    for rows in QKV_ROWS:
        g = _gen(rows + D)
        dq = torch.randint(-8, 9, (rows, D), generator=g, device=DEV).to(dt)
        dqkv = _nan(rows, 3 * D, dtype=dt)
        dqkv[:, :D] = dq
        dqkv = _padded(dqkv)
        dout = _padded(torch.randint(-8, 9, (rows, D), generator=g, device=DEV).to(dt))
        db = _nan(3 * D)
        ws = _nan(int(C.lib().lvl_workspace_floats(b'qkv_bias_grad', rows, D)))
        _call(C.lib().lvl_qkv_bias_grad(_p(dqkv), _p(dout), _p(db), _p(ws), rows, D, C.dtype_code(dqkv), C.stream_ptr()),
              'lvl_qkv_bias_grad')
        tag = f' [{str(dt)[6:]} rows={rows} D={D}]'
        assert torch.equal(db[:D].double(), dq.double().sum(0)), f'q third not exact{tag}'
        assert bool((db[D:2 * D] == 0).all()) and not bool(torch.signbit(db[D:2 * D]).any()), f'k third not +0{tag}'
        assert torch.equal(db[2 * D:].double(), dout.double().sum(0)), f'v third not exact{tag}'


# ==== token assembly, patch gather, operand split ==========================================================================
@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_embed_tokens_fwd_past_the_grid_cap(dt):
    """B = 64 clips of 4 x 196 patches of 768: 4.8 M 8-wide work items, past grid_for's 16384 x 256. Bit-exact against the
    CPU f32 restatement in the kernel's order: pe + (pos + temporal) (cls: cls + pos[0]), one rounding."""
    C = _lib()
    B, F, N, D = 64, 4, 196, 768
    assert B * (1 + F * N) * (D // 8) > R.GRID_FOR_BLOCKS * R.GRID_FOR_THREADS
    g = _gen(64)
    pe = _padded(torch.randn(B, F * N, D, generator=g, device=DEV).to(dt))
    cls, pos, tem = (0.5 * torch.randn(*s, generator=g, device=DEV) for s in ((D,), (N + 1, D), (8, D)))
    x = torch.full((B + 1, 1 + F * N, D), SENT, dtype=dt, device=DEV)
    _call(C.lib().lvl_embed_tokens_fwd(_p(pe), _p(cls), _p(pos), _p(tem), _p(x), B, F, N, D, C.dtype_code(pe),
                                       C.stream_ptr()), 'lvl_embed_tokens_fwd')
    assert bool((x[B] == SENT).all()), 'a token behind the last clip was written'
    pc, posc, temc = pe.float().cpu(), pos.cpu(), tem.cpu()
    want = torch.empty(B, 1 + F * N, D)
    want[:, 0] = cls.cpu() + posc[0]
    want[:, 1:] = (pc.reshape(B, F, N, D) + (posc[1:][None] + temc[:F, None])[None]).reshape(B, F * N, D)
    assert torch.equal(x[:B].cpu().float(), want.to(dt).float())


@pytest.mark.parametrize('dt', DTYPES, ids=str)
@pytest.mark.parametrize('B', [1, 2, 3, 5, 63])
def test_embed_tokens_bwd_exact(B, dt):
    """Integer dx: d pos_embed, d temporal_embed (zero rows for frames >= F included: num_frames = 8 > F = 4) and
    d cls_token (= dpos[0]) exact. B < kEmbedBwdChunks leaves chunks empty, 3, 5, 63 do not divide into them. Outputs and
    workspace are NaN before the call."""
    C = _lib()
    F, N, D, nf = 4, 196, 768, 8
    g = _gen(B)
    dx = _padded(torch.randint(-8, 9, (B, 1 + F * N, D), generator=g, device=DEV).to(dt))
    dpos, dtem = _nan(N + 1, D), _nan(nf, D)
    ws = _nan(int(C.lib().lvl_embed_tokens_bwd_ws(F, N, D)))
    _call(C.lib().lvl_embed_tokens_bwd(_p(dx), _p(dpos), _p(dtem), _p(ws), B, F, N, D, nf, C.dtype_code(dx),
                                       C.stream_ptr()), 'lvl_embed_tokens_bwd')
    d = dx.double()
    body = d[:, 1:].reshape(B, F, N, D)
    assert torch.equal(dpos[0].double(), d[:, 0].sum(0)), 'd cls_token'
    assert torch.equal(dpos[1:].double(), body.sum((0, 1))), 'd pos_embed'
    assert torch.equal(dtem[:F].double(), body.sum((0, 2))), 'd temporal_embed'
    assert torch.equal(dtem[F:], torch.zeros_like(dtem[F:])), 'd temporal_embed of frames >= F'


@pytest.mark.parametrize('frame_major', [False, True])
@pytest.mark.parametrize('P,dt', [(16, torch.bfloat16), (16, torch.float32), (14, torch.bfloat16), (14, torch.float32)],
                         ids=['p16-bf16', 'p16-f32', 'p14-bf16', 'generic-f32'])
def test_patchify_past_the_grid_cap(P, dt, frame_major):
    """512 clips of 224^2 (P = 16: 4.8 M patch rows, P = 14 bf16: 5.5 M, the generic kernel (P = 14 f32): 77 M pixels)
    past grid_for's 16384 x 256 threads; bit-exact against oracle.patchify."""
    C = _lib()
    B, F, Ch, H = 128, 4, 3, 224
    g = _gen(P)
    video = torch.randn(B, F, Ch, H, H, generator=g, device=DEV) if frame_major else \
        torch.randn(B, Ch, F, H, H, generator=g, device=DEV)
    threads = B * Ch * F * H * (H // P if (P == 16 or dt == torch.bfloat16) else H)
    assert threads > R.GRID_FOR_BLOCKS * R.GRID_FOR_THREADS
    N = (H // P) ** 2
    out = torch.full((B + 1, F * N, Ch * P * P), SENT, dtype=dt, device=DEV)
    _call(C.lib().lvl_patchify(_p(video), _p(out), B, Ch, F, H, H, P, int(frame_major), C.dtype_code(out),
                               C.stream_ptr()), 'lvl_patchify')
    assert bool((out[B] == SENT).all()), 'a patch row behind the last clip was written'
    want = O.patchify(video.permute(0, 2, 1, 3, 4) if frame_major else video, P).to(dt)
    assert torch.equal(out[:B], want)


@pytest.mark.parametrize('stack', [False, True])
@pytest.mark.parametrize('role', [0, 1])
@pytest.mark.parametrize('cols', [96, 1028])
def test_split3_past_the_row_cap(cols, role, stack):
    """lvl_split_bf16x3 at 16384 +- 1 and 2 x 16384 + 3 rows: exactly h = bf16(x), l = bf16(x - h) in the term order of
    the role, side by side ([R, 3C]) or stacked ([3R, C]); every element written (NaN before the call)."""
    C = _lib()
    for rows in (R.SPLIT_ROW_BLOCKS - 1, R.SPLIT_ROW_BLOCKS, R.SPLIT_ROW_BLOCKS + 1, 2 * R.SPLIT_ROW_BLOCKS + 3):
        g = _gen(rows + cols + role)
        x = torch.randn(rows, cols, generator=g, device=DEV) * \
            torch.exp2(torch.randint(-20, 21, (rows, cols), generator=g, device=DEV).float())
        x[::97, 5] = float('inf')
        x[1::89, 3] = -float('inf')
        x = _padded(x)
        if stack:
            out = _nan(3 * rows, cols, dtype=torch.bfloat16)
            rs, ts = cols, rows * cols
        else:
            out = _nan(rows, 3 * cols, dtype=torch.bfloat16)
            rs, ts = 3 * cols, cols
        _call(C.lib().lvl_split_bf16x3(_p(x), _p(out), rows, cols, cols, rs, ts, role, C.stream_ptr()),
              'lvl_split_bf16x3')
        h, l = R.split3_ref(x)
        terms = (h, h, l) if role == 0 else (h, l, h)
        got = out.reshape(3, rows, cols) if stack else out.reshape(rows, 3, cols).transpose(0, 1)
        for t in range(3):
            assert torch.equal(got[t].view(torch.int16), terms[t].view(torch.int16)), (rows, t)


# ==== the framework wrappers on a NaN workspace ============================================================================
def test_wrappers_on_a_nan_workspace_equal_the_direct_calls(monkeypatch):
    """ops.layernorm_bwd_raw, ops.bias_quick_gelu's backward and ops._qkv_bias_grad take their workspace from
    lavila_amd._cabi.workspace (torch.empty): filled with NaN it must not change any result bit."""
    from lavila_amd import _cabi as C
    from lavila_amd import ops
    real = C.workspace
    monkeypatch.setattr(C, 'workspace', lambda *a, **k: real(*a, **k).fill_(float('nan')))
    rows, cols = 3 * R.LN_BWD_PARTS * R.LN_ROWS_PER_BLOCK + 5, 768
    g = _gen(5)
    x = torch.randn(rows, cols, generator=g, device=DEV).bfloat16()
    dy, dadd = torch.randn_like(x), torch.randn_like(x)
    gamma, beta = torch.randn(cols, generator=g, device=DEV), torch.randn(cols, generator=g, device=DEV)
    _, _, mean, rstd = ops.layernorm_fwd_raw(x, None, None, gamma, beta, 1e-6, False)
    got = ops.layernorm_bwd_raw(dy, x, None, None, gamma, mean, rstd, dadd, True, True)
    want = _ln_bwd_run(dy, x, None, None, gamma, mean, rstd, dadd, True)
    for a, b in zip((got[0], got[4], got[1], got[2], got[3]), want):
        assert torch.equal(a, b)
    u = torch.randn(rows, 3072, generator=g, device=DEV).bfloat16().requires_grad_(True)
    bias = torch.randn(3072, generator=g, device=DEV).requires_grad_(True)
    da = torch.randn(rows, 3072, generator=g, device=DEV).bfloat16()
    a = ops.bias_quick_gelu(u, bias)
    a.backward(da)
    a2, du2, db2 = _gelu_run(u.detach(), bias.detach(), da)
    assert torch.equal(a, a2) and torch.equal(u.grad, du2) and torch.equal(bias.grad, db2)
    dqkv = torch.randn(rows, 3 * cols, generator=g, device=DEV).bfloat16()
    dout = torch.randn(rows, cols, generator=g, device=DEV).bfloat16()
    db = ops._qkv_bias_grad(dqkv, dout, torch.float32)
    ws = _nan(int(C.lib().lvl_workspace_floats(b'qkv_bias_grad', rows, cols)))
    db2 = _nan(3 * cols)
    _call(C.lib().lvl_qkv_bias_grad(_p(dqkv), _p(dout), _p(db2), _p(ws), rows, cols, C.LVL_BF16, C.stream_ptr()), 'qkv')
    assert torch.equal(db, db2)
    assert not math.isnan(db.sum().item())
