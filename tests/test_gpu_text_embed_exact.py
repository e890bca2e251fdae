"""GPU (-m gpu): lvl_text_embed_fwd / lvl_text_embed_bwd (csrc/text_embed.hip) through the C ABI at every width the three
text towers use and at every branch of the table kernel's scan, against the float64 reference of
tests/text_embed_reference.py; then the autograd wrapper ops.text_embed at its edges.

The cases (text_embed_reference.CASES; what each reaches is printed and asserted by tests/test_text_embed_reference_cpu.py)
put a width on each side of every column-group and pass boundary (512 / 1024 / 1536), R = B L at 1, 63, 64, 65, 512, 513 and
beyond, and token patterns that are formulas, not draws.

  forward            x == (table[tokens] + pos[:L]).to(dtype) to the bit: one float32 add, one rounding.
  backward, exact    dx holds integers in [-8, 8] (exact in bfloat16); with at most 4096 rows every partial sum in any order
                     is an integer below 2^15, so dtable and dpos must EQUAL the float64 sums. A dropped, doubled or
                     misattributed row, column group or window changes an integer.
  backward, random   every element within n 2^-24 sum|dx_i| of the float64 sum, n its number of terms: the first-order bound
                     of an n-term float32 sum in any order ((n - 1) u sum|x| with u = 2^-24; n for the higher-order terms).
                     Nothing in the bound is measured. A second call into fresh buffers is bit-identical.

Every output is a view into a larger buffer filled with NaN, GUARD elements before and behind it, and the int32 workspace is
followed by 64 sentinel words; every launch asserts them untouched. Token ids are always inside [0, V): the kernels' clamp of
other ids is memory safety, read in the source and not exercised on a device.
"""
import ctypes
import functools

import pytest
import torch

import text_embed_reference as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ('f32', 'bf16')
GUARD = 512                      # elements of NaN before and behind every output (keeps the view 16-byte aligned)
WS_GUARD = 64
DX_GUARD_ROWS = 576              # 8 waves x 64 rows + 64: as far as eight rounded-up ranges can reach past R
SENTINEL = 0x5a5a5a5a
EINVAL = -22
_id = lambda c: '-'.join(map(str, c))            # noqa: E731


def _C():
    from lavila_amd import _cabi as C
    return C


def _code(dt):
    C = _C()
    return C.LVL_F32 if dt == torch.float32 else C.LVL_BF16


def _guarded(n, dt):
    buf = torch.full((n + 2 * GUARD,), float('nan'), dtype=dt, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def _device_dx(dx, dt):
    """dx [B, L, W] on the device in dtype dt, with DX_GUARD_ROWS rows of NaN behind it: a scan that ran past row R (the
    words behind the token list in the workspace are first[]: text_embed_reference.overrun_matches) would add a NaN row."""
    B, L, W = dx.shape
    buf = torch.full(((B * L + DX_GUARD_ROWS) * W,), float('nan'), dtype=dt, device=DEV)
    buf[:B * L * W] = dx.reshape(-1).to(DEV, dt)
    return buf[:B * L * W].reshape(B, L, W)


def _device_tokens(tokens, stride):
    """The [B, L] view the kernels read in place and the tensor that owns its memory."""
    full = R.strided_tokens(tokens, stride).to(DEV)
    view = full[:, :tokens.shape[1]]
    assert view.stride(1) == 1 and (view.shape[0] == 1 or view.stride(0) == stride)
    return full, view


def _fwd(view, stride, table, pos, dt):
    C = _C()
    (B, L), (V, W) = view.shape, table.shape
    buf, x = _guarded(B * L * W, dt)
    rc = C.lib().lvl_text_embed_fwd(C.ptr(view), stride, C.ptr(table), C.ptr(pos), C.ptr(x), B, L, W, V, _code(dt),
                                    C.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, C.lib().lvl_last_error()
    assert _guards_intact(buf)
    return x.reshape(B, L, W)


def _bwd(dx, view, stride, V, ctx, want_table=True, want_pos=True):
    """One lvl_text_embed_bwd into fresh NaN-filled, guarded buffers -> (dtable [V, W] | None, dpos [ctx, W] | None, ws)."""
    C = _C()
    B, L, W = dx.shape
    tbuf, dtable = _guarded(V * W, torch.float32) if want_table else (None, None)
    pbuf, dpos = _guarded(ctx * W, torch.float32) if want_pos else (None, None)
    n_ws = int(C.lib().lvl_text_embed_bwd_ws(B, L, V))
    assert n_ws == B * L + 2 * V
    ws = torch.full((n_ws + WS_GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    rc = C.lib().lvl_text_embed_bwd(C.ptr(dx), C.ptr(view), stride, C.ptr(dtable), C.ptr(dpos), C.ptr(ws), B, L, W, V, ctx,
                                    _code(dx.dtype), C.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, C.lib().lvl_last_error()
    assert bool((ws[n_ws:] == SENTINEL).all()), 'workspace guard words overwritten'
    for buf in (tbuf, pbuf):
        assert buf is None or _guards_intact(buf)
    return (dtable.reshape(V, W) if want_table else None, dpos.reshape(ctx, W) if want_pos else None, ws[:n_ws])


@functools.lru_cache(maxsize=None)
def _case(i):
    """The CPU side of case i, computed once and shared by the tests (never modified)."""
    B, L, ctx, V, W, name, stride = R.CASES[i]
    g = torch.Generator().manual_seed(100 + i)
    tokens = R.pattern(name, B, L, V)
    table, pos = torch.randn(V, W, generator=g), torch.randn(ctx, W, generator=g)
    dxi = R.integer_dx(B, L, W)
    _, dtable, dpos = R.reference(tokens, table, pos, dxi)
    return dict(B=B, L=L, ctx=ctx, V=V, W=W, stride=stride, tokens=tokens, table=table, pos=pos, dxi=dxi,
                dxr=torch.randn(B, L, W, generator=g), dtable_int=dtable, dpos_int=dpos, ids=torch.unique(tokens))


CASE_IDS = [_id(c) for c in R.CASES]


@pytest.mark.parametrize('dt', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('i', range(len(R.CASES)), ids=CASE_IDS)
def test_forward_to_the_bit(i, dt):
    c = _case(i)
    full, view = _device_tokens(c['tokens'], c['stride'])
    x = _fwd(view, c['stride'], c['table'].to(DEV), c['pos'].to(DEV), dt)
    want = (c['table'][c['tokens']] + c['pos'][:c['L']]).to(dt)             # float32 on the CPU: one add, one rounding
    assert torch.equal(x.cpu(), want)


def _assert_exact_backward(c, dtable, dpos):
    ids, L = c['ids'], c['L']
    if dtable is not None:
        dtable = dtable.cpu()
        assert torch.equal(dtable[ids], c['dtable_int'][ids].float())
        # rows of ids that do not occur are exact zeros (a NaN left behind or a stray write counts as non-zero)
        assert int(torch.count_nonzero(dtable)) == int(torch.count_nonzero(dtable[ids]))
        assert torch.equal(dtable, c['dtable_int'].float())
    if dpos is not None:
        dpos = dpos.cpu()
        assert torch.equal(dpos[:L], c['dpos_int'][:L].float())
        assert int(torch.count_nonzero(dpos[L:])) == 0


@pytest.mark.parametrize('dt', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('i', range(len(R.CASES)), ids=CASE_IDS)
def test_backward_integer_operands_exact(i, dt):
    c = _case(i)
    full, view = _device_tokens(c['tokens'], c['stride'])
    dx = _device_dx(c['dxi'], dt)
    assert torch.equal(dx.float().cpu(), c['dxi'])                           # the integers survive the cast
    dtable, dpos, ws = _bwd(dx, view, c['stride'], c['V'], c['ctx'])
    _assert_exact_backward(c, dtable, dpos)
    assert torch.equal(ws[:c['B'] * c['L']].cpu(), c['tokens'].reshape(-1).int())      # the census' token list


@pytest.mark.parametrize('dt', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('i', range(len(R.CASES)), ids=CASE_IDS)
def test_backward_random_within_summation_bound(i, dt):
    c = _case(i)
    B, L, V, W, ctx = c['B'], c['L'], c['V'], c['W'], c['ctx']
    full, view = _device_tokens(c['tokens'], c['stride'])
    dx = _device_dx(c['dxr'], dt)
    d = dx.cpu().double()                                                    # what the kernel reads: dx rounded to dt
    _, ref_t, ref_p = R.reference(c['tokens'], c['table'], c['pos'], d)
    flat = c['tokens'].reshape(-1)
    abs_t = torch.zeros(V, W, dtype=torch.float64).index_add_(0, flat, d.abs().reshape(-1, W))
    n_t = torch.bincount(flat, minlength=V).double()[:, None]
    u = 2.0 ** -24
    bound_t = n_t * u * abs_t
    bound_p = torch.zeros(ctx, W, dtype=torch.float64)
    bound_p[:L] = B * u * d.abs().sum(0)
    dtable, dpos, _ = _bwd(dx, view, c['stride'], V, ctx)
    err_t, err_p = (dtable.cpu().double() - ref_t).abs(), (dpos.cpu().double() - ref_p).abs()
    worst = max(float((e[b > 0] / b[b > 0]).max()) if bool((b > 0).any()) else 0.0
                for e, b in ((err_t, bound_t), (err_p, bound_p)))
    print(f'[text_embed bwd {R.CASES[i]} {dt}] worst error / derived bound {worst:.3f}')
    assert bool((err_t <= bound_t).all()) and bool((err_p <= bound_p).all())
    again_t, again_p, _ = _bwd(dx, view, c['stride'], V, ctx)                # fresh NaN-filled buffers
    assert torch.equal(again_t, dtable) and torch.equal(again_p, dpos)


@pytest.mark.parametrize('case', R.LARGE_CASES, ids=_id)
def test_full_sized_tables(case):
    """GPT-2 XL's tied table (V = 50257, W = 1600, 1024 positions) and DistilBERT's (V = 30522, W = 768, 512 positions), bf16:
    forward to the bit against torch's own gather on the device, integer backward equal to float64 on the rows that occur,
    every other row of the [V, W] gradient an exact zero. No float64 [V, W] reference is built."""
    B, L, ctx, V, W, name, stride = case
    dt = torch.bfloat16
    tokens = R.pattern(name, B, L, V)
    assert int(tokens.max()) == V - 1 and int(tokens.min()) == 0            # the first and the last row of the table
    full, view = _device_tokens(tokens, stride)
    g = torch.Generator(device=DEV).manual_seed(7)
    table = torch.randn(V, W, generator=g, device=DEV)
    pos = torch.randn(ctx, W, generator=g, device=DEV)
    x = _fwd(view, stride, table, pos, dt)
    assert torch.equal(x, (table[view] + pos[:L]).to(dt))
    del table, x
    dxi = R.integer_dx(B, L, W)
    ids, rows, counts = R.occurring_rows(tokens, dxi)
    dtable, dpos, _ = _bwd(_device_dx(dxi, dt), view, stride, V, ctx)
    got = dtable[ids.to(DEV)]
    assert torch.equal(got.cpu(), rows.float())
    assert int(torch.count_nonzero(dtable)) == int(torch.count_nonzero(got))
    assert torch.equal(dpos[:L].cpu(), dxi.double().sum(0).float())
    assert int(torch.count_nonzero(dpos[L:])) == 0


# ----------------------------------------------------------------------------------------------------------------------
# argument checks and the nullable outputs of lvl_text_embed_bwd
# ----------------------------------------------------------------------------------------------------------------------
def _off(t, nbytes):
    return ctypes.c_void_p(t.data_ptr() + nbytes)


def test_bad_arguments_return_einval_and_write_nothing():
    C = _C()
    lib = C.lib()
    B, L, ctx, V, W = 2, 3, 4, 5, 8
    big = 2056                                                               # every buffer is large enough for the widest call
    tok = torch.zeros(B, ctx, dtype=torch.int64, device=DEV)
    table, pos = torch.zeros(V, big, device=DEV), torch.zeros(ctx, big, device=DEV)
    for dt in DTYPES:
        nan = lambda n, d=torch.float32: torch.full((n,), float('nan'), dtype=d, device=DEV)      # noqa: E731
        dx, x = nan(B * L * big + 16, dt), nan(B * L * big + 16, dt)
        dtable, dpos = nan(V * big + 16), nan(ctx * big + 16)
        ws = torch.full((B * L + 2 * V + WS_GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        code, st = _code(dt), C.stream_ptr()
        p = C.ptr
        bwd = dict(dx=p(dx), tokens=p(tok), stride=ctx, dtable=p(dtable), dpos=p(dpos), ws=p(ws), B=B, L=L, W=W, V=V, ctx=ctx)
        bad_bwd = {
            'W % 8 != 0': dict(W=12), 'W > 2048': dict(W=big), 'ctx < L': dict(ctx=L - 1), 'tok_stride < L': dict(stride=L - 1),
            'dtable misaligned': dict(dtable=_off(dtable, 4)), 'dpos misaligned': dict(dpos=_off(dpos, 8)),
            'dx misaligned': dict(dx=_off(dx, 8)), 'dx null': dict(dx=None), 'tokens null': dict(tokens=None),
            'both outputs null': dict(dtable=None, dpos=None), 'ws null with a dtable': dict(ws=None),
            'B = 0': dict(B=0), 'unknown dtype': dict(code=7),
        }
        for what, change in bad_bwd.items():
            a = {**bwd, 'code': code, **change}
            rc = lib.lvl_text_embed_bwd(a['dx'], a['tokens'], a['stride'], a['dtable'], a['dpos'], a['ws'], a['B'], a['L'],
                                        a['W'], a['V'], a['ctx'], a['code'], st)
            assert rc == EINVAL, (what, rc)
        fwd = dict(tokens=p(tok), stride=ctx, table=p(table), pos=p(pos), x=p(x), W=W)
        bad_fwd = {'W % 4 != 0': dict(W=6), 'tok_stride < L': dict(stride=L - 1), 'x null': dict(x=None),
                   'tokens null': dict(tokens=None), 'table null': dict(table=None), 'pos null': dict(pos=None),
                   'table misaligned': dict(table=_off(table, 4)), 'x misaligned': dict(x=_off(x, 2))}
        for what, change in bad_fwd.items():
            a = {**fwd, **change}
            rc = lib.lvl_text_embed_fwd(a['tokens'], a['stride'], a['table'], a['pos'], a['x'], B, L, a['W'], V, code, st)
            assert rc == EINVAL, (what, rc)
        torch.cuda.synchronize()
        for t in (x, dtable, dpos):
            assert bool(torch.isnan(t).all())                                # the prefilled outputs keep their NaNs
        assert bool((ws == SENTINEL).all())


NULLABLE = [4, 13]               # seven ragged captions at W = 520 and at W = 2040


@pytest.mark.parametrize('dt', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('i', NULLABLE, ids=[CASE_IDS[i] for i in NULLABLE])
def test_null_dtable_or_null_dpos_leaves_the_other_output_exact(i, dt):
    c = _case(i)
    full, view = _device_tokens(c['tokens'], c['stride'])
    dx = _device_dx(c['dxi'], dt)
    none, dpos, ws = _bwd(dx, view, c['stride'], c['V'], c['ctx'], want_table=False)
    assert none is None
    _assert_exact_backward(c, None, dpos)
    assert bool((ws == SENTINEL).all())                                      # no init, no census: the workspace is not touched
    dtable, none, ws = _bwd(dx, view, c['stride'], c['V'], c['ctx'], want_pos=False)
    assert none is None
    _assert_exact_backward(c, dtable, None)
    # a null dtable needs no workspace either
    C = _C()
    pbuf, dpos2 = _guarded(c['ctx'] * c['W'], torch.float32)
    rc = C.lib().lvl_text_embed_bwd(C.ptr(dx), C.ptr(view), c['stride'], None, C.ptr(dpos2), None, c['B'], c['L'], c['W'],
                                    c['V'], c['ctx'], _code(dt), C.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and _guards_intact(pbuf) and torch.equal(dpos2.reshape(c['ctx'], c['W']), dpos)


# ----------------------------------------------------------------------------------------------------------------------
# ops.text_embed under autograd
# ----------------------------------------------------------------------------------------------------------------------
def _record(monkeypatch, name):
    """Replaces an entry point of the loaded library by a wrapper that records its arguments and forwards."""
    lib = _C().lib()
    real = getattr(lib, name)
    calls = []

    def forward(*a):
        calls.append(a)
        return real(*a)
    monkeypatch.setattr(lib, name, forward)
    return calls


def _is_null(p):
    return p is None or (isinstance(p, ctypes.c_void_p) and not p.value)


def _params(V, W, ctx, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(V, W, generator=g).to(DEV).requires_grad_(True), torch.randn(ctx, W, generator=g).to(DEV).requires_grad_(True),
            g)


def test_in_place_write_to_the_tokens_before_backward_raises():
    from lavila_amd import ops
    table, pos, _ = _params(16, 8, 4)
    text = R.pattern('tail_pair', 2, 3, 16).to(DEV)
    x = ops.text_embed(text, table, pos, torch.float32)
    text.add_(0)
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        x.sum().backward()


@pytest.mark.parametrize('dt', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('frozen', ['table', 'pos'])
def test_frozen_parameter_gets_a_null_pointer_and_no_gradient(frozen, dt, monkeypatch):
    from lavila_amd import ops
    B, L, ctx, V, W = 7, 9, 16, 64, 520
    table, pos, g = _params(V, W, ctx)
    text = R.strided_tokens(R.pattern('captions', B, L, V), ctx).to(DEV)[:, :L]
    up = torch.randn(B, L, W, generator=g).to(DEV)
    (ops.text_embed(text, table, pos, dt).float() * up).sum().backward()
    want = {'table': table.grad.clone(), 'pos': pos.grad.clone()}
    table.grad = pos.grad = None
    (table if frozen == 'table' else pos).requires_grad_(False)
    calls = _record(monkeypatch, 'lvl_text_embed_bwd')
    x = ops.text_embed(text, table, pos, dt)
    (x.float() * up).sum().backward()
    assert len(calls) == 1
    dtable_arg, dpos_arg, ws_arg = calls[0][3], calls[0][4], calls[0][5]
    if frozen == 'table':
        assert _is_null(dtable_arg) and _is_null(ws_arg) and not _is_null(dpos_arg)
        assert table.grad is None and torch.equal(pos.grad, want['pos'])
    else:
        assert _is_null(dpos_arg) and not _is_null(dtable_arg) and not _is_null(ws_arg)
        assert pos.grad is None and torch.equal(table.grad, want['table'])


def _forward_backward(text, table, pos, up, dt):
    from lavila_amd import ops
    table.grad = pos.grad = None
    x = ops.text_embed(text, table, pos, dt)
    assert x is not None
    (x.float() * up).sum().backward()
    return x.detach(), table.grad.clone(), pos.grad.clone()


@pytest.mark.parametrize('layout', ['expand', 'expand_row', 'column_t', 'view', 'view_one_row'])
def test_token_layouts_nn_embedding_accepts_never_raise(layout):
    """B = 1 is read with stride L whatever torch reports for the size-1 dimension; a batch whose rows overlap (row stride
    below L) is read from a contiguous copy; `[:, :L]` views are read in place. Each gives the bits of the contiguous call."""
    B, L, ctx, V, W, dt = 3, 5, 9, 32, 16, torch.bfloat16
    table, pos, g = _params(V, W, ctx)
    ids = (torch.arange(L) * 7 + 3) % V
    if layout == 'expand':
        text = ids.to(DEV).expand(B, L)
        assert text.stride() == (0, 1)
    elif layout == 'expand_row':
        text = ids.to(DEV)[None].expand(B, L)
        assert text.stride(0) == 0
    elif layout == 'column_t':
        text = ids.to(DEV).reshape(L, 1).t()
        assert text.shape == (1, L) and text.stride() == (1, 1)
    elif layout == 'view':
        text = R.strided_tokens(R.pattern('captions', B, L, V), ctx).to(DEV)[:, :L]
        assert text.stride() == (ctx, 1)
    else:
        text = R.strided_tokens(R.pattern('captions', 1, L, V), ctx).to(DEV)[:, :L]
    up = torch.randn(text.shape[0], L, W, generator=g).to(DEV)
    got = _forward_backward(text, table, pos, up, dt)
    want = _forward_backward(text.contiguous(), table, pos, up, dt)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert torch.equal(got[0], (torch.nn.functional.embedding(text, table) + pos[:L]).detach().to(dt))


@pytest.mark.parametrize('what', ['int32 tokens', 'bf16 table', 'W % 8 != 0', 'W > 2048', 'too few positions',
                                  'non-unit inner stride'])
def test_ineligible_inputs_return_none_and_launch_nothing(what, monkeypatch):
    from lavila_amd import ops
    B, L, ctx, V, W = 2, 4, 8, 16, 16
    if what == 'W % 8 != 0':
        W = 12
    if what == 'W > 2048':
        W = 2056
    if what == 'too few positions':
        ctx = L - 1
    table, pos = torch.zeros(V, W, device=DEV), torch.zeros(ctx, W, device=DEV)
    text = torch.zeros(B, 2 * L, dtype=torch.int64, device=DEV)[:, :L]
    if what == 'int32 tokens':
        text = text.int()
    if what == 'bf16 table':
        table = table.bfloat16()
    if what == 'non-unit inner stride':
        text = torch.zeros(B, 2 * L, dtype=torch.int64, device=DEV)[:, ::2]
        assert text.shape == (B, L) and text.stride(1) == 2
    calls = _record(monkeypatch, 'lvl_text_embed_fwd')
    assert ops.text_embed(text, table, pos, torch.float32) is None
    assert calls == []
    if what != 'too few positions':                                          # what the caller then keeps does work
        torch.nn.functional.embedding(text, table) + pos[:L]
