"""GPU (-m gpu): the GEMMs of a decoder whose widths are multiples of 64 but not of 256 (GPT-2 XL: 1600 / 3200 / 4800).

  * lvl_linear_tn_ragged = lvl_linear_tn's persistent kernel over the full 256-column tiles + the edge kernel
    (csrc/gemm_tn_edge.hip) over the 64 / 128 / 192 columns behind them: exact on small integers, bit-identical repeats,
    the full-tile columns bit-equal to what lvl_linear_tn computes for W[:N0], nothing read or written out of bounds,
    the real XL shapes within the bf16 bound, loud refusals;
  * lvl_linear_wgrad's 160-family tiles (5x5 and 8x5 MFMA tiles per wave): exact on small integers with and without
    dbias on both schedules (the plans of every earlier shape: tests/test_gemm_ragged_cpu.py).

Integer data: every product and partial sum is an integer far below 2^24 (exact in f32 in any summation order). For the TN
GEMM the RESULT must also be a bf16 number: an activation row has 48 non-zero entries in {-2..2}, the weights are in
{-2..2} and the bias in {-3..3}, so |y| <= 48 * 4 + 3 = 195 < 256 (every integer up to 256 is a bf16 number)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF = torch.bfloat16
SENT16 = 0x7FA5           # a NaN payload nobody computes: the guard pattern of output buffers

RAGGED_N = (64, 128, 192, 320, 448, 640, 960)       # zero, one and several full column tiles under each remainder
RAGGED_K = (64, 192, 320, 1600)                     # 1 K block (static schedule), 3, 5 (= DYN_MIN_NB: dynamic), 25
RAGGED_M = (1, 255, 256, 257, 300, 513)


def _ragged(x, w, bias, y, sched, epilogue=0, dtype=None):
    from lavila_amd import _cabi as C
    M, K = x.shape
    N = w.shape[0]
    blk = torch.zeros(16, dtype=torch.int32, device=DEV) if sched else None
    C.check(C.lib().lvl_linear_tn_ragged(C.ptr(x), C.ptr(w), C.ptr(bias), C.ptr(y), C.ptr(blk), M, N, K, epilogue,
                                         C.LVL_BF16 if dtype is None else dtype, C.stream_ptr()), 'lvl_linear_tn_ragged')
    if blk is not None:
        torch.cuda.synchronize()
        assert int(blk.abs().sum()) == 0, blk.tolist()          # the kernel leaves the counter block zeroed
    return y


def _int_problem(M, N, K, g):
    """x [M,K] with 48 non-zero entries per row (every K block is hit by some row), w [N,K], bias [N]: small integers"""
    x = torch.randint(-2, 3, (M, K), generator=g)
    keep = torch.rand(M, K, generator=g).argsort(1) < 48
    x = x * keep
    w = torch.randint(-2, 3, (N, K), generator=g)
    b = torch.randint(-3, 4, (N,), generator=g)
    return x.to(DEV).to(BF), w.to(DEV).to(BF), b.to(DEV).float()


@pytest.mark.parametrize('N', RAGGED_N)
def test_ragged_tn_exact_on_integers(N):
    g = torch.Generator().manual_seed(1000 + N)
    worst = 0
    for K in RAGGED_K:
        for M in RAGGED_M:
            x, w, b = _int_problem(M, N, K, g)
            want0 = x.double() @ w.double().t()
            for bias in (b, None):
                want = want0 if bias is None else want0 + bias.double()
                worst = max(worst, int(want.abs().max()))
                assert want.abs().max() <= 256
                for sched in (False, True):
                    runs = []
                    for _ in range(2):
                        y = torch.empty(M, N, dtype=BF, device=DEV)
                        y.view(torch.int16).fill_(SENT16)
                        runs.append(_ragged(x, w, bias, y, sched))
                    assert torch.equal(runs[0].double(), want), (M, N, K, bias is not None, sched)
                    assert torch.equal(runs[0], runs[1]), (M, N, K, bias is not None, sched)
    print(f'[ragged tn exact N={N}] {len(RAGGED_K) * len(RAGGED_M) * 4} problems x 2 runs equal to float64; max |y| {worst}')


@pytest.mark.parametrize('N', [320, 960])
def test_ragged_full_tile_columns_are_the_main_kernels(N):
    """Y[:, :N0] of the ragged call == lvl_linear_tn on W[:N0], bit for bit, on random bf16 data: the persistent kernel
    runs the launch it always ran, only its output stride differs."""
    from lavila_amd import ops
    g = torch.Generator().manual_seed(2000 + N)
    N0 = N // 256 * 256
    for M, K in ((300, 320), (513, 64), (257, 1600)):
        x = torch.randn(M, K, generator=g).to(DEV).to(BF)
        w = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV).to(BF)
        b = torch.randn(N, generator=g).to(DEV)
        for bias in (b, None):
            for sched in (False, True):
                y = _ragged(x, w, bias, torch.empty(M, N, dtype=BF, device=DEV), sched)
                ref = ops.linear_tn_raw(x, w[:N0].contiguous(), None if bias is None else bias[:N0].contiguous())
                assert torch.equal(y[:, :N0], ref), (M, N, K, bias is not None, sched)
                want = x.double() @ w.double().t() + (0 if bias is None else bias.double())
                assert (y.double() - want).abs().max() <= 2.0 ** -7 * want.abs().max()


def _carved(t, guard=4096):
    """t as the middle of a larger buffer whose guard regions (before and after) are NaN; 16-byte alignment kept"""
    n = t.numel()
    buf = torch.full((guard + n + guard,), float('nan'), dtype=t.dtype, device=DEV)
    buf[guard:guard + n] = t.reshape(-1)
    return buf[guard:guard + n].view(t.shape)


@pytest.mark.parametrize('M', [257, 1])
def test_ragged_bounds(M):
    """Operands and result carved out of NaN / sentinel buffers: a read past X, W or bias that reaches an output shows as
    NaN; every guard byte around Y is unchanged."""
    N, guard = 320, 4096
    g = torch.Generator().manual_seed(3000 + M)
    for K in (64, 320):
        x, w, b = _int_problem(M, N, K, g)
        want = x.double() @ w.double().t() + b.double()
        xs, ws, bs = _carved(x), _carved(w), _carved(b)
        for sched in (False, True):
            ybuf = torch.empty(guard + M * N + guard, dtype=BF, device=DEV)
            ybuf.view(torch.int16).fill_(SENT16)
            y = ybuf[guard:guard + M * N].view(M, N)
            _ragged(xs, ws, bs, y, sched)
            torch.cuda.synchronize()
            assert torch.isfinite(y).all()
            assert torch.equal(y.double(), want), (M, K, sched)
            raw = ybuf.view(torch.int16)
            assert bool((raw[:guard] == SENT16).all()) and bool((raw[guard + M * N:] == SENT16).all()), (M, K, sched)


@pytest.mark.parametrize('N,K', [(4800, 1600), (1600, 1600), (3200, 1600), (1600, 6400), (1600, 4800), (1600, 3200)])
def test_ragged_tn_at_the_xl_shapes(N, K):
    """c_attn, c_proj / q_attn, the cross c_attn, and the input gradients of c_fc, c_attn and the cross c_attn at width 1600:
    within 2^-7 of the output's maximum (bf16 operands, f32 accumulation, one bf16 rounding), repeats bit-identical."""
    M = 300
    g = torch.Generator().manual_seed(4000 + N + K)
    x = torch.randn(M, K, generator=g).to(DEV).to(BF)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV).to(BF)
    b = torch.randn(N, generator=g).to(DEV)
    want = x.double() @ w.double().t() + b.double()
    y = _ragged(x, w, b, torch.empty(M, N, dtype=BF, device=DEV), False)
    y2 = _ragged(x, w, b, torch.empty(M, N, dtype=BF, device=DEV), False)
    ratio = ((y.double() - want).abs().max() / want.abs().max()).item()
    print(f'[ragged tn {M}x{N}x{K}] max|d| / max|want| {ratio:.2e} (bound {2.0 ** -7:.2e})')
    assert ratio <= 2.0 ** -7
    assert torch.equal(y, y2)


def test_ragged_refusals():
    from lavila_amd import _cabi as C
    from lavila_amd import ops
    E = C.HipExtensionError

    def call(M, N, K, **kw):
        x = torch.zeros(M, K, dtype=BF, device=DEV)
        w = torch.zeros(N, K, dtype=BF, device=DEV)
        return _ragged(x, w, None, torch.empty(M, N, dtype=BF, device=DEV), False, **kw)

    with pytest.raises(E, match=r'N % 64 == 0 and K % 64 == 0'):
        call(40, 96, 64)
    with pytest.raises(E, match=r'N % 64 == 0 and K % 64 == 0'):
        call(40, 64, 96)
    with pytest.raises(E, match='bf16 only'):
        call(40, 64, 64, dtype=C.LVL_F32)
    with pytest.raises(E, match='LVL_EPI_BIAS only'):
        call(40, 64, 64, epilogue=C.EPI_BIAS_RESIDUAL)
    with pytest.raises(E, match='unknown epilogue'):
        call(40, 64, 64, epilogue=17)
    with pytest.raises(E, match='16-byte aligned'):
        x = torch.zeros(40 * 64 + 8, dtype=BF, device=DEV)[4:4 + 40 * 64].view(40, 64)
        _ragged(x, torch.zeros(64, 64, dtype=BF, device=DEV), None, torch.empty(40, 64, dtype=BF, device=DEV), False)
    call(40, 64, 64)                                       # the control: this one runs
    torch.cuda.synchronize()
    # lvl_linear_tn itself keeps refusing a width that is not a multiple of 256
    with pytest.raises(E, match=r'N % 256 == 0'):
        ops.linear_tn_raw(torch.zeros(40, 64, dtype=BF, device=DEV), torch.zeros(320, 64, dtype=BF, device=DEV))


# ----------------------------------------------------------------------------------------------------------------------
# weight gradient
# ----------------------------------------------------------------------------------------------------------------------
def _wgrad(dy, x, want_dbias, sched):
    from lavila_amd import _cabi as C
    M, N = dy.shape
    K = x.shape[1]
    n_ws = C.lib().lvl_workspace_floats(b'linear_wgrad', N, K)
    assert n_ws > 0, (N, K)
    ws = torch.full((n_ws,), float('nan'), device=DEV)
    dw = torch.full((N, K), float('nan'), device=DEV)
    db = torch.full((N,), float('nan'), device=DEV) if want_dbias else None
    blk = torch.zeros(1024, dtype=torch.int32, device=DEV) if sched else None
    C.check(C.lib().lvl_linear_wgrad(C.ptr(dy), C.ptr(x), C.ptr(dw), C.ptr(db), C.ptr(ws), C.ptr(blk), M, N, K, C.LVL_BF16,
                                     C.stream_ptr()), 'lvl_linear_wgrad')
    if blk is not None:
        torch.cuda.synchronize()
        assert int(blk.abs().sum()) == 0
    return dw, db


# the issue's shapes, and the tied lm_head of a decoder with a small vocabulary (padded to 256s) at widths 320 and 1600
@pytest.mark.parametrize('N,K', [(160, 160), (320, 160), (160, 320), (960, 320), (320, 1280), (1600, 4800), (6400, 1600),
                                 (512, 320), (512, 1600)])
def test_wgrad_160_family_exact_on_integers(N, K):
    g = torch.Generator().manual_seed(5000 + N + K)
    for M in (33, 200, 3100):
        dy = torch.randint(-2, 3, (M, N), generator=g).to(DEV).to(BF)
        x = torch.randint(-2, 3, (M, K), generator=g).to(DEV).to(BF)
        want = dy.double().t() @ x.double()                 # |dW| <= 4 * 3100: exact in f32 in any order
        want_b = dy.double().sum(0)
        for want_dbias in (True, False):
            for sched in (False, True):
                dw, db = _wgrad(dy, x, want_dbias, sched)
                assert torch.equal(dw.double(), want), (M, N, K, want_dbias, sched)
                if want_dbias:
                    assert torch.equal(db.double(), want_b), (M, N, K, sched)
