"""GPU (the tests marked gpu): the skinny GEMMs of the decoder on operands whose product is EXACT.

tests/test_gpu_narrator.py holds lvl_linear_skinny to atol = rtol = 1e-2 (3e-2 with the LayerNorm prologue) on random
operands; these kernels split the contraction over 8 waves, fetch k-steps in rounds of 6 (3, 7) and in pairs and add the
partial sums in LDS, and one dropped or doubled k-step of one wave at K = 3072 sits near the edge of that band. Here, as in
test_linear_tn_exact_on_integer_operands: x integers in [-2, 2], w sparse +-1, bias integers in [-8, 8], |x w^T + b| < 256
(asserted on the CPU reference) -- every partial sum is an integer that float32 holds and the result one that bf16 holds,
so the assertion is torch.equal, on every dispatch branch of the three entry points (the dispatch is restated in Python
and the shape lists are checked against it before anything runs).
"""
import functools

import pytest
import torch

from oracle import oracle as O

gpu = pytest.mark.gpu
DEV = 'cuda'
BF = torch.bfloat16
NAN = float('nan')


# ---- the dispatch of gemm_skinny.hip, restated -------------------------------------------------------------------------
def _skinny_branch(M, N, K):
    """lvl_linear_skinny: which kernel template a shape runs on."""
    assert N % 16 == 0 and K % 32 == 0
    if K % 64 == 0:
        if N >= 8192 and M <= 128:
            return 'mid 64x128, few rows'
        if M > 128:
            if N >= 2048:
                return 'mid 64x128'
            return 'mid 32x64, two K groups' if K % 128 == 0 else 'mid 32x64'
    if M > 128:
        if N >= 2048 and N % 64 == 0:
            return 'strips <4,4>'
        return 'strips <2,4>' if N % 32 == 0 else 'strips <1,2>'
    if N >= 2048 and N % 64 == 0:
        return 'strips <4,2>'
    return 'strips <1,1,paired>'


def _f32c_branch(M, N, K):
    assert N % 16 == 0 and K % 32 == 0
    if M > 128:
        return 'strips <4,4>' if N % 64 == 0 else 'strips <2,4>' if N % 32 == 0 else 'strips <1,2>'
    return 'strips <4,2>' if N >= 2048 and N % 64 == 0 else 'strips <1,1,paired>'


def _ln_branch(M, N, K):
    assert N % 16 == 0 and K % 32 == 0 and K <= 1792
    if K <= 768:
        return '<4,2,3>' if N >= 2048 and N % 64 == 0 else '<1,1,3>'
    return '<1,1,7>'


SKINNY = {
    'strips <1,1,paired>': [(1, 48, 32), (16, 48, 32), (65, 192, 192), (128, 768, 3072), (33, 1600, 1600)],
    'strips <4,2>': [(7, 2304, 768), (100, 2048, 96)],
    'mid 64x128, few rows': [(64, 50432, 768), (3, 8192, 64)],
    'mid 64x128': [(129, 2304, 768), (640, 3072, 768)],
    'mid 32x64, two K groups': [(257, 768, 768), (150, 64, 3072)],
    'mid 32x64': [(131, 128, 64), (333, 1600, 1600)],
    'strips <4,4>': [(150, 2048, 96)],
    'strips <2,4>': [(150, 64, 96)],
    'strips <1,2>': [(150, 48, 32)],
}
SKINNY_SHAPES = [s for shapes in SKINNY.values() for s in shapes]
F32C = {
    'strips <1,1,paired>': [(1, 48, 32), (65, 192, 192), (33, 1600, 1600)],
    'strips <4,2>': [(7, 2304, 768)],
    'strips <4,4>': [(150, 64, 96), (257, 768, 768)],
    'strips <2,4>': [(150, 96, 128)],
    'strips <1,2>': [(150, 48, 32)],
}
F32C_SHAPES = [s for shapes in F32C.values() for s in shapes]
LN = {'<1,1,3>': [(1, 48, 32), (64, 768, 768)], '<4,2,3>': [(7, 2304, 768)], '<1,1,7>': [(33, 1600, 1600), (128, 192, 1792)]}
LN_SHAPES = [s for shapes in LN.values() for s in shapes]


def test_shape_lists_reach_every_dispatch_branch():
    """Host only: every branch of the three dispatches has its shapes, and every k-step remainder of the 8-way split."""
    for table, branch_of, n in ((SKINNY, _skinny_branch, 9), (F32C, _f32c_branch, 5), (LN, _ln_branch, 3)):
        assert len(table) == n
        for branch, shapes in table.items():
            assert shapes and all(branch_of(*s) == branch for s in shapes), branch
    # the thresholds themselves: one row, one column block or one k-step further and the branch changes
    assert _skinny_branch(128, 768, 3072) != _skinny_branch(129, 768, 3072)
    assert _skinny_branch(100, 2048, 96) != _skinny_branch(100, 2032, 96)
    assert _skinny_branch(3, 8192, 64) != _skinny_branch(3, 8176, 64) != _skinny_branch(3, 8192, 96)
    assert _ln_branch(64, 768, 768) != _ln_branch(64, 768, 800)
    # the strips split K / 32 steps over 8 waves: one step, fewer steps than waves, a whole number of rounds of 6 x 8
    # steps (96 = 2 rounds: the last step of wave 7 is the last of K) and a partial round (50 = 6 x 8 + 2)
    steps = {K // 32 for M, N, K in SKINNY['strips <1,1,paired>']}
    assert {1, 6, 96, 50} <= steps and any(s % 8 == 0 for s in steps)
    assert {K // 32 for M, N, K in LN_SHAPES} >= {1, 24, 50, 56}           # 56 = 7 steps on each of 8 waves: the cap


# ---- operands ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _integer_case(M, N, K, kind='plain'):
    """x, w, b in float32 on the CPU and the exact product x w^T; |x w^T| + |b| < 256 is asserted.
    'plain': x in [-2, 2], w +-1 on the first column of every 32-wide k-step and on about 200 further columns per row
             (min(1/2, 200 / K) of them), so every k-step of every weight row carries a nonzero; b in [-8, 8];
    'small': x in [-2, 2], w +-1 on two columns per row, b in [-3, 3]: |x w^T + b| <= 7, so the SQUARE stays < 256;
    'gelu':  x in {0, 1}, w = 1 on two columns per row, b in [-3, 3]: the pre-activation is an integer in [-3, 5] --
             where gelu_new bends (at -3 .. 2 it differs from the identity by more than a bf16 rounding: 5 of the 9
             values, 3/4 of the products without bias; _gelu_visible asserts a share of 40 %), and not below -3, where the float32 formula's 1 + tanh cancels (at -3 it is 2.4e-3,
             computed with an absolute error of about 1.2e-7: 5e-5 relative, far inside one bf16 rounding; at -4
             that error is already 7e-3 relative)."""
    g = torch.Generator().manual_seed(M * 7919 + N * 31 + K + len(kind))
    x = torch.randint(0, 2, (M, K), generator=g).float() if kind == 'gelu' else torch.randint(-2, 3, (M, K), generator=g).float()
    sign = torch.where(torch.rand(N, K, generator=g) < 0.5, -1.0, 1.0)
    if kind == 'plain':
        w = (torch.rand(N, K, generator=g) < min(0.5, 200.0 / K)).float()
        w[:, ::32] = 1.0
        w = w * sign
        assert bool((w.reshape(N, K // 32, 32) != 0).any(-1).all())
    else:
        w = torch.zeros(N, K).scatter_(1, torch.randint(0, K, (N, 2), generator=g), 1.0) * (sign if kind == 'small' else 1.0)
    lo, hi = {'plain': (-8, 8), 'small': (-3, 3), 'gelu': (-3, 3)}[kind]
    b = torch.randint(lo, hi + 1, (N,), generator=g).float()
    xw = x @ w.t()                                   # integers far below 2^24: exact in float32 in any order
    assert (xw.abs().max() + b.abs().max()).item() < 256
    return x, w, b, xw


def _gelu_visible(pre):
    """The gelu_new check must see the activation: at least 40 % of the pre-activations are nonzero and sit where
    gelu_new differs from the identity by more than the 2^-8 band of the assertion (a kernel that skipped the
    activation, or used a wrong constant in it, fails there), none is below -3, and both signs occur with a bias."""
    assert pre.min() >= -3 and pre.max() <= 5
    bent = (O.gelu_new(pre.double()) - pre.double()).abs() > 2.0 ** -8 * pre.double().abs()
    assert bent.double().mean().item() >= 0.4, bent.double().mean().item()
    return bent


ACT_SHAPES = [s for s in SKINNY_SHAPES if s[1] < 50000]


@pytest.mark.parametrize('M,N,K', ACT_SHAPES)
def test_gelu_operands_sit_where_gelu_new_bends(M, N, K):
    """Host only: the operands of the gelu_new check on every shape it runs, with and without the bias."""
    x, w, b, xw = _integer_case(M, N, K, 'gelu')
    _gelu_visible(xw + b)
    _gelu_visible(xw)
    assert (xw + b).min() < 0 or M * N < 100


def _skinny(x, w, bias, M, N, K, act):
    """One lvl_linear_skinny call into a NaN-filled buffer with a guard row; returns the [M, N] result."""
    from lavila_amd import _cabi as C
    y = torch.full((M + 1, N), NAN, dtype=BF, device=DEV)
    C.check(C.lib().lvl_linear_skinny(C.ptr(x), C.ptr(w), C.ptr(bias), C.ptr(y), M, N, K, act, C.stream_ptr()),
            'lvl_linear_skinny')
    torch.cuda.synchronize()
    assert torch.isnan(y[M].float()).all(), 'the guard row below the result was written'
    return y[:M].float().cpu()


@gpu
@pytest.mark.parametrize('M,N,K', SKINNY_SHAPES)
def test_linear_skinny_exact_on_integer_operands(M, N, K):
    """Every branch of lvl_linear_skinny, with and without bias: torch.equal."""
    x, w, b, xw = _integer_case(M, N, K)
    xd, wd, bd = x.to(DEV, BF), w.to(DEV, BF), b.to(DEV)
    for bias, want in ((bd, xw + b), (None, xw)):
        assert want.abs().max() < 256
        got = _skinny(xd, wd, bias, M, N, K, -1)
        if not torch.equal(got, want):
            i = torch.nonzero(got != want)[0].tolist()
            raise AssertionError(f'{_skinny_branch(M, N, K)} {(M, N, K)} bias={bias is not None}: '
                                 f'{int((got != want).sum())} of {want.numel()} values wrong, first at {i}: got '
                                 f'{got[tuple(i)].item()}, want {want[tuple(i)].item()}')


@gpu
@pytest.mark.parametrize('M,N,K', ACT_SHAPES)
def test_linear_skinny_activations_on_integer_operands(M, N, K):
    """relu^2 of an integer below 16 is exact; gelu_new of the exact pre-activation within one bf16 rounding (2^-8
    relative), on integer pre-activations in [-3, 5], where gelu_new is not the identity (see _integer_case)."""
    from lavila_amd import _cabi as C
    x, w, b, xw = _integer_case(M, N, K, 'small')
    pre = xw + b
    assert pre.abs().max() < 16 and pre.max() >= 2
    xd, wd, bd = x.to(DEV, BF), w.to(DEV, BF), b.to(DEV)
    got = _skinny(xd, wd, bd, M, N, K, C.ACT_SQRELU)
    assert torch.equal(got, O.sq_relu(pre)), f'sqrelu {_skinny_branch(M, N, K)}'
    got = _skinny(xd, wd, None, M, N, K, C.ACT_SQRELU)
    assert torch.equal(got, O.sq_relu(xw))
    x, w, b, xw = _integer_case(M, N, K, 'gelu')
    xd, wd, bd = x.to(DEV, BF), w.to(DEV, BF), b.to(DEV)
    for bias, pre in ((bd, xw + b), (None, xw)):
        _gelu_visible(pre)
        want = O.gelu_new(pre.double())
        got = _skinny(xd, wd, bias, M, N, K, C.ACT_GELU_NEW).double()
        err = (got - want).abs()
        assert bool((err <= 2.0 ** -8 * want.abs()).all()), \
            f'gelu_new {_skinny_branch(M, N, K)}: worst {(err / want.abs().clamp_min(1e-30)).max().item():.3e} relative'


# ---- f32-class mode ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('M,N,K', F32C_SHAPES)
def test_linear_skinny_f32c_exact_on_integer_operands(M, N, K):
    """lvl_linear_skinny_f32c called directly on the term images of integer operands (their low terms are exactly
    zero): the float32 result equals the reference, on all five branches."""
    from lavila_amd import _cabi as C
    from lavila_amd import ops
    x, w, b, xw = _integer_case(M, N, K)
    x3, w3 = ops.split3(x.to(DEV), 0), ops.split3(w.to(DEV), 1)
    assert x3.shape == (M, 3 * K) and not x3[:, 2 * K:].any() and not w3[:, K:2 * K].any()
    for bias, want in ((b.to(DEV), xw + b), (None, xw)):
        y = torch.full((M + 1, N), NAN, dtype=torch.float32, device=DEV)           # a guard row below the result
        C.check(C.lib().lvl_linear_skinny_f32c(C.ptr(x3), C.ptr(w3), C.ptr(bias), C.ptr(y), M, N, 3 * K, -1,
                                               C.stream_ptr()), 'lvl_linear_skinny_f32c')
        torch.cuda.synchronize()
        assert torch.isnan(y[M]).all(), 'the guard row below the result was written'
        assert torch.equal(y[:M].cpu(), want), f'{_f32c_branch(M, N, K)} {(M, N, K)} bias={bias is not None}'


@gpu
@pytest.mark.parametrize('M,N,K', [(65, 768, 768), (150, 96, 128)])
def test_linear_skinny_f32c_vs_float64(M, N, K):
    """Random float32 operands against float64, elementwise inside the bound of test_linear_tn_f32_class_vs_float64:
    3 * 2^-17 * (|x| |w|^T) + 1e-6 (the three dropped low-low products of the split)."""
    from lavila_amd import ops
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    ref = x.double() @ w.double().t() + b.double()
    bound = 3 * 2.0 ** -17 * (x.double().abs() @ w.double().abs().t()) + 1e-6
    y = ops.linear_skinny_f32c_raw(ops.split3(x, 0), ops.split3(w, 1), b)
    assert ((y.double() - ref).abs() <= bound).all(), ((y.double() - ref).abs() / bound).max()


# ---- LayerNorm prologue ------------------------------------------------------------------------------------------------
LN_A, LN_EPS = 4.0, 1e-5


def _ln_case(M, N, K):
    """The operands of test_linear_skinny_ln_exact_by_construction and its float64 reference, preconditions asserted."""
    g = torch.Generator().manual_seed(M + N + K)
    a, eps = LN_A, LN_EPS
    sign = torch.ones(M, K)
    sign[:, K // 2:] = -1
    sign = torch.gather(sign, 1, torch.argsort(torch.rand(M, K, generator=g), 1))
    assert bool((sign.sum(1) == 0).all())
    gamma = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (K,), generator=g)]
    beta = torch.randint(-2, 3, (K,), generator=g).float()
    beta = torch.where(beta.abs() == gamma, torch.zeros_like(beta), beta)        # +-gamma + beta never cancels to 0
    w = torch.randint(-1, 2, (N, K), generator=g).float() * (torch.rand(N, K, generator=g) < 1.5 * min(0.5, 60.0 / K))
    b = torch.randint(-8, 9, (N,), generator=g).float()
    s64 = (a * sign).double()
    # the float64 formula, and the precondition: the normalised operand rounds to sign * gamma + beta
    h64 = O.layer_norm(s64, gamma.double(), beta.double(), eps)
    ideal = sign.double() * gamma.double() + beta.double()
    assert eps / a ** 2 < 2.0 ** -8 / 4
    assert bool(((h64 - ideal).abs() <= 2.0 ** -8 / 4 * ideal.abs()).all())
    assert torch.equal(h64.to(BF).double(), ideal)
    want64 = h64.to(BF).double() @ w.double().t() + b.double()
    assert want64.abs().max() < 256 and torch.equal(want64.to(BF).double(), want64)
    return sign, gamma, beta, w, b, s64, want64


@pytest.mark.parametrize('M,N,K', LN_SHAPES)
def test_linear_skinny_ln_operands_are_exact_by_construction(M, N, K):
    """Host only: the preconditions of the exact LayerNorm-prologue test hold for every shape."""
    _ln_case(M, N, K)


@gpu
@pytest.mark.parametrize('with_y', [False, True])
@pytest.mark.parametrize('M,N,K', LN_SHAPES)
def test_linear_skinny_ln_exact_by_construction(M, N, K, with_y):
    """Every row of the new residual is +a on half of its channels and -a on the other half (a random permutation per
    row; with_y: res = +-a/2 and y = +-a/2 of the same sign): mean 0, variance a^2, and the normalised row is
    +-gamma (1 - eps / (2 a^2) + ...) + beta. With gamma a power of two and beta a small integer that rounds to the bf16
    value +-gamma + beta in the fused kernel and in the float64 formula alike, as long as eps / a^2 stays below a
    quarter bf16 ulp -- asserted below -- and with sparse +-1 weights the product is exact again: torch.equal with the
    float64 reference rounded to bf16."""
    from lavila_amd import _cabi as C
    a, eps = LN_A, LN_EPS
    sign, gamma, beta, w, b, s64, want64 = _ln_case(M, N, K)
    if with_y:
        res, y = (0.5 * a * sign).to(DEV, BF), (0.5 * a * sign).to(DEV, BF)
    else:
        res, y = (a * sign).to(DEV, BF), None
    out = torch.full((M + 1, N), NAN, dtype=BF, device=DEV)
    new_res = torch.full((M + 1, K), NAN, dtype=BF, device=DEV)
    gd, bed, wd, bd = gamma.to(DEV), beta.to(DEV), w.to(DEV, BF), b.to(DEV)
    C.check(C.lib().lvl_linear_skinny_ln(C.ptr(res), C.ptr(y), None, C.ptr(gd), C.ptr(bed), eps,
                                         C.ptr(new_res) if with_y else None, C.ptr(wd), C.ptr(bd), C.ptr(out), M, N, K, -1,
                                         C.stream_ptr()), 'lvl_linear_skinny_ln')
    torch.cuda.synchronize()
    assert torch.isnan(out[M].float()).all() and torch.isnan(new_res[M].float()).all()
    if with_y:
        assert torch.equal(new_res[:M].double().cpu(), s64)
    else:
        assert torch.isnan(new_res.float()).all()
    got = out[:M].double().cpu()
    if not torch.equal(got, want64):
        i = torch.nonzero(got != want64)[0].tolist()
        raise AssertionError(f'{_ln_branch(M, N, K)} {(M, N, K)}: {int((got != want64).sum())} of {got.numel()} values '
                             f'wrong, first at {i}: got {got[tuple(i)].item()}, want {want64[tuple(i)].item()}')
