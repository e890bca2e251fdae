"""GPU (-m gpu): lvl_vec_mat_f32 (out[k] = sum_n v[n] W[n, k], the column-sum token rule of a Linear) on its own.

The token test reaches it only at N = K = 256, where neither the 16-row tail loop behind the 128-row steps nor the k < K
column tail runs (nor do they at 768 or 1024, the widths the towers use). Here:

  * small integers (|v|, |W| <= 8: every partial sum is an integer below 2^24, so float32 is exact in any order) at every
    N around the 16-row and 128-row steps and every K around the 64-column block -- the result must equal the integer
    product;
  * random data against float64 under the bound of the kernel's summation: each of the 16 waves runs one fma chain over at
    most ceil(N / 16) rows, the 16 partial sums are added in a chain of 16, so
    |err[k]| <= (N / 16 + 17) 2^-24 sum_n |v[n] W[n, k]|;
  * ops.vec_mat on a non-contiguous weight and on a bf16 weight (the wrapper hands the kernel a contiguous float32 copy).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NS = [1, 15, 16, 17, 127, 128, 129, 255, 768, 1600]
KS = [1, 63, 64, 65, 768]


def _ints(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-8, 9, (N,), generator=g).float(), torch.randint(-8, 9, (N, K), generator=g).float())


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('N', NS)
def test_vec_mat_small_integers_exact(N, K):
    from lavila_amd import ops
    v, W = _ints(N, K, 1000 * N + K)
    assert N * 64 < 2 ** 24
    want = v.double() @ W.double()
    got = ops.vec_mat(v.to(DEV), W.to(DEV))
    assert got.shape == (K,) and got.dtype == torch.float32
    assert torch.equal(got.double().cpu(), want), f'N={N} K={K}: max error {(got.double().cpu() - want).abs().max().item()}'


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('N', NS)
def test_vec_mat_random_vs_float64(N, K):
    from lavila_amd import ops
    g = torch.Generator().manual_seed(7 + 1000 * N + K)
    v, W = torch.randn(N, generator=g), torch.randn(N, K, generator=g)
    want = v.double() @ W.double()
    bound = (N / 16 + 17) * 2.0 ** -24 * (v.double().abs() @ W.double().abs())
    err = (ops.vec_mat(v.to(DEV), W.to(DEV)).double().cpu() - want).abs()
    worst = (err / bound).max().item()
    print(f'vec_mat N={N} K={K}: largest error / bound = {worst:.3f}')
    assert bool((err <= bound).all()), f'N={N} K={K}: error {worst:.3f} x the fma-chain bound'


@pytest.mark.parametrize('N,K', [(129, 65), (768, 768)])
def test_vec_mat_takes_a_strided_and_a_bf16_weight(N, K):
    from lavila_amd import ops
    v, W = _ints(N, K, 3)
    want = v.double() @ W.double()
    Wt = W.t().contiguous().to(DEV)                   # [K, N]: its transposed view is the [N, K] weight, column-major
    assert not Wt.t().is_contiguous()
    assert torch.equal(ops.vec_mat(v.to(DEV), Wt.t()).double().cpu(), want)
    wide = torch.zeros(N, 2 * K + 3)
    wide[:, 1:2 * K:2] = W                            # every other column of a wider buffer
    view = wide.to(DEV)[:, 1:2 * K:2]
    assert not view.is_contiguous()
    assert torch.equal(ops.vec_mat(v.to(DEV), view).double().cpu(), want)
    assert torch.equal(ops.vec_mat(v.to(DEV), W.to(DEV, torch.bfloat16)).double().cpu(), want)      # |W| <= 8: bf16-exact
    param = torch.nn.Parameter(W.to(DEV))             # a parameter: read detached, no graph, no gradient
    out = ops.vec_mat(v.to(DEV), param)
    assert not out.requires_grad and torch.equal(out.double().cpu(), want)
