"""CPU: the helper of test_gpu_rowops_at_scale.py (rowops_reference.py). Its mirrored grid caps must match the kernel
sources, its float64 restatements the oracle, its row counts must straddle the caps, its fingerprints must stay exact in
f32, and its error bounds must hold for a plain float32 evaluation while staying 10x below the effects they must see."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import rowops_reference as R
from oracle import oracle as O


@pytest.mark.parametrize('name', sorted(R.SOURCE_CAPS))
def test_caps_match_the_sources(name):
    fname, pat = R.SOURCE_CAPS[name]
    with open(os.path.join(R.CSRC, fname)) as f:
        found = re.findall(pat, f.read())
    assert len(found) == 1, f'{name}: pattern {pat!r} matched {len(found)} times in {fname}'
    assert int(found[0]) == getattr(R, name), f'{name}: {fname} says {found[0]}, rowops_reference says {getattr(R, name)}'


def test_grid_for_is_the_only_cap_of_the_1d_kernels():
    with open(os.path.join(R.CSRC, 'elementwise.hip')) as f:
        src = f.read()
    assert src.count('dim3(grid_for(') == 4 and src.count(', 256)), dim3(256)') == 4     # patchify x 3, embed_tokens


def _ln_rows(rows, cols, g):
    x = 2 * torch.randn(rows, cols, generator=g, dtype=torch.float64) + 0.5
    x[3::8] = 0.75
    x[6::8] = 1e-3 * torch.randn(x[6::8].shape, generator=g, dtype=torch.float64)
    return x


@pytest.mark.parametrize('cols', [8, 264, 768, 1032, 4096])
def test_layernorm_references_match_the_oracle(cols):
    g = torch.Generator().manual_seed(cols)
    s = _ln_rows(37, cols, g)
    gamma, beta = 1 + 0.2 * torch.randn(cols, generator=g), 0.1 * torch.randn(cols, generator=g)
    y, mu, rs = R.ln_fwd_ref(s, gamma, beta, 1e-5)
    assert torch.allclose(y, O.layer_norm(s, gamma.double(), beta.double(), 1e-5), rtol=1e-12, atol=1e-12)
    assert torch.allclose(y, F.layer_norm(s, (cols,), gamma.double(), beta.double(), 1e-5), rtol=1e-10, atol=1e-10)
    # backward at the exact float64 statistics = autograd of F.layer_norm
    xs = s.clone().requires_grad_(True)
    gw = gamma.double().requires_grad_(True)
    dy = torch.randn(37, cols, generator=g, dtype=torch.float64)
    F.layer_norm(xs, (cols,), gw, beta.double(), 1e-5).backward(dy)
    dxp, dx, t = R.ln_bwd_ref(dy, s, gamma, mu, rs, dadd=dy)
    assert torch.allclose(dxp, xs.grad, rtol=1e-9, atol=1e-9)
    assert torch.allclose(dx, xs.grad + dy, rtol=1e-9, atol=1e-9)
    assert torch.allclose(t.sum(0), gw.grad, rtol=1e-9, atol=1e-9)


def test_gelu_reference_matches_the_oracle():
    g = torch.Generator().manual_seed(1)
    u = (3 * torch.randn(64, 24, generator=g, dtype=torch.float64)).requires_grad_(True)
    b = torch.randn(24, generator=g, dtype=torch.float64)
    a, f = R.gelu_ref(u.detach(), b)
    ao = O.quick_gelu(u + b)
    ao.backward(torch.ones_like(ao))
    assert torch.allclose(a, ao.detach(), rtol=1e-12, atol=1e-14)
    assert torch.allclose(f, u.grad, rtol=1e-10, atol=1e-12)


def test_split3_reference():
    x = torch.tensor([1.0, 1 + 2 ** -9, -3 * 2 ** -10 * (1 + 2 ** -12), float('inf'), 1 + 2 ** -8 + 2 ** -20])
    h, l = R.split3_ref(x)
    assert torch.equal(h.float()[:3] + l.float()[:3], x[:3])          # 16 significant bits: exact in two terms
    assert h[1].item() == 1 and l[1].item() == 2 ** -9
    assert l[3].item() == 0 and h[3].item() == float('inf')
    assert h[4].item() == 1 + 2 ** -7 and l[4].item() == -2 ** -8    # x - h = -2^-8 + 2^-20 rounds to -2^-8
    assert abs(x[4] - h.float()[4] - l.float()[4]) <= 2 ** -18 * abs(x[4])


def test_row_counts_straddle_the_caps():
    # LayerNorm: at C - 1 and C every wave owns at most one row, at C + 1 one wave owns two
    for cap_blocks, x2 in ((R.LN_FWD_BLOCKS, False), (R.LN_FWD_X2_BLOCKS, True)):
        C = R.ln_fwd_cap_rows(x2)
        sweep = R.cap_sweep(C, bench=True)
        assert {C - 1, C, C + 1, 4 * C + 5, R.BENCH_ROWS} <= set(sweep)
        blocks = lambda rows: min(-(-rows // R.LN_ROWS_PER_BLOCK), cap_blocks)      # noqa: E731
        assert blocks(C) * R.LN_ROWS_PER_BLOCK == C and blocks(C + 1) * R.LN_ROWS_PER_BLOCK == C
        assert R.BENCH_ROWS > 4 * C + 5 or not x2
    Cb = R.LN_BWD_PARTS * R.LN_ROWS_PER_BLOCK
    assert R.ln_bwd_blocks(Cb) == R.ln_bwd_blocks(Cb + 1) == R.LN_BWD_PARTS > R.ln_bwd_blocks(Cb - 4)
    # the unrolled loops: at 4 gy - 1 the last row block never enters it, at 4 gy every block does, + 3 runs the rest
    for cols in (8, 768, 1032, 2048, 3072, 4096):
        for gy in (R.GELU_FWD_BLOCKS // R.gelu_gx(cols), R.GELU_BWD_ROW_BLOCKS):
            lo, at, hi = R.unroll_edges(gy)
            assert lo in R.gelu_rows(cols) and at in R.gelu_rows(cols) and hi in R.gelu_rows(cols)
            assert len(R.unrolled_rows(lo, gy)[0]) == 4 * (gy - 1)
            assert R.unrolled_rows(at, gy) == (R.unrolled_rows(at, gy)[0], []) and len(R.unrolled_rows(at, gy)[0]) == at
            assert len(R.unrolled_rows(hi, gy)[1]) == 3
        for rows in R.gelu_rows(cols):
            for gy in (R.gelu_fwd_gy(rows, cols), R.gelu_bwd_gy(rows)):
                a, b = R.unrolled_rows(rows, gy)
                assert sorted(a + b) == list(range(rows))
    # the 1-D kernels: past grid_for's cap at the shapes the GPU tests use
    cap = R.GRID_FOR_BLOCKS * R.GRID_FOR_THREADS
    assert 64 * 785 * 96 > cap                                   # embed_tokens, B = 64
    assert 512 * 3 * 224 * 14 > cap and 512 * 3 * 224 * 16 > cap and 512 * 3 * 224 * 224 > cap   # patchify
    assert R.grid_for(64 * 785 * 96) == R.GRID_FOR_BLOCKS
    assert 2 * R.SPLIT_ROW_BLOCKS + 3 > 2 * R.SPLIT_ROW_BLOCKS


@pytest.mark.parametrize('rows', R.cap_sweep(R.LN_BWD_PARTS * R.LN_ROWS_PER_BLOCK, bench=True))
def test_marks_sit_on_the_boundaries(rows):
    C = R.LN_BWD_PARTS * R.LN_ROWS_PER_BLOCK
    stride = R.ln_bwd_blocks(rows) * R.LN_ROWS_PER_BLOCK
    mk = R.mark_rows(rows, stride, C)
    assert len(mk) == len(set(mk)) <= 24 and all(0 <= m < rows for m in mk)
    assert 0 in mk and rows - 1 in mk
    if rows > C:
        assert {r for r in (C - 1, C, C + 1, rows - stride, (rows - 1) // stride * stride) if r < rows} <= set(mk)
    # +-2^-k marks: every subset sum is exact in f32 and names its rows
    v = R.mark_values(len(mk), 4, 'cpu')
    assert torch.equal(v.sum(0).double(), v.double().sum(0))
    drop = v.sum(0) - v[len(mk) // 2]
    assert R.decode_marks(drop, v.double().sum(0), mk) == [mk[len(mk) // 2]]


def test_fingerprint_sums_fit_in_24_bits():
    assert 8 * R.BENCH_ROWS < R.MAX_EXACT                        # LayerNorm dbeta, dy in [-8, 8]
    assert 8 * (4 * 4096 + 3) < R.MAX_EXACT                      # qkv bias thirds
    assert 8 * 63 * 196 < R.MAX_EXACT and 8 * 63 * 4 < R.MAX_EXACT   # d temporal_embed, d pos_embed
    s = sum(2.0 ** -k for k in range(24))                        # marks 2^0 .. 2^-23 span 24 bits
    assert float(torch.tensor(s, dtype=torch.float32)) == s


@pytest.mark.parametrize('cols', [8, 128, 264, 768, 1032, 1600, 4096])
def test_layernorm_bounds_hold_for_float32_and_see_the_effects(cols):
    """A float32 LayerNorm (torch's own order) stays within 2x the model bound; the bound stays >= 10x below an n - 1
    variance divisor (rstd, every row) and an eps outside the square root (rstd and y, the low-variance rows)."""
    g = torch.Generator().manual_seed(cols + 1)
    eps = 1e-6
    s = _ln_rows(64, cols, g).float().double()
    gamma, beta = 1 + 0.2 * torch.randn(cols, generator=g), 0.1 * torch.randn(cols, generator=g)
    y64, mu, rs = R.ln_fwd_ref(s, gamma, beta, eps)
    for dt in (torch.float32, torch.bfloat16):
        ey, emu, ers = R.ln_fwd_bounds(s, s.abs(), 0, gamma, beta, eps, cols, dt)
        s32 = s.float()
        m32 = s32.mean(-1, keepdim=True)
        v32 = ((s32 - m32) ** 2).mean(-1, keepdim=True)
        r32 = torch.rsqrt(v32 + eps)
        y32 = ((s32 - m32) * r32 * gamma + beta).to(dt)
        assert ((y32.double() - y64).abs() <= 2 * ey).all()
        assert ((m32[:, 0].double() - mu).abs() <= 2 * emu).all()
        assert ((r32[:, 0].double() - rs).abs() <= 2 * ers).all()
        var = ((s - mu[:, None]) ** 2).mean(-1)
        nm1 = torch.rsqrt(var * cols / (cols - 1) + eps)
        low = torch.zeros(64, dtype=torch.bool)
        low[3::8] = low[6::8] = True
        assert ((nm1 - rs)[~low].abs() >= 10 * 2 * ers[~low]).all(), 'n - 1 divisor hidden in the rstd bound'
        late = torch.rsqrt(var) + eps                            # eps added after rsqrt
        assert ((late - rs)[low].abs() >= 10 * 2 * ers[low]).all()
        y_late = (s - mu[:, None]) * late[:, None] * gamma.double() + beta.double()
        sm = low.clone()
        sm[3::8] = False                                         # constant rows: y_late is nan / inf
        assert ((y_late - y64)[sm].abs().amax(-1) >= 10 * 2 * ey[sm].amax(-1)).all()
        assert not torch.isfinite(late[3::8]).any()


@pytest.mark.parametrize('cols', [8, 768, 4096])
def test_layernorm_bwd_bounds_hold_for_float32(cols):
    g = torch.Generator().manual_seed(cols + 2)
    x = (2 * torch.randn(48, cols, generator=g) + 0.5).double()
    gamma = 1 + 0.2 * torch.randn(cols, generator=g)
    _, mu, rs = R.ln_fwd_ref(x, gamma, gamma, 1e-6)
    mu, rs = mu.float(), rs.float()
    dy = torch.randint(-8, 9, (48, cols), generator=g).float()
    dadd = torch.randn(48, cols, generator=g)
    dxp64, dx64, _ = R.ln_bwd_ref(dy, x, gamma, mu, rs, dadd)
    ep, ex, _ = R.ln_bwd_bounds(dy, x, x.abs(), 0, gamma, mu, rs, dadd, cols, torch.float32)
    xh = (x.float() - mu[:, None]) * rs[:, None]
    dg = dy * gamma
    c1, c2 = dg.mean(-1, keepdim=True), (dg * xh).mean(-1, keepdim=True)
    dxp = rs[:, None] * (dg - c1 - xh * c2)
    assert ((dxp.double() - dxp64).abs() <= 2 * ep).all()
    assert (((dxp + dadd).double() - dx64).abs() <= 2 * ex).all()


def test_gelu_bounds_hold_for_float32():
    g = torch.Generator().manual_seed(3)
    u = (3 * torch.randn(256, 64, generator=g)).double()
    b = torch.randn(64, generator=g)
    a64, f64 = R.gelu_ref(u, b)
    ea, ef = R.gelu_bounds(u, b, torch.float32)
    y = u.float() + b
    s = 1 / (1 + torch.exp(-(1.702 * y)))
    assert (((y * s).double() - a64).abs() <= 2 * ea).all()
    f = s + 1.702 * y * s * (1 - s)
    assert ((f.double() - f64).abs() <= 2 * ef).all()
