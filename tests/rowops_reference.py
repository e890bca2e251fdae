"""Float64 restatements of the HBM-bound row kernels (csrc/layernorm.hip, csrc/elementwise.hip), their error models, and
the row counts that straddle their grid caps.

Every row kernel caps its grid and walks rows with a grid stride (LayerNorm also prefetches the next row of its chain,
bias+QuickGELU and the qkv bias partials unroll the row loop by 4). The caps below mirror the sources;
test_rowops_reference_cpu.py parses each one back out of the source text, so a changed cap fails loudly instead of
quietly moving the GPU tests (test_gpu_rowops_at_scale.py) off their boundaries.

The references are plain torch float64 ops on whatever device their inputs live on (never the project's kernels). The
bound functions return per-element (or per-row / per-column) absolute error bounds from a first-order model of the
kernel's f32 arithmetic; the asserts multiply them by 2 to cover the second-order terms the model drops.
"""
import math
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'lavila_amd', 'csrc')

U = 2.0 ** -24                     # f32 unit round-off
U_OUT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8}     # half an ulp of the stored element, relative

# ---- grid caps, mirrored from the sources (file, regex whose groups are the values) ---------------------------------------
LN_ROWS_PER_BLOCK = 4              # layernorm.hip kRowsPerBlock: one wave per row, 4 waves per workgroup
LN_FWD_BLOCKS = 8192               # lvl_layernorm_fwd: one operand
LN_FWD_X2_BLOCKS = 3072            # lvl_layernorm_fwd: with x2 (the fused residual add)
LN_BWD_PARTS = 768                 # kLnBwdParts: workgroups = partial slabs of the backward
COLSUM_MID = 64                    # kColsumMid: row chunks of the column reduction's first stage
GELU_THREADS = 128                 # bias_gelu_*_kernel workgroup: 128 threads x 8 columns
GELU_FWD_BLOCKS = 4096             # lvl_bias_quickgelu_fwd: gx * gy <= 4096
GELU_BWD_ROW_BLOCKS = 1024         # kGeluBwdRowBlocks
GELU_UNROLL = 4                    # kGeluUnroll
QKV_BIAS_ROW_BLOCKS = 1024         # kBiasGradRowBlocks
GRID_FOR_BLOCKS = 16384            # grid_for(): workgroups of the 1-D grid-stride kernels
GRID_FOR_THREADS = 256             # ... of 256 threads (patchify, embed_tokens)
EMBED_BWD_CHUNKS = 4               # kEmbedBwdChunks: batch chunks of the token-assembly backward
SPLIT_ROW_BLOCKS = 16384           # lvl_split_bf16x3: row blocks

SOURCE_CAPS = {
    'LN_ROWS_PER_BLOCK': ('layernorm.hip', r'constexpr int kRowsPerBlock = (\d+);'),
    'LN_FWD_BLOCKS': ('layernorm.hip', r'const int64_t cap = x2 == nullptr \? (\d+) : \d+;'),
    'LN_FWD_X2_BLOCKS': ('layernorm.hip', r'const int64_t cap = x2 == nullptr \? \d+ : (\d+);'),
    'LN_BWD_PARTS': ('layernorm.hip', r'constexpr int kLnBwdParts = (\d+);'),
    'COLSUM_MID': ('layernorm.hip', r'constexpr int kColsumMid = (\d+);'),
    'GELU_THREADS': ('elementwise.hip', r'__launch_bounds__\((\d+)\) void bias_gelu_fwd_kernel'),
    'GELU_FWD_BLOCKS': ('elementwise.hip', r'int64_t gy = rows < (\d+) / gx \? rows : \d+ / gx;'),
    'GELU_BWD_ROW_BLOCKS': ('elementwise.hip', r'constexpr int kGeluBwdRowBlocks = (\d+);'),
    'GELU_UNROLL': ('elementwise.hip', r'constexpr int kGeluUnroll = (\d+);'),
    'QKV_BIAS_ROW_BLOCKS': ('elementwise.hip', r'constexpr int kBiasGradRowBlocks = (\d+);'),
    'GRID_FOR_BLOCKS': ('elementwise.hip', r'if \(g > (\d+)\) g = \d+;'),
    'GRID_FOR_THREADS': ('elementwise.hip', r'grid_for\(total, (\d+)\)'),
    'EMBED_BWD_CHUNKS': ('elementwise.hip', r'constexpr int kEmbedBwdChunks = (\d+);'),
    'SPLIT_ROW_BLOCKS': ('elementwise.hip', r'const unsigned gy = \(unsigned\)\(rows < (\d+) \? rows : \d+\);'),
}

BENCH_ROWS = 256 * 785             # the benched video tower: 256 clips x (1 + 4 x 196) tokens of 768
MAX_EXACT = 2 ** 24                # integers (and sums of powers of two spanning fewer bits) stay exact in f32


def cap_sweep(cap, bench=False):
    """Row counts around a cap of `cap` rows: one row, a partial workgroup, both sides of the cap, and chains of 2 and 4
    passes with a remainder."""
    rows = [1, 3, cap - 1, cap, cap + 1, 2 * cap + 3, 4 * cap + 5]
    if bench:
        rows.append(BENCH_ROWS)
    return sorted(set(rows))


# ---- launch geometry (what the launchers compute) -----------------------------------------------------------------------
def ln_fwd_cap_rows(x2):
    return (LN_FWD_X2_BLOCKS if x2 else LN_FWD_BLOCKS) * LN_ROWS_PER_BLOCK


def ln_bwd_blocks(rows):
    return max(1, min(-(-rows // LN_ROWS_PER_BLOCK), LN_BWD_PARTS))


def ln_dispatch(cols):
    """(VPL, W) of LN_DISPATCH: vectors per lane and vector width; VPL * W elements of a row per lane."""
    if cols % 256 == 0 and cols <= 1024:
        return min(cols // 256, 4), 4
    if cols // 8 <= 128:
        return 2, 8
    if cols // 8 <= 256:
        return 4, 8
    return 8, 8


def ln_exact_width(cols):
    vpl, w = ln_dispatch(cols)
    return vpl * 64 * w == cols


def gelu_gx(cols):
    return -(-(cols // 8) // GELU_THREADS)


def gelu_fwd_gy(rows, cols):
    return max(1, min(rows, GELU_FWD_BLOCKS // gelu_gx(cols)))


def gelu_bwd_gy(rows):
    return max(1, min(rows, GELU_BWD_ROW_BLOCKS))


def unroll_edges(gy):
    """rows = 4 gy - 1: the last row block never enters the unrolled loop; 4 gy: every block runs it once; + 3: and the
    remainder loop runs again."""
    return [GELU_UNROLL * gy - 1, GELU_UNROLL * gy, GELU_UNROLL * gy + 3]


def gelu_rows(cols):
    """Row counts for one width: the forward cap's sweep and unroll edges, the backward's (and the qkv partials') likewise."""
    cf = GELU_FWD_BLOCKS // gelu_gx(cols)
    rows = set(cap_sweep(cf)) | set(unroll_edges(cf)) | set(cap_sweep(GELU_BWD_ROW_BLOCKS)) | \
        set(unroll_edges(GELU_BWD_ROW_BLOCKS))
    return sorted(rows)


def unrolled_rows(rows, gy):
    """Simulates the rows walked by the row loop of bias_gelu_*_kernel / qkv_bias_partial_kernel (unroll 4, stride gy):
    returns (rows visited by the unrolled loop, rows visited by the remainder loop), each as a list (duplicates kept)."""
    unrolled, rest = [], []
    for r0 in range(gy):
        r = r0
        while r + (GELU_UNROLL - 1) * gy < rows:
            unrolled += [r + k * gy for k in range(GELU_UNROLL)]
            r += GELU_UNROLL * gy
        while r < rows:
            rest.append(r)
            r += gy
    return unrolled, rest


def grid_for(total, block=GRID_FOR_THREADS):
    return max(1, min(-(-total // block), GRID_FOR_BLOCKS))


def colsum_depth(chain, nparts, lds=0):
    """Longest chain of f32 additions behind one column sum: `chain` terms added in sequence per thread, `lds` more in the
    workgroup combine, then the two-stage column reduction of `nparts` slab rows (stage 1: ceil(nparts / 64) rows per
    chunk, 2 more merging its 4 waves; stage 2: 4 + 16)."""
    return chain + lds + -(-nparts // COLSUM_MID) + 2 + 4 + 16


def ln_bwd_depth(rows):
    blocks = ln_bwd_blocks(rows)
    return colsum_depth(-(-rows // (blocks * LN_ROWS_PER_BLOCK)), blocks, lds=3)


def gelu_bwd_depth(rows):
    gy = gelu_bwd_gy(rows)
    return colsum_depth(-(-rows // gy), gy)


# ---- marked rows --------------------------------------------------------------------------------------------------------
def mark_rows(rows, stride, cap, limit=24):
    """Boundary rows of a grid-stride row walk: first and last, both sides of the cap, the starts of the first and last
    passes, the rows of the last pass (whose prefetch is clamped to rows - 1 in the exact-width LayerNorm kernels), the
    unroll-group starts. At most `limit` rows (so that marks 2^-k, k < limit, add up exactly in f32)."""
    cand = [0, rows - 1, cap - 1, cap, cap + 1, 1, rows - 2, stride - 1, stride, 2 * stride, 3 * stride, 4 * stride - 1,
            4 * stride, rows - stride - 1, rows - stride, rows - stride + 1, (rows - 1) // stride * stride,
            (rows - 1) // stride * stride - 1, rows // 2, 2 * stride - 1, 3 * stride - 1, 5 * stride + 1]
    out = []
    for r in cand:
        if 0 <= r < rows and r not in out:
            out.append(r)
    return out[:limit]


def mark_values(n, cols, device, sign_seed=0):
    """[n, cols] float32: mark k carries +-2^-k (the sign varies along the columns)."""
    g = torch.Generator().manual_seed(sign_seed)
    sign = torch.randint(0, 2, (n, cols), generator=g).float() * 2 - 1
    return (sign * torch.tensor([2.0 ** -k for k in range(n)])[:, None]).to(device)


def decode_marks(got, want, marks):
    """Names the marked rows whose bit is wrong in a column sum of +-2^-k marks (empty when got == want)."""
    diff = (got.double() - want.double()).abs().max().item()
    if diff == 0:
        return []
    bad = [marks[k] for k in range(len(marks)) if math.floor(diff / 2.0 ** -k + 1e-9) % 2 == 1] or ['(not a mark bit)']
    return bad


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------
def ln_sum64(x, x2=None, bias=None):
    s = x.double()
    if x2 is not None:
        s = s + x2.double()
    if bias is not None:
        s = s + bias.double()
    return s


def ln_sum_f32(x, x2=None, bias=None):
    """The kernels' f32 sum: (x + x2) + bias, one rounding per addition."""
    s = x.float()
    if x2 is not None:
        s = s + x2.float()
    if bias is not None:
        s = s + bias.float()
    return s


def ln_fwd_ref(s64, gamma, beta, eps):
    """float64 LayerNorm of rows s64 (biased variance, eps inside the square root): y, mean, rstd."""
    mu = s64.mean(-1, keepdim=True)
    d = s64 - mu
    var = (d * d).mean(-1, keepdim=True)
    rs = torch.rsqrt(var + eps)
    return d * rs * gamma.double() + beta.double(), mu[:, 0], rs[:, 0]


def ln_fwd_bounds(s64, absum, n_add, gamma, beta, eps, cols, dtype):
    """Error model of ln_fwd_kernel / ln_fwd_exact_kernel against ln_fwd_ref(s64).

    absum: |x| + |x2| + |bias| (float64); n_add: f32 additions forming the row (0: the kernel normalises exactly s64).
      ds  = n_add u absum                         the row's f32 sum
      dmu = mean(ds) + (nl + 8) u mean(absum)     nl = VPL W terms per lane, 6 butterfly levels, x inv_cols (2 roundings)
      e   = ds + u |d|                            d^ = s^ - mu^ per element, beside the common shift dmu
      dvar = (nl + 8) u var + 2 mean(|d| e) + mean((e + dmu)^2)      (sum d = 0: dmu enters at second order only)
      rel_rs = (dvar + u (var + eps)) / (2 (var + eps)) + 2 u       + eps, rsqrtf (<= 1 ulp), the square root halves
      y: |g| rs (e + dmu + |d| rel_rs) + u |g d rs| + u |y|, then rounding to the stored type (u_out).
    Returns (y bound [rows, cols], mean bound [rows], rstd bound [rows])."""
    nl = math.prod(ln_dispatch(cols))
    mu = s64.mean(-1, keepdim=True)
    d = s64 - mu
    var = (d * d).mean(-1, keepdim=True)
    rs = torch.rsqrt(var + eps)
    ds = n_add * U * absum
    dmu = ds.mean(-1, keepdim=True) + (nl + 8) * U * absum.mean(-1, keepdim=True)
    e = ds + U * d.abs()
    dvar = (nl + 8) * U * var + 2 * (d.abs() * e).mean(-1, keepdim=True) + ((e + dmu) ** 2).mean(-1, keepdim=True)
    rel_rs = (dvar + U * (var + eps)) / (2 * (var + eps)) + 2 * U
    g = gamma.double().abs()
    y = d * rs * gamma.double() + beta.double()
    ey = g * rs * (e + dmu + d.abs() * rel_rs) + U * (g * d.abs() * rs) + U * y.abs()
    ey = ey + U_OUT[dtype] * (y.abs() + ey)
    return ey, dmu[:, 0], (rel_rs * rs)[:, 0]


def ln_bwd_ref(dy, s64, gamma, mean, rstd, dadd=None):
    """float64 LayerNorm backward at GIVEN mean / rstd (the f32 values the kernel reads): dx_plain, dx, and the row terms
    dy * xhat of dgamma."""
    xh = (s64 - mean.double()[:, None]) * rstd.double()[:, None]
    dg = dy.double() * gamma.double()
    c1 = dg.mean(-1, keepdim=True)
    c2 = (dg * xh).mean(-1, keepdim=True)
    rs = rstd.double()[:, None]
    dxp = rs * (dg - c1 - xh * c2)
    dx = dxp + dadd.double() if dadd is not None else dxp
    return dxp, dx, dy.double() * xh


def ln_bwd_bounds(dy, s64, absum, n_add, gamma, mean, rstd, dadd, cols, dtype):
    """Error model of ln_bwd_kernel / ln_bwd_exact_kernel against ln_bwd_ref (same mean / rstd).
      e_xh = rs (n_add u absum + u |s - mu|) + u |xh|            xh^ = ((s^ - mu) rs), two roundings beside the sum's
      dc1  = (nl + 9) u mean|dy g|                               c1 = sum(dy g) / cols
      dc2  = mean(|dy g| e_xh) + (nl + 9) u mean|dy g xh|        c2 = sum fma(dy g, xh) / cols
      dx_plain = rs fma(-xh, c2, dy g - c1):
           rs (u |dy g| + dc1 + u |dy g - c1| + |xh| dc2 + e_xh |c2| + u |inner|) + u |dx_plain|
      dx = dx_plain + dadd: + u |dx|; each stored value then rounds (u_out).
    Returns (dx_plain bound, dx bound, per-element bound of the dgamma terms dy xh)."""
    nl = math.prod(ln_dispatch(cols))
    rs = rstd.double()[:, None]
    d = s64 - mean.double()[:, None]
    xh = d * rs
    e_xh = rs * (n_add * U * absum + U * d.abs()) + U * xh.abs()
    dg = dy.double() * gamma.double()
    c1 = dg.mean(-1, keepdim=True)
    c2 = (dg * xh).mean(-1, keepdim=True)
    dc1 = (nl + 9) * U * dg.abs().mean(-1, keepdim=True)
    dc2 = (dg.abs() * e_xh).mean(-1, keepdim=True) + (nl + 9) * U * (dg * xh).abs().mean(-1, keepdim=True)
    inner = dg - c1 - xh * c2
    dxp = rs * inner
    ep = rs * (U * dg.abs() + dc1 + U * (dg - c1).abs() + xh.abs() * dc2 + e_xh * c2.abs() + U * inner.abs()) + \
        U * dxp.abs()
    ex = ep
    dx = dxp
    if dadd is not None:
        dx = dxp + dadd.double()
        ex = ep + U * dx.abs()
    uo = U_OUT[dtype]
    et = dy.double().abs() * e_xh + U * (dy.double() * xh).abs()
    return ep + uo * (dxp.abs() + ep), ex + uo * (dx.abs() + ex), et


# ---- bias + QuickGELU ---------------------------------------------------------------------------------------------------
def gelu_ref(u, bias=None):
    """a = y sigmoid(1.702 y), y = u + bias; f = da/dy = s + 1.702 y s (1 - s)  (float64)."""
    y = u.double() + (bias.double() if bias is not None else 0)
    s = torch.sigmoid(1.702 * y)
    return y * s, s + 1.702 * y * s * (1 - s)


def gelu_bounds(u, bias, dtype):
    """Error model of bias_gelu_fwd_kernel / bias_gelu_bwd_kernel (sigmoid = rcp(1 + __expf(-t)), t = 1.702f y):
      t    relative 3 u                           y = u + b, the f32 constant 1.702f, the product
      e    relative (2 |t| + 4) u + 3 u |t|       __expf = exp2(t log2e): the product's rounding is |t| u absolute in the
                                                   exponent, log2e's another, v_exp_f32 <= 1 ulp (4 u in all); t's own error
      s    relative (1 - s) rel_e + 3 u            1 + e, rcp <= 1 ulp
      a = y s:  |a| (rel_s + 2 u), then rounding (u_out)
      f = s + t s (1 - s) (contractions allowed):  s rel_s (1 + |t| |1 - 2 s|) + 6 u |t| s (1 - s) + u (s + |t s (1 - s)|)
      du = da f: |da| ef + u |du|, then rounding (u_out).
    Returns (a bound, bound of f, i.e. du bound per unit |da| before the final rounding)."""
    y = u.double() + (bias.double() if bias is not None else 0)
    t = 1.702 * y
    s = torch.sigmoid(t)
    rel_s = (1 - s) * ((5 * t.abs() + 4) * U) + 3 * U
    a = y * s
    uo = U_OUT[dtype]
    ea = a.abs() * (rel_s + 2 * U)
    ea = ea + uo * (a.abs() + ea)
    q = t.abs() * s * (1 - s)
    ef = s * rel_s * (1 + t.abs() * (1 - 2 * s).abs()) + 6 * U * q + U * (s + q)
    return ea, ef


def gelu_du_bound(da, f, ef, dtype):
    du = da.double() * f
    e = da.double().abs() * ef + U * du.abs()
    return e + U_OUT[dtype] * (du.abs() + e)


# ---- f32-class operand split --------------------------------------------------------------------------------------------
def split3_ref(x):
    """h = bf16(x), l = bf16(x - h) (the f32 subtraction is exact); inf / nan leave l = 0."""
    h = x.to(torch.bfloat16)
    hf = h.float()
    l = torch.where(hf.abs() <= 3.38e38, x - hf, torch.zeros_like(x)).to(torch.bfloat16)
    return h, l


# ---- lvl_layernorm_bwd against the models above (test_gpu_rowops_at_scale.py, test_gpu_large_operands.py) ------------------
def row_chunks(rows, cols):
    step = max(1, (1 << 25) // max(cols, 1))
    return [(r, min(r + step, rows)) for r in range(0, rows, step)]


def ln_bwd_check(within, tag, dt, out, dy, x, x2, b, gamma, mean, rstd, dadd, plain):
    """One lvl_layernorm_bwd result (out = dx, dx_plain, dgamma, dbeta, dxsum) against float64, in row chunks: dx, dx_plain
    elementwise and dgamma / dbeta / dxsum within the error models above. within(name, got, want, bound, what): the caller's
    assertion |got - want| <= 2 bound (test_gpu_rowops_at_scale._within records the worst ratio)."""
    dx, dxp, dgamma, dbeta, dxsum = out
    rows, cols = x.shape
    n_add = (1 if x2 is not None else 0) + (1 if b is not None else 0)
    sg, sb, sx = (torch.zeros(cols, dtype=torch.float64, device=x.device) for _ in range(3))
    ag, ab, ax = (torch.zeros(cols, dtype=torch.float64, device=x.device) for _ in range(3))
    eg = torch.zeros(cols, dtype=torch.float64, device=x.device)
    for r0, r1 in row_chunks(rows, cols):
        sl = slice(r0, r1)
        s64 = ln_sum64(x[sl], x2[sl] if x2 is not None else None, b)
        absum = x[sl].double().abs() + (x2[sl].double().abs() if x2 is not None else 0) + \
            (b.double().abs() if b is not None else 0)
        da = dadd[sl] if dadd is not None else None
        dxp64, dx64, t64 = ln_bwd_ref(dy[sl], s64, gamma, mean[sl], rstd[sl], da)
        ep, ex, et = ln_bwd_bounds(dy[sl], s64, absum, n_add, gamma, mean[sl], rstd[sl], da, cols, dt)
        within(f'ln_bwd dx {str(dt)[6:]}', dx[sl], dx64, ex, tag)
        if plain:
            within(f'ln_bwd dx_plain {str(dt)[6:]}', dxp[sl], dxp64, ep, tag)
        own = (dxp if plain else dx)[sl].double()         # dxsum sums the kernel's own rounded output
        sg += t64.sum(0); ag += t64.abs().sum(0); eg += et.sum(0)
        sb += dy[sl].double().sum(0); ab += dy[sl].double().abs().sum(0)
        sx += own.sum(0); ax += own.abs().sum(0)
    # column sums: f32 chains of depth D (rows per wave, LDS combine, both colsum stages): D u sum|term|
    depth = ln_bwd_depth(rows)
    within('ln_bwd dgamma', dgamma, sg, eg + (depth + 1) * U * ag, tag)
    within('ln_bwd dbeta', dbeta, sb, depth * U * ab, tag)
    within('ln_bwd dxsum', dxsum, sx, depth * U * ax, tag)
