"""GPU (-m gpu): selective activation recompute (use_checkpoint='selective').

The mode keeps neither the three LayerNorm outputs of a video block nor its MLP hidden activation and rebuilds each of
them right before the weight-gradient GEMM that reads it (lvl_layernorm_apply, lvl_quickgelu_apply). Everything here is
an equality: a rebuilt tensor must be the forward's tensor to the bit, so the kernels are compared with the forward kernels
(`torch.equal`), the autograd functions with the same arithmetic composed from raw calls that keep everything, the float32
model with its plain step. The bf16 step is not bit-equal to the plain bf16 step (the selective MLP activates the fc1
output after its rounding to bf16, the plain one before) and is held to the float32 oracle with the plain step's bounds.
Inputs carry NaN rows behind their last row and outputs sentinel rows, as in test_gpu_rowops_at_scale.py."""
import contextlib
import ctypes
import io
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import load_golden
from helpers import build_model, fixture_weights
from oracle import oracle as O
from oracle.gen_golden import synthetic_inputs

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PAD = 3
SENT = -1536.0                       # exact in bf16 and f32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _C():
    from lavila_amd import _cabi as C
    return C


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _padded(x):
    buf = torch.full((x.shape[0] + PAD, *x.shape[1:]), float('nan'), dtype=x.dtype, device=DEV)
    buf[:x.shape[0]] = x
    return buf[:x.shape[0]]


def _sentinel_out(rows, cols, dtype):
    buf = torch.full((rows + PAD, cols), SENT, dtype=dtype, device=DEV)
    buf[:rows] = float('nan')
    return buf


def _check_out(buf, rows, want, what):
    assert bool((buf[rows:] == SENT).all()), f'{what}: wrote behind the last row'
    got = buf[:rows]
    if not torch.equal(got, want):
        bad = (got != want) & ~(got.isnan() & want.isnan())
        idx = bad.nonzero()
        raise AssertionError(f'{what}: {int(bad.sum())} of {got.numel()} elements differ; first at {idx[0].tolist()}: '
                             f'{got[tuple(idx[0])].item()!r} != {want[tuple(idx[0])].item()!r}')
    assert not bool(got.isnan().any()), f'{what}: NaN in the output (unwritten, or a row read past the end)'


# ==== lvl_layernorm_apply against lvl_layernorm_fwd ========================================================================
FORMS = ('x', 'x_x2', 'x_x2_bias', 'kept_sum')


def _ln_case(rows, cols, dtype, form, seed):
    """Operands of one forward call (padded with NaN rows), its results, and the operands the apply call gets."""
    from lavila_amd import ops
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = _padded((2 * torch.randn(rows, cols, generator=g, device=DEV) + 0.5).to(dtype))
    x2 = _padded(torch.randn(rows, cols, generator=g, device=DEV).to(dtype)) if form != 'x' else None
    xb = 0.1 * torch.randn(cols, generator=g, device=DEV) if form in ('x_x2_bias', 'kept_sum') else None
    gamma = 1 + 0.2 * torch.randn(cols, generator=g, device=DEV)
    beta = 0.3 * torch.randn(cols, generator=g, device=DEV)
    y, s, mean, rstd = ops.layernorm_fwd_raw(x, x2, xb, gamma, beta, 1e-6, form == 'kept_sum')
    if form == 'kept_sum':
        return y, (_padded(s), None, None, gamma, beta, mean, rstd)
    return y, (x, x2, xb, gamma, beta, mean, rstd)


def _apply(operands, rows, cols, dtype, what):
    C = _C()
    x, x2, xb, gamma, beta, mean, rstd = operands
    out = _sentinel_out(rows, cols, dtype)
    C.check(C.lib().lvl_layernorm_apply(_p(x), _p(x2), _p(xb), _p(gamma), _p(beta), _p(mean), _p(rstd), _p(out), rows, cols,
                                        C.dtype_code(x), C.stream_ptr()), 'lvl_layernorm_apply')
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('cols', [8, 264, 768, 1024, 1032, 4096])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
def test_layernorm_apply_equals_the_forward(dtype, cols, form):
    rows = 5
    y, operands = _ln_case(rows, cols, dtype, form, seed=cols + len(form))
    _check_out(_apply(operands, rows, cols, dtype, form), rows, y, f'layernorm_apply {form} {cols} columns')
    # the public wrapper is the same call
    from lavila_amd import ops
    assert torch.equal(ops.layernorm_apply_raw(*operands), y)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('rows', [200960, 803072])          # the token rows of the benched steps: 256 clips of 4 x 196 + 1 and of 16 x 196 + 1
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
def test_layernorm_apply_past_the_grid_caps(dtype, rows, form):
    cols = 768
    y, operands = _ln_case(rows, cols, dtype, form, seed=rows % 1000 + len(form))
    _check_out(_apply(operands, rows, cols, dtype, form), rows, y, f'layernorm_apply {form} {rows} rows')


_CHILD = r'''
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
from lavila_amd import ops
out = {}
for dtype in (torch.bfloat16, torch.float32):
    for cols in (768, 1024):
        for form in ('x', 'x_x2_bias'):
            g = torch.Generator().manual_seed(cols + len(form))
            rows = 37
            x = (2 * torch.randn(rows, cols, generator=g) + 0.5).to(dtype).cuda()
            x2 = torch.randn(rows, cols, generator=g).to(dtype).cuda() if form != 'x' else None
            xb = (0.1 * torch.randn(cols, generator=g)).cuda() if form != 'x' else None
            gamma, beta = (1 + 0.2 * torch.randn(cols, generator=g)).cuda(), (0.3 * torch.randn(cols, generator=g)).cuda()
            y, _, mean, rstd = ops.layernorm_fwd_raw(x, x2, xb, gamma, beta, 1e-6, False)
            ya = ops.layernorm_apply_raw(x, x2, xb, gamma, beta, mean, rstd)
            torch.cuda.synchronize()
            out[(str(dtype), cols, form)] = tuple(t.cpu() if t is not None else None for t in (x, x2, xb, gamma, beta, y, mean, rstd, ya))
torch.save(out, sys.argv[2])
'''


def test_layernorm_apply_crosses_the_two_kernel_families(tmp_path):
    """A child process with LAVILA_LN_EXACT=0 runs the general forward and the general apply kernel at the exact widths;
    this process runs the exact-width ones on the same operands: the four results agree to the bit."""
    from lavila_amd import ops
    if os.environ.get('LAVILA_LN_EXACT') == '0':
        pytest.skip('this process itself runs the general kernels')
    script, path = tmp_path / 'child.py', tmp_path / 'general.pt'
    script.write_text(_CHILD)
    env = dict(os.environ, LAVILA_LN_EXACT='0')
    subprocess.run([sys.executable, str(script), ROOT, str(path)], env=env, check=True, timeout=300)
    res = torch.load(path, weights_only=False)
    assert len(res) == 8
    for key, (x, x2, xb, gamma, beta, y_g, mean_g, rstd_g, ya_g) in res.items():
        d = lambda t: None if t is None else t.to(DEV)
        x, x2, xb, gamma, beta, y_g, mean_g, rstd_g, ya_g = map(d, (x, x2, xb, gamma, beta, y_g, mean_g, rstd_g, ya_g))
        y_e, _, mean_e, rstd_e = ops.layernorm_fwd_raw(x, x2, xb, gamma, beta, 1e-6, False)
        ya_e = ops.layernorm_apply_raw(x, x2, xb, gamma, beta, mean_g, rstd_g)         # exact apply on the general statistics
        assert torch.equal(mean_e, mean_g) and torch.equal(rstd_e, rstd_g), key
        assert torch.equal(y_e, y_g) and torch.equal(ya_g, y_g) and torch.equal(ya_e, y_g), key


# ==== lvl_quickgelu_apply against the GEMM epilogue ============================================================================
@pytest.mark.parametrize('N', [3072, 4096])
@pytest.mark.parametrize('f32', [False, True], ids=['bf16', 'f32class'])
def test_quickgelu_apply_equals_the_gemm_epilogue(f32, N):
    from lavila_amd import ops
    C = _C()
    M, K = 3 * 785, 768
    assert M % 256 != 0
    g = torch.Generator(device=DEV).manual_seed(N + int(f32))
    x = torch.randn(M, K, generator=g, device=DEV)
    w = torch.randn(N, K, generator=g, device=DEV) * (2.0 * K ** -0.5)         # pre-activations of a few units
    b = torch.randn(N, generator=g, device=DEV)
    if f32:
        y, u = ops.linear_tn_raw(ops.split3(x, 0), ops.split3(w, 1), b, C.EPI_BIAS_QUICKGELU, f32=True)
    else:
        y, u = ops.linear_tn_raw(x.bfloat16(), w.bfloat16(), b, C.EPI_BIAS_QUICKGELU)
    assert u.abs().max() > 4 and bool((u < -3).any())       # both tails of the sigmoid are exercised
    u = _padded(u)
    out = _sentinel_out(M, N, u.dtype)
    C.check(C.lib().lvl_quickgelu_apply(_p(u), _p(out), M, N, C.dtype_code(u), C.stream_ptr()), 'lvl_quickgelu_apply')
    torch.cuda.synchronize()
    _check_out(out, M, y, f'quickgelu_apply {"f32" if f32 else "bf16"} N={N}')
    assert torch.equal(ops.quickgelu_apply_raw(u), y)


def test_quickgelu_apply_whole_tensor_equals_row_slices():
    """200 960 x 3072 bf16 (fc1's output in the benched step) lies beyond the grid cap; the kernel is row-independent, so
    a grid-stride error shows as a difference between the whole tensor's result and the results of its row slices."""
    from lavila_amd import ops
    C = _C()
    M, N = 200960, 3072
    g = torch.Generator(device=DEV).manual_seed(5)
    u = _padded((3 * torch.randn(M, N, generator=g, device=DEV)).bfloat16())
    out = _sentinel_out(M, N, torch.bfloat16)
    C.check(C.lib().lvl_quickgelu_apply(_p(u), _p(out), M, N, C.dtype_code(u), C.stream_ptr()), 'lvl_quickgelu_apply')
    torch.cuda.synchronize()
    assert bool((out[M:] == SENT).all()) and not bool(out[:M].isnan().any())
    cuts = [0, 1, 5, 2355, 40000, 40003, 131072, 200959, M]
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        assert torch.equal(ops.quickgelu_apply_raw(u[r0:r1]), out[r0:r1]), (r0, r1)
    # and it is QuickGELU: against float64 within the bf16 rounding of the result (+ the 1-ulp exp / rcp)
    ud = u[:4096].double()
    want = ud * torch.sigmoid(1.702 * ud)
    assert bool(((out[:4096].double() - want).abs() <= 2.0 ** -8 * want.abs() + 1e-30).all())


# ==== the autograd functions against raw calls that keep everything ============================================================
ROWS, D = 3 * 785, 768


def _param(g, *shape, scale=1.0, shift=0.0):
    return (shift + scale * torch.randn(*shape, generator=g, device=DEV)).requires_grad_(True)


def test_selective_mlp_function_equals_raw_composition():
    """norm2 -> selective _MlpResidualLayerNormFn (fc1 + QuickGELU, fc2 + residual, norm3) -> qkv Linear, forward and
    backward, against linear_tn_raw (epilogues 1, 3, 2) / layernorm_fwd_raw / layernorm_bwd_raw / linear_wgrad_raw on kept
    a, h2, h3."""
    from lavila_amd import ops
    C = _C()
    g = torch.Generator(device=DEV).manual_seed(11)
    x1 = torch.randn(3, 785, D, generator=g, device=DEV).bfloat16().requires_grad_(True)
    g2, be2 = _param(g, D, scale=0.2, shift=1.0), _param(g, D, scale=0.3)
    g3, be3 = _param(g, D, scale=0.2, shift=1.0), _param(g, D, scale=0.3)
    w1, b1 = _param(g, 4 * D, D, scale=D ** -0.5), _param(g, 4 * D, scale=0.5)
    w2, b2 = _param(g, D, 4 * D, scale=(4 * D) ** -0.5), _param(g, D, scale=0.5)
    wq, bq = _param(g, 3 * D, D, scale=D ** -0.5), _param(g, 3 * D, scale=0.5)
    dq = torch.randn(3, 785, 3 * D, generator=g, device=DEV).bfloat16()
    ds = torch.randn(3, 785, D, generator=g, device=DEV).bfloat16()
    eps = 1e-6
    leaves = [x1, g2, be2, w1, b1, w2, b2, g3, be3, wq, bq]

    h2, r2 = ops.layer_norm(x1, g2, be2, eps, recipe=True)
    s, h3, r3 = ops.mlp_residual_layer_norm(h2, w1, b1, w2, b2, x1, g3, be3, eps, ln=r2, recipe=True)
    q = ops.linear(h3, wq, bq, ln=r3)
    del h2, h3
    torch.autograd.backward([q, s], [dq, ds])
    torch.cuda.synchronize()
    got = [s.detach(), q.detach()] + [t.grad for t in leaves]

    with torch.no_grad():
        X = x1.detach().reshape(ROWS, D)
        w1b, w1t = ops.weight_copies(w1)
        w2b, w2t = ops.weight_copies(w2)
        wqb, wqt = ops.weight_copies(wq)
        kh2, _, m2, rs2 = ops.layernorm_fwd_raw(X, None, None, g2.detach(), be2.detach(), eps, False)
        ka, ku = ops.linear_tn_raw(kh2, w1b, b1.detach(), C.EPI_BIAS_QUICKGELU)
        ks = ops.linear_tn_raw(ka, w2b, b2.detach(), C.EPI_BIAS_RESIDUAL, aux_in=X)
        kh3, _, m3, rs3 = ops.layernorm_fwd_raw(ks, None, None, g3.detach(), be3.detach(), eps, False)
        kq = ops.linear_tn_raw(kh3, wqb, bq.detach(), C.EPI_BIAS)
        dq2, ds2 = dq.reshape(ROWS, 3 * D), ds.reshape(ROWS, D)
        dh3 = ops.linear_tn_raw(dq2, wqt, None, C.EPI_BIAS)
        dwq = ops.linear_wgrad_raw(dq2, kh3, False)[0]
        dbq = dq2.sum(0, dtype=torch.float32)
        dsum, dg3, dbe3, db2 = ops.layernorm_bwd_raw(dh3, ks, None, None, g3.detach(), m3, rs3, ds2, True)
        du, db1 = ops.linear_tn_raw(dsum, w2t, None, C.EPI_QUICKGELU_BWD, aux_in=ku)
        dw2 = ops.linear_wgrad_raw(dsum, ka, False)[0]
        dh2 = ops.linear_tn_raw(du, w1t, None, C.EPI_BIAS)
        dw1 = ops.linear_wgrad_raw(du, kh2, False)[0]
        dx_ln, dg2, dbe2, _ = ops.layernorm_bwd_raw(dh2, X, None, None, g2.detach(), m2, rs2, None, False)
    torch.cuda.synchronize()
    want = {'s': ks.reshape(3, 785, D), 'q': kq.reshape(3, 785, 3 * D), 'g2': dg2, 'be2': dbe2, 'w1': dw1, 'b1': db1, 'w2': dw2,
            'b2': db2, 'g3': dg3, 'be3': dbe3, 'wq': dwq, 'bq': dbq}
    names = ['s', 'q', 'x1', 'g2', 'be2', 'w1', 'b1', 'w2', 'b2', 'g3', 'be3', 'wq', 'bq']
    for name, t in zip(names, got):
        assert t is not None, name
        if name == 'x1':        # two gradients arrive at x1 (the residual's and norm2's); their bf16 sum in either order
            assert torch.equal(t.reshape(ROWS, D), dsum + dx_ln), name
        else:
            assert torch.equal(t, want[name]), name


def test_selective_layernorm_linear_site_equals_raw_composition():
    """norm1 (x + y_t + b_t, the three-operand form) -> qkv Linear with the recipe, against the raw calls on a kept h1."""
    from lavila_amd import ops
    C = _C()
    g = torch.Generator(device=DEV).manual_seed(12)
    x = torch.randn(3, 785, D, generator=g, device=DEV).bfloat16().requires_grad_(True)
    y = torch.randn(3, 785, D, generator=g, device=DEV).bfloat16().requires_grad_(True)
    yb = _param(g, D, scale=0.5)
    g1, be1 = _param(g, D, scale=0.2, shift=1.0), _param(g, D, scale=0.3)
    wq, bq = _param(g, 3 * D, D, scale=D ** -0.5), _param(g, 3 * D, scale=0.5)
    dq = torch.randn(3, 785, 3 * D, generator=g, device=DEV).bfloat16()
    eps = 1e-6
    _, h1, r1 = ops.add_layer_norm_pass(x, y, yb, g1, be1, eps, recipe=True)
    q = ops.linear(h1, wq, bq, ln=r1)
    del h1
    q.backward(dq)
    with torch.no_grad():
        wqb, wqt = ops.weight_copies(wq)
        kh, _, m, rs = ops.layernorm_fwd_raw(x.detach(), y.detach(), yb.detach(), g1.detach(), be1.detach(), eps, False)
        kq = ops.linear_tn_raw(kh.reshape(ROWS, D), wqb, bq.detach(), C.EPI_BIAS)
        dq2 = dq.reshape(ROWS, 3 * D)
        dh = ops.linear_tn_raw(dq2, wqt, None, C.EPI_BIAS)
        dwq = ops.linear_wgrad_raw(dq2, kh.reshape(ROWS, D), False)[0]
        dx, dg, db, dsum = ops.layernorm_bwd_raw(dh.reshape(3, 785, D), x.detach(), y.detach(), yb.detach(), g1.detach(), m, rs,
                                                 None, True)
    torch.cuda.synchronize()
    assert torch.equal(q.detach().reshape(ROWS, 3 * D), kq)
    for name, a, b in (('x', x.grad, dx), ('y', y.grad, dx), ('yb', yb.grad, dsum), ('g1', g1.grad, dg), ('be1', be1.grad, db),
                       ('wq', wq.grad, dwq), ('bq', bq.grad, dq2.sum(0, dtype=torch.float32))):
        assert torch.equal(a, b), name


# ==== the model ===================================================================================================================
def _poison():
    """1 GiB of NaN allocated and freed: what the caching allocator hands out next (the rebuilt tensors) starts as NaN."""
    t = torch.full((1 << 28,), float('nan'), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    del t


@pytest.mark.parametrize('name', ['tiny_p16', 'tiny_f16', 'tiny_p14_gated', 'tsfb_224_f16_b2_spread'])
def test_f32_selective_step_equals_the_plain_step(name):
    """float32: the plain MLP already activates the unrounded f32 pre-activation it keeps, so selective and plain run the
    same arithmetic and must agree to the bit -- on the f32-class kernels (width 768) and on the library-GEMM / composed
    paths of the tiny fixtures (tanh gating included)."""
    from lavila.models.loss import CLIPLoss
    fx = load_golden(f'model_{name}.pt')
    c = fx['config']
    model = build_model(c)
    model.load_state_dict(fixture_weights(fx), strict=True)
    model.to(DEV).train()
    video, tokens = synthetic_inputs(c, seed=fx['input_seed'])
    video, tokens = video.to(DEV), tokens.to(DEV)
    runs = {}
    for mode in (False, 'selective'):
        model.zero_grad(set_to_none=True)
        out = model(video, tokens, use_checkpoint=mode, norm_embed=True)
        loss = CLIPLoss(use_vissl=False, cache_labels=True, rank=0, world_size=1)(out)['loss']
        if mode:
            _poison()
        loss.backward()
        torch.cuda.synchronize()
        runs[mode] = (loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()})
    assert torch.equal(runs[False][0], runs['selective'][0])
    assert torch.isfinite(runs['selective'][0])
    for k, gp in runs[False][1].items():
        assert torch.equal(gp, runs['selective'][1][k]), k


def test_tsfb_bf16_selective_step_vs_oracle_f32():
    """The step of test_gpu_parity_bf16.test_tsfb_bf16_training_step_vs_oracle_f32 (same model, seeds, batch) with
    use_checkpoint='selective', against the float32 oracle with that test's bounds and its treatment of near-zero
    gradients. Its error model counts "the MLP hidden pair" among the ~10 roundings of the token stream per block:
    the plain step rounds a = QuickGELU(u) and quickgelu'(u); the selective step rounds u and a = QuickGELU(round(u)),
    the reference's AMP arithmetic -- the same number of independent O(2^-9) perturbations, none added. Two selective
    runs agree to the bit."""
    from lavila.models import models
    from lavila.models.loss import CLIPLoss
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        model = models.CLIP_OPENAI_TIMESFORMER_BASE(num_frames=4, project_embed_dim=256)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    w = O.procedural_weights(shapes, seed=17)
    model.load_state_dict(w)
    model.to(DEV).train()
    B = 4
    video, tokens = O.synthetic_batch(B, 4, 224, seed=31)
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            out = model(video.to(DEV), tokens.to(DEV), use_checkpoint='selective', norm_embed=True)
            crit = CLIPLoss()
            ld = crit(out)
        _poison()
        ld['loss'].backward()
        dbg = crit.debug_slabs(out)
        torch.cuda.synchronize()
        runs.append((ld['loss'].detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for k, gp in runs[0][1].items():
        assert torch.equal(gp, runs[1][1][k]), f'two selective runs differ in {k}'

    torch.set_num_threads(min(32, torch.get_num_threads() or 1))
    wo = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in w.items()}
    oo = O.clip_forward(video, tokens, wo, 12, 8, norm_embed=True)
    lo = O.clip_loss(oo['image_embed'], oo['text_embed'], oo['logit_scale'])
    lo['loss'].backward()

    def rel(a, b):
        return ((a.float().cpu() - b).norm() / b.norm().clamp_min(1e-30)).item()
    e_img, e_txt = rel(out['image_embed'], oo['image_embed'].detach()), rel(out['text_embed'], oo['text_embed'].detach())
    dlogit = (dbg['logits'][0].cpu() - lo['logits_per_image'].detach()).abs().max().item()
    dloss = abs(ld['loss'].item() - lo['loss'].item())
    worst, num, den = [], 0.0, 0.0
    grads = dict(model.named_parameters())
    for k, p in wo.items():
        if not p.requires_grad:
            continue
        got, want = grads[k].grad, p.grad
        assert got is not None and torch.isfinite(got).all(), k
        d = (got.float().cpu() - want).norm().item()
        num += d * d
        den += want.norm().item() ** 2
        worst.append((d / max(want.norm().item(), 1e-30), d, want.norm().item(), k))
    agg = math.sqrt(num / den)
    scale = math.sqrt(den / len(worst))            # RMS gradient norm of a parameter tensor
    bad = [(r, d, n, k) for r, d, n, k in worst if r > 1e-1 and d > 1e-3 * scale]
    worst.sort(reverse=True)
    print(f'[bf16 TSF-B step, selective recompute] rel L2: image_embed {e_img:.2e} text_embed {e_txt:.2e}; max |d logit| '
          f'{dlogit:.3f}; |d loss| {dloss:.2e}; gradients: aggregate {agg:.2e}, worst {worst[0][0]:.2e} ({worst[0][3]}), '
          f'median {worst[len(worst) // 2][0]:.2e} over {len(worst)} tensors')
    assert e_img < 2.5e-2 and e_txt < 2.5e-2, (e_img, e_txt)
    assert dlogit < 0.1 and dloss < 2e-2, (dlogit, dloss)
    assert torch.equal(dbg['labels'].cpu(), lo['labels'])
    top2 = lo['logits_per_image'].detach().topk(2, -1).values
    safe = (top2[:, 0] - top2[:, 1]) > 2 * 0.1
    assert torch.equal(dbg['pred'][0].cpu()[safe], lo['pred'][safe])
    assert agg < 5e-2, agg
    assert not bad, bad[:5]


def _tower(depth, dtype=torch.float32, frames=4):
    from lavila.models.openai_model import QuickGELU
    from lavila.models.timesformer import SpaceTimeTransformer
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        vis = SpaceTimeTransformer(img_size=224, patch_size=16, embed_dim=768, depth=depth, num_heads=12, num_frames=frames,
                                   time_init='rand', attention_style='frozen-in-time', ln_pre=True, act_layer=QuickGELU,
                                   num_classes=0)
    with torch.no_grad():
        for p in vis.parameters():
            if p.ndim > 1:
                p.normal_(0, 0.02)
    return vis.to(DEV).train()


def test_selective_reruns_nothing_and_keeps_seven_units_less_per_block(monkeypatch):
    """Video tower alone (width 768, depth 4, 4 x 224^2, batch 4, bf16 autocast), plain against selective: the same number
    of GEMM, attention and LayerNorm forward calls (whole-block checkpointing would double them); the storages saved for
    backward shrink by the 7 units per full block of the table in DESIGN.md (h3, h1, h2: 3; a: 4), one unit of allowance
    for beta copies and small recipe tensors; the peak of forward + backward by the same minus the one [rows, 4D] and one
    [rows, D] rebuilt tensor that may be alive at it."""
    from lavila_amd import ops
    depth, B = 4, 4
    vis = _tower(depth)
    g = torch.Generator().manual_seed(3)
    video = torch.randn(B, 3, 4, 224, 224, generator=g).to(DEV)
    counts = {}
    for fname in ('linear_tn_raw', 'divided_attn_fwd_raw', 'layernorm_fwd_raw', 'layernorm_apply_raw', 'quickgelu_apply_raw'):
        def wrap(*a, _f=getattr(ops, fname), _n=fname, **k):
            counts[_n] = counts.get(_n, 0) + 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, fname, wrap)
    res = {}
    for mode in (False, 'selective'):
        for warm in (True, False):          # the first pass of each mode warms the allocator and the weight copies
            vis.zero_grad(set_to_none=True)
            counts.clear()
            seen, nbytes = set(), 0

            def pack(t):
                nonlocal nbytes
                st = t.untyped_storage()
                if t.is_cuda and st.data_ptr() not in seen:
                    seen.add(st.data_ptr())
                    nbytes += st.nbytes()
                return t
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
                with torch.autocast('cuda', dtype=torch.bfloat16):
                    out = vis(video, use_checkpoint=mode)
                loss = out.float().sum()
            loss.backward()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            del out, loss
        res[mode] = (dict(counts), nbytes, peak)
    plain, sel = res[False], res['selective']
    for fname in ('linear_tn_raw', 'divided_attn_fwd_raw', 'layernorm_fwd_raw'):
        assert plain[0][fname] == sel[0][fname], (fname, plain[0][fname], sel[0][fname])
    assert plain[0].get('layernorm_apply_raw', 0) == 0 and plain[0].get('quickgelu_apply_raw', 0) == 0
    assert sel[0]['layernorm_apply_raw'] == 3 * (depth - 1) and sel[0]['quickgelu_apply_raw'] == depth - 1
    unit = B * 785 * 768 * 2
    d_saved, d_peak = (plain[1] - sel[1]) / unit, (plain[2] - sel[2]) / unit
    print(f'[selective recompute] depth {depth}, {B * 785} rows: saved for backward {plain[1] / unit:.1f} -> {sel[1] / unit:.1f} units '
          f'(-{d_saved:.2f}; required >= {7 * (depth - 1) - 1}); peak of forward + backward {plain[2] / unit:.1f} -> '
          f'{sel[2] / unit:.1f} units (-{d_peak:.2f}; required >= {7 * (depth - 1) - 5})')
    assert d_saved >= 7 * (depth - 1) - 1, d_saved
    assert d_peak >= 7 * (depth - 1) - 5, d_peak


def test_frozen_temporal_weights_skip_the_rebuild(monkeypatch):
    """After freeze_temporal_weights() the time qkv weight wants no gradient, h3 has no reader in backward: one
    lvl_layernorm_apply call fewer per full block; the remaining gradients equal the plain frozen step's."""
    from lavila_amd import ops
    depth, B = 3, 2
    g = torch.Generator().manual_seed(4)
    video = torch.randn(B, 3, 4, 224, 224, generator=g).to(DEV)
    n = [0]

    def wrap(*a, _f=ops.layernorm_apply_raw, **k):
        n[0] += 1
        return _f(*a, **k)
    monkeypatch.setattr(ops, 'layernorm_apply_raw', wrap)

    def step(vis, mode):
        vis.zero_grad(set_to_none=True)
        n[0] = 0
        out = vis(video, use_checkpoint=mode)
        if mode:
            _poison()
        out.sum().backward()
        torch.cuda.synchronize()
        return n[0], {k: (None if p.grad is None else p.grad.clone()) for k, p in vis.named_parameters()}
    vis = _tower(depth)
    calls_unfrozen, _ = step(vis, 'selective')
    with contextlib.redirect_stdout(io.StringIO()):
        vis.freeze_temporal_weights()
    calls_frozen, g_sel = step(vis, 'selective')
    _, g_plain = step(vis, False)
    assert calls_unfrozen == 3 * (depth - 1)
    assert calls_frozen == calls_unfrozen - (depth - 1), (calls_frozen, calls_unfrozen)
    assert any(v is not None for v in g_plain.values())
    for k, v in g_plain.items():
        if v is None:
            assert g_sel[k] is None, k
        else:
            assert torch.equal(v, g_sel[k]), k


def test_selective_refuses_the_f32_residual_stream_and_unknown_modes(monkeypatch):
    from lavila_amd import ops
    vis = _tower(2)
    video = torch.randn(1, 3, 4, 224, 224, device=DEV)
    with pytest.raises(ValueError):
        vis(video, use_checkpoint='nonsense')
    with pytest.raises(ValueError):
        vis.forward_features(video.permute(0, 2, 1, 3, 4).contiguous(), use_checkpoint='nonsense')
    c = dict(img=32, patch=16, frames=2, dim=128, depth=2, heads=2, t_width=128, t_heads=2, t_layers=2, vocab=512, embed=64,
             batch=2, gated=False)
    clip = build_model(c).to(DEV)
    v, t = O.synthetic_batch(2, 2, 32, seed=5)
    with pytest.raises(ValueError):
        clip(v.to(DEV), (t % 510 + 1).to(DEV), use_checkpoint='nonsense')
    monkeypatch.setattr(ops, 'CHECKPOINT', 'nonsense')
    with pytest.raises(ValueError):
        vis(video, use_checkpoint=True)
    monkeypatch.setattr(ops, 'CHECKPOINT', 'selective')
    monkeypatch.setattr(ops, 'RESIDUAL_F32', True)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        with pytest.raises(NotImplementedError):
            vis(video, use_checkpoint='selective')
        with pytest.raises(NotImplementedError):
            vis(video, use_checkpoint=True)            # LAVILA_CHECKPOINT=selective


def test_selective_block_is_hip_graph_capturable():
    """test_gpu_model.test_block_forward_backward_is_hip_graph_capturable with chain(selective=True): the two rebuild
    kernels are allocation-free and stream-ordered like every other entry point. Compared on what that test holds to the
    bit: the block output and the fc1 weight gradient (the operand of which is the rebuilt h2)."""
    from lavila.models.openai_model import QuickGELU
    from lavila.models.timesformer import SpaceTimeBlock
    torch.manual_seed(0)
    Fr, N, Dm, H, B = 4, 196, 768, 12, 2
    blk = SpaceTimeBlock(Dm, H, qkv_bias=True, act_layer=QuickGELU, time_init='rand').to(DEV)
    with torch.no_grad():
        for p in blk.parameters():
            if p.ndim > 1:
                p.normal_(0, 0.02)
    x_static = torch.randn(B, 1 + Fr * N, Dm, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    g_static = torch.randn(B, 1 + Fr * N, Dm, device=DEV, dtype=torch.bfloat16)

    def step():
        for p in blk.parameters():
            p.grad = None
        x_static.grad = None
        with torch.autocast('cuda', dtype=torch.bfloat16):
            x1, y, b = blk.chain(x_static, None, None, Fr, N, selective=True)
            out = x1 + y + b.to(y.dtype)
        out.backward(g_static)
        return out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_static = step()
    gw_static = blk.mlp.fc1.weight.grad
    gq_static = blk.timeattn.qkv.weight.grad
    with torch.no_grad():
        x_static.copy_(torch.randn_like(x_static))
        g_static.copy_(torch.randn_like(g_static))
    graph.replay()
    torch.cuda.synchronize()
    got = (out_static.clone(), gw_static.clone(), gq_static.clone())
    out_e = step()
    torch.cuda.synchronize()
    assert torch.equal(got[0], out_e)
    nbad = int((got[1] != blk.mlp.fc1.weight.grad).sum())
    assert nbad == 0, f'fc1 weight gradient differs in {nbad} elements'
    assert torch.isfinite(got[2]).all()
