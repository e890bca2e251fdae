"""GPU (-m gpu): the exact-GELU MLP on the fused chain -- ops.mlp(act=ops.ACT_GELU) as a function, and CLIP_HF around the
default-constructed SpaceTimeTransformer (GELU, no ln_pre, eps 1e-6: the tower of CLIP_HF_TIMESFORMER_DISTILBERT_BASE) against
the committed outputs of the unmodified reference (tests/golden/gelu_tower_clip_hf.pt) at the bars of tests/test_gpu_clip_hf.py:
float32 embeddings / loss at atol = rtol = 1e-3, gradients at 1e-4 / 5e-3; bf16 autocast at 4e-2. Reads only the fixture."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import gelu_tower_helpers as H
from test_gpu_selective_recompute import _poison

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF = torch.bfloat16
TOL = dict(atol=1e-3, rtol=1e-3)
GTOL = dict(atol=1e-4, rtol=5e-3)
ROWS, D, HID = 300, 256, 1024


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / b.double().norm().clamp_min(1e-300)).item()


# ---- the function -------------------------------------------------------------------------------------------------------------
def _mlp_operands(dtype, seed=5):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(ROWS, D, generator=g, device=DEV).to(dtype)
    w1 = torch.randn(HID, D, generator=g, device=DEV) * D ** -0.5
    b1 = torch.randn(HID, generator=g, device=DEV) * 0.5
    w2 = torch.randn(D, HID, generator=g, device=DEV) * HID ** -0.5
    dy = torch.randn(ROWS, D, generator=g, device=DEV).to(dtype)
    return x, w1, b1, w2, dy


def _run(fn, x, w1, b1, w2, dy):
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, w1, b1, w2)]
    y = fn(*leaves)
    y.backward(dy.to(y.dtype))
    torch.cuda.synchronize()
    return [y.detach()] + [t.grad for t in leaves]


def _float64(x, w1, b1, w2, dy):
    return _run(lambda x, w1, b1, w2: F.gelu(x @ w1.t() + b1) @ w2.t(), *(t.double() for t in (x, w1, b1, w2, dy)))


NAMES = ('y', 'dx', 'dw1', 'db1', 'dw2')


def test_fused_gelu_mlp_bf16_is_no_further_from_float64_than_the_composed_form():
    """ops.mlp(act=GELU) on epilogues 8 and 5 against the form the MLP ran in before (Linear + bias, torch's GELU, Linear:
    every [rows, 4D] tensor rounded to bf16 between the passes), both against float64 on the same inputs.
    y and dw2 hang on the hidden activation: the fused form rounds it once and the pre-activation not at all -- no margin.
    dx, dw1 and db1 hang on du = da * gelu'(u). The composed form rounds da, u and du; the fused form rounds gelu'(u) and du.
    That is one rounding fewer, but not a smaller one: where the gradient is largest (u > 0.75) gelu'(u) lies in [1, 1.13],
    the coarse end of a bf16 binade (spacing 2^-7, relative error up to 2^-8), while the composed form's da is spread over
    its binades (on average 0.72 of that). One of the about five equal error shares of du's path (the bf16 weights, da or
    gelu', du, the result) may therefore count up to twice: sqrt(6 / 5) = 1.095 -- a margin of 1.1 on these three.
    Measured on an MI355X (fused / composed): y 3.28e-3 / 3.81e-3, dx 4.04e-3 / 3.94e-3, dw1 3.29e-3 / 3.16e-3,
    db1 2.88e-3 / 3.40e-3, dw2 2.27e-3 / 3.00e-3."""
    from lavila_amd import ops
    ops_in = _mlp_operands(BF)
    want = _float64(*ops_in)
    fused = _run(lambda x, w1, b1, w2: ops.mlp(x, w1, b1, w2, ops.ACT_GELU), *ops_in)
    composed = _run(lambda x, w1, b1, w2: ops.linear(F.gelu(ops.linear(x, w1, b1)), w2), *ops_in)
    for name, f, c, w in zip(NAMES, fused, composed, want):
        ef, ec = _rel(f, w), _rel(c, w)
        print(f'[gelu mlp bf16] {name}: relative L2 to float64, fused {ef:.3e}, composed {ec:.3e}')
        assert ef <= (1.0 if name in ('y', 'dw2') else 1.1) * ec, (name, ef, ec)
    assert fused[0].dtype == BF and fused[3].dtype == torch.float32


def test_fused_gelu_mlp_f32_class():
    from lavila_amd import ops
    ops_in = _mlp_operands(torch.float32)
    want = _float64(*ops_in)
    with ops_guard():
        got = _run(lambda x, w1, b1, w2: ops.mlp(x, w1, b1, w2, ops.ACT_GELU), *ops_in)
    for name, g, w in zip(NAMES, got, want):
        e = _rel(g, w)
        print(f'[gelu mlp f32-class] {name}: relative L2 to float64 {e:.3e}')
        assert g.dtype == torch.float32 and e <= 1e-3, (name, e)


@contextlib.contextmanager
def ops_guard(gemm=True):
    """the fused function and nothing else: torch's GELU and (gemm) the library GEMMs raise"""
    from lavila_amd.guards import forbid_library_gemm
    real = F.gelu

    def boom(*a, **k):
        raise AssertionError('torch GELU called on the fused path')
    F.gelu = boom
    try:
        with forbid_library_gemm() if gemm else contextlib.nullcontext():
            yield
    finally:
        F.gelu = real


def _ln_params(seed=9):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return 1 + 0.2 * torch.randn(D, generator=g, device=DEV), 0.3 * torch.randn(D, generator=g, device=DEV)


def test_selective_gelu_mlp_f32_equals_the_plain_one_to_the_bit():
    """float32: plain and selective both keep the unrounded pre-activation, so they run the same arithmetic (what
    test_gpu_selective_recompute.py asserts for QuickGELU)."""
    from lavila_amd import ops
    x, w1, b1, w2, dy = _mlp_operands(torch.float32, seed=6)
    gam, bet = _ln_params()

    def plain(x, w1, b1, w2):
        return ops.mlp(ops.layer_norm(x, gam, bet, 1e-6), w1, b1, w2, ops.ACT_GELU)

    def selective(x, w1, b1, w2):
        h, rec = ops.layer_norm(x, gam, bet, 1e-6, recipe=True)
        y = ops.mlp(h, w1, b1, w2, ops.ACT_GELU, ln=rec)
        del h
        _poison()
        return y
    a, b = _run(plain, x, w1, b1, w2, dy), _run(selective, x, w1, b1, w2, dy)
    for name, p, s in zip(NAMES, a, b):
        assert torch.equal(p, s), name


def test_selective_gelu_mlp_bf16_equals_the_raw_composition():
    """bf16, selective: the function keeps u (epilogue 6), rebuilds a = lvl_act_fwd(u) and the LayerNorm output, and its
    backward is epilogue 7 -- equal to the bit to the same raw calls on kept tensors (as test_gpu_selective_recompute.py
    asserts for QuickGELU); and within the drop-path tests' bar for two modes of one step (5e-2 aggregate) of the plain
    function, which keeps gelu'(u) of the unrounded u instead."""
    from lavila_amd import _cabi as C
    from lavila_amd import ops
    x, w1, b1, w2, dy = _mlp_operands(BF, seed=7)
    gam, bet = _ln_params()

    def selective(x, w1, b1, w2):
        h, rec = ops.layer_norm(x, gam, bet, 1e-6, recipe=True)
        y = ops.mlp(h, w1, b1, w2, ops.ACT_GELU, ln=rec)
        del h
        _poison()
        return y
    got = _run(selective, x, w1, b1, w2, dy)
    with torch.no_grad():
        w1b, w1t = ops.weight_copies(w1)
        w2b, w2t = ops.weight_copies(w2)
        kh, _, mean, rstd = ops.layernorm_fwd_raw(x, None, None, gam, bet, 1e-6, False)
        ka, ku = ops.linear_tn_raw(kh, w1b, b1, C.EPI_BIAS_GELU)
        ky = ops.linear_tn_raw(ka, w2b, None, C.EPI_BIAS)
        du, db1 = ops.linear_tn_raw(dy, w2t, None, C.EPI_GELU_BWD, aux_in=ku)
        dw2 = ops.linear_wgrad_raw(dy, ka, False)[0]
        dh = ops.linear_tn_raw(du, w1t, None, C.EPI_BIAS)
        dw1 = ops.linear_wgrad_raw(du, kh, False)[0]
        dx = ops.layernorm_bwd_raw(dh, x, None, None, gam, mean, rstd, None, False)[0]
        assert torch.equal(ops.gelu_apply_raw(ku), ka)
    torch.cuda.synchronize()
    for name, g, w in zip(NAMES, got, (ky, dx, dw1, db1, dw2)):
        assert torch.equal(g, w), name
    plain = _run(lambda x, w1, b1, w2: ops.mlp(ops.layer_norm(x, gam, bet, 1e-6), w1, b1, w2, ops.ACT_GELU), x, w1, b1, w2, dy)
    for name, g, p in zip(NAMES, got, plain):
        e = _rel(g, p)
        print(f'[gelu mlp bf16] selective against plain, {name}: relative L2 {e:.2e}')
        assert e <= 5e-2, (name, e)


# ---- the golden ---------------------------------------------------------------------------------------------------------------
def _model(drop_path_rate=0.0):
    fx = H.fixture()
    m = H.build_model(fx['config'], drop_path_rate)
    m.load_state_dict(H.weights(), strict=True)
    return m.to(DEV).train()


def _step(model, amp=None, use_checkpoint=False):
    from lavila.models.loss import CLIPLoss
    video, ids, mask = H.inputs()
    model.zero_grad(set_to_none=True)
    ctx = torch.autocast('cuda', dtype=amp) if amp is not None else contextlib.nullcontext()
    with ctx:
        out = model(video.to(DEV), ids.to(DEV), mask=mask.to(DEV), use_checkpoint=use_checkpoint, norm_embed=True)
        ld = CLIPLoss(use_vissl=False, cache_labels=True, rank=0, world_size=1)(out)
    ld['loss'].backward()
    torch.cuda.synchronize()
    return out, ld, {k: p.grad.clone() for k, p in model.named_parameters()}


def _check_fp32(tag, out, ld, grads, rec):
    fx = H.fixture()
    for k in ('image_embed', 'text_embed', 'logit_scale'):
        err = (out[k].detach().cpu() - rec[k]).abs().max().item()
        print(f'[gelu tower {tag} fp32] {k}: max abs error {err:.2e}')
        torch.testing.assert_close(out[k].detach().cpu(), rec[k], **TOL, msg=lambda m, k=k: f'{k}: {m}')
    print(f'[gelu tower {tag} fp32] loss {ld["loss"].item():.6f} reference {rec["loss"].item():.6f}')
    torch.testing.assert_close(ld['loss'].detach().cpu(), rec['loss'], **TOL)
    assert all(g is not None for g in grads.values())
    assert H.check_selected(grads, rec, **GTOL, what=tag) == len(fx['param_names'])
    for k, want in rec['grad_norms'].items():
        got = grads[k].norm().item()
        assert abs(got - want) <= 5e-3 * want + 1e-6, (k, got, want)


def test_golden_step_fp32_on_the_own_gemms():
    from lavila_amd.guards import forbid_library_gemm
    fx = H.fixture()
    model = _model()
    out, ld, grads = _step(model)
    _check_fp32('plain', out, ld, grads, fx['plain'])
    # the video tower alone, forward and backward, float32: every GEMM is lavila_amd's own (f32-class mode), GELU included
    model.zero_grad(set_to_none=True)
    video = H.inputs()[0].to(DEV)
    with ops_guard():
        feat = model.visual(video)
        feat.square().sum().backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.visual.parameters())


def test_golden_step_bf16():
    fx = H.fixture()
    A = fx['plain']
    for amp in (torch.bfloat16, torch.float16):                # fp16 autocast is re-entered as bf16
        out, ld, grads = _step(_model(), amp=amp)
        for k in ('image_embed', 'text_embed'):
            err = (out[k].float().cpu() - A[k]).abs().max().item()
            print(f'[gelu tower {amp}] {k}: max abs error {err:.2e}')
            torch.testing.assert_close(out[k].detach().float().cpu(), A[k], atol=4e-2, rtol=4e-2)
        assert abs(ld['loss'].item() - A['loss'].item()) < 0.1
        for k in ('visual.blocks.0.mlp.fc1.bias', 'visual.blocks.1.mlp.fc1.bias', 'visual.patch_embed.proj.bias'):
            g = grads[k]
            assert g is not None and torch.isfinite(g).all() and g.dtype == torch.float32
            cos = F.cosine_similarity(g.float().cpu().flatten(), A['grads'][k].flatten(), dim=0)
            print(f'[gelu tower {amp}] d {k}: cosine to the reference {cos.item():.4f}')
            assert cos > 0.98, (k, cos)


def test_golden_drop_path_step_with_injected_masks(monkeypatch):
    """The record with drop_path_rate = 0.5 under the masks the reference drew: float32 at the float32 bars; in bf16 the
    block-checkpointed step equals the plain one to the bit (the same kernels on the same masks), and so does a repeat."""
    fx = H.fixture()
    model = _model(fx['config']['drop_path_rate'])
    calls = H.inject_masks(monkeypatch, model, H.fixture_scales())
    out, ld, grads = _step(model)
    assert calls == [1, 1]
    _check_fp32('drop', out, ld, grads, fx['drop'])
    assert abs(ld['loss'].item() - fx['plain']['loss'].item()) > 1e-3          # the masks matter
    runs = [_step(model, amp=BF), _step(model, amp=BF), _step(model, amp=BF, use_checkpoint='block')]
    assert calls == [1] * (2 + 2 + 2 + 4)
    for other in runs[1:]:
        assert torch.equal(runs[0][1]['loss'], other[1]['loss'])
        assert torch.equal(runs[0][0]['image_embed'], other[0]['image_embed'])
        for k, g in runs[0][2].items():
            assert torch.equal(g, other[2][k]), k
    torch.testing.assert_close(runs[0][0]['image_embed'].float().cpu(), fx['drop']['image_embed'], atol=4e-2, rtol=4e-2)


def test_gelu_tower_step_runs_on_the_gelu_epilogues(monkeypatch):
    """A bf16 training step of the default-constructed tower (depth 2: block 0's MLP deferred into block 1's norm3, block 1
    cls-only): fc1 runs lvl_linear_tn with LVL_EPI_BIAS_GELU_DERIV, its backward LVL_EPI_MUL_AUX_COLSUM, the deferred MLP's
    fc2 the residual epilogue; no QuickGELU epilogue, no torch GELU."""
    from lavila_amd import _cabi as C
    from lavila_amd import ops
    fx = H.fixture()
    vis = H.build_vision(fx['config'])
    vis.load_state_dict({k[len('visual.'):]: v for k, v in H.weights().items() if k.startswith('visual.')}, strict=True)
    vis.to(DEV).train()
    epis, fused = [], []
    real_tn, real_res = ops.linear_tn_raw, ops.mlp_residual_layer_norm

    def tn(x, w, bias=None, epilogue=C.EPI_BIAS, aux_in=None, f32=False):
        epis.append(epilogue)
        return real_tn(x, w, bias, epilogue, aux_in=aux_in, f32=f32)

    def res(*a, **k):
        out = real_res(*a, **k)
        fused.append((k.get('act'), out is not None))
        return out

    def boom(*a, **k):
        raise AssertionError('torch GELU called in a GELU tower\'s training step')
    monkeypatch.setattr(ops, 'linear_tn_raw', tn)
    monkeypatch.setattr(ops, 'mlp_residual_layer_norm', res)
    monkeypatch.setattr(torch.nn.GELU, 'forward', boom)
    monkeypatch.setattr(Mlp_module(), 'hidden', boom)
    video = H.inputs()[0].to(DEV)
    with ops_guard(gemm=False), torch.autocast('cuda', dtype=BF):
        feat = vis(video)
        feat.float().square().sum().backward()
    torch.cuda.synchronize()
    assert fused == [(ops.ACT_GELU, True)]
    assert epis.count(C.EPI_BIAS_GELU_DERIV) == 2 and epis.count(C.EPI_MUL_AUX_COLSUM) == 2
    assert epis.count(C.EPI_BIAS_RESIDUAL) >= 2            # block 0's space projection and its deferred MLP's fc2
    assert not {C.EPI_BIAS_QUICKGELU, C.EPI_BIAS_QUICKGELU_DERIV, C.EPI_QUICKGELU_BWD, C.EPI_BIAS_GELU, C.EPI_GELU_BWD} & set(epis)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in vis.parameters())
    # selective recompute keeps u instead: epilogues 6 and 7 for the deferred MLP
    epis.clear()
    vis.zero_grad(set_to_none=True)
    with ops_guard(gemm=False), torch.autocast('cuda', dtype=BF):
        vis(video, use_checkpoint='selective').float().square().sum().backward()
    torch.cuda.synchronize()
    assert epis.count(C.EPI_BIAS_GELU) == 1 and epis.count(C.EPI_GELU_BWD) == 1, epis


def Mlp_module():
    from lavila_amd.timesformer import Mlp
    return Mlp
