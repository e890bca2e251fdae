"""GPU (-m gpu): the max-margin ranking losses of the retrieval fine-tune on their kernels (csrc/margin_loss.hip:
lvl_margin_loss_prepare / _fwd / _bwd) against the float64 restatements of tests/rank_loss_reference.py, which
tests/test_margin_loss_cpu.py pins to the reference's own outputs.

Fence terms. A hinge term relu(z) changes its gradient at z = 0, so a kernel whose z is within its arithmetic error of
float64's may legitimately decide a term with |z64| < delta either way. delta is derived per mode in `delta_of`; the
comparisons below excuse exactly those terms (the CPU suite bounds their share at 1e-3 for these very problems), and the
exact-structure test has none, so there nothing is excused."""
import pytest
import torch

from conftest import load_golden
import rank_loss_reference as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = [torch.float32, torch.bfloat16]


def delta_of(dtype, E):
    """Bound on |z_device - z_float64| of one hinge argument z = m_i - d_i + x (inputs identical), unit rows.
    float32 rows: a product of two operands carried as bf16 hi + lo loses hi*lo rounding + the lo*lo term, 3 * 2^-17
    of |a_k b_k| at most; sum_k |a_k b_k| <= |a| |b| (Cauchy-Schwarz), so 3 * 2^-17 on a cosine. bf16 rows: the products
    are exact in float32, the float32 accumulation over E terms loses at most E * 2^-24 of sum_k |a_k b_k| <= 1.
    Both modes: d_i is a float32 FMA chain of E/64 terms per lane + a 6-level tree, the two norms and the two scalings
    are one rounding each: (E/64 + 32) * 2^-24 covers them and the final c + x."""
    common = (E / 64 + 32) * 2.0 ** -24
    d = 3 * 2.0 ** -17 + common if dtype == torch.float32 else E * 2.0 ** -24 + common
    assert d <= 1e-4          # the share of terms this close to zero is what the CPU suite caps
    return d


def run_kernels(img, txt, w, margin, fix_norm, B, row0, dtype, coef=None):
    """The three kernels through the C ABI wrappers on rows rounded to `dtype`; everything back on the CPU."""
    from lavila_amd import ops
    G = img.shape[0]
    N = 2 * G * (G - 1) if fix_norm else 2 * G * G
    i, t = img.to(dtype).to(DEV).contiguous(), txt.to(dtype).to(DEV).contiguous()
    wd = None if w is None else w.float().to(DEV).contiguous()
    prep = ops.margin_loss_prepare_raw(i, t, wd, margin)
    hinge, count = ops.margin_loss_fwd_raw(i, t, prep, B, row0, not fix_norm)
    up = torch.ones(1, device=DEV)
    dimg, dtxt = ops.margin_loss_bwd_raw(i, t, prep, up, (1.0 / N) if coef is None else coef, B, row0)
    torch.cuda.synchronize()
    return prep.cpu(), hinge.cpu(), count.cpu(), dimg.cpu(), dtxt.cpu()


def float64_slab(img, txt, w, margin, fix_norm, B, row0, dtype):
    """The same problem in float64 ON THE ROUNDED INPUTS (the bf16 recipe is applied before the float64 evaluation)."""
    G = img.shape[0]
    N = 2 * G * (G - 1) if fix_norm else 2 * G * G
    i, t = img.to(dtype).double(), txt.to(dtype).double()
    wd = None if w is None else w.float().double()
    prep = R.slab_prepare(i, t, wd, margin)
    hinge, count = R.slab_forward(i, t, prep, B, row0, not fix_norm)
    dimg, dtxt = R.slab_backward(i, t, prep, torch.ones(1, dtype=torch.float64), 1.0 / N, B, row0)
    return i, t, wd, N, hinge, count, dimg, dtxt


def compare_with_float64(img, txt, w, margin, fix_norm, B, row0, dtype, tag, expect_no_fence=False):
    G, E = img.shape
    delta = delta_of(dtype, E)
    _, hinge, count, dimg, dtxt = run_kernels(img, txt, w, margin, fix_norm, B, row0, dtype)
    i64, t64, w64, N, hinge64, count64, dimg64, dtxt64 = float64_slab(img, txt, w, margin, fix_norm, B, row0, dtype)
    f_t, f_v = R.fence_masks(i64, t64, margin, w64, delta)
    own = slice(row0, row0 + B)
    fence_rows = torch.stack([f_t[own].sum(1), f_v[own].sum(1)])          # own-threshold fence terms per (direction, row)
    F = R.fence_per_index(f_t, f_v)[own].double()
    if expect_no_fence:
        assert int(f_t.sum() + f_v.sum()) == 0
    # active counts: differ from float64's by at most the row's own fence terms
    dcount = (count.long() - count64.long()).abs()
    # hinge sums: every active term within delta, a fence term decided the other way moves the sum by < delta, and the
    # float32 summation of <= G terms (G/64 per lane, then two fixed merges) loses (G/64 + 16) * 2^-24 of the sum
    hinge_tol = delta * (count64 + fence_rows).double() + (G / 64 + 16) * 2.0 ** -24 * hinge64.abs() + 1e-12
    dh = (hinge.double() - hinge64).abs()
    # the loss of the slab: at most 2 * delta per term on average (delta from the term, delta from a flipped fence term)
    terms = 2 * B * (G - 1 if fix_norm else G)
    loss, loss64 = hinge.double().sum().item() / N, hinge64.sum().item() / N
    loss_tol = 2 * delta * terms / N + (G / 64 + 16) * 2.0 ** -24 * abs(loss64)
    # gradients, row by row. Base: 2e-6 of the tensor's max (float32 rounding of sums of <= 2G unit rows). Fence terms:
    # deciding one hinge term the other way changes d(sum)/d(unit row i) by one unit vector through s_ij and, when it is
    # one of row i's own terms, by a second one through cnt_i: at most 2 unit vectors of weight coef = 1/N. The
    # normalisation backward is a projection (norm <= 1) divided by |u_i|. So each of the F_i fence terms that involve
    # index i moves any element of row i's gradient by at most 2 / (N |u_i|).
    worst = {}
    for name, got, want, raw in (('dimg', dimg, dimg64, i64), ('dtxt', dtxt, dtxt64, t64)):
        norm = raw[own].norm(dim=1).clamp_min(R.EPS)
        tol = 2e-6 * want.abs().max() + 2 * F / (N * norm)
        err = (got.double() - want).abs().max(dim=1).values
        worst[name] = (err / tol).max().item()
    print(f'{tag}: delta {delta:.2e} fence terms {int(f_t.sum() + f_v.sum())} |d count| max {int(dcount.max())} '
          f'|d hinge|/tol {float((dh / hinge_tol).max()):.3f} |d loss| {abs(loss - loss64):.2e} (tol {loss_tol:.2e}) '
          f'gradient err/tol dimg {worst["dimg"]:.3f} dtxt {worst["dtxt"]:.3f} '
          f'active share {float(count64.sum()) / terms:.3f}')
    assert (dcount <= fence_rows).all(), (tag, int((dcount - fence_rows).max()))
    assert (dh <= hinge_tol).all(), (tag, float((dh / hinge_tol).max()))
    assert abs(loss - loss64) <= loss_tol, (tag, loss, loss64, loss_tol)
    assert worst['dimg'] <= 1 and worst['dtxt'] <= 1, (tag, worst)
    assert dimg64.abs().max() > 0 and dtxt64.abs().max() > 0
    return dcount, count, count64


# ---- 1. kernels through the C ABI against float64 -----------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('k', range(len(R.GPU_PROBLEMS)))
def test_kernels_match_float64(k, dtype):
    B, G, E, row0 = R.GPU_PROBLEMS[k]
    img, txt, w = R.make_inputs(G, E, R.GPU_SEED0 + k)
    for name, margin in R.CLASSES:
        for fix_norm in (True, False):
            compare_with_float64(img, txt, w if name.startswith('Adaptive') else None, margin, fix_norm, B, row0, dtype,
                                 f'{name} fix_norm={fix_norm} B={B} G={G} E={E} row0={row0} {dtype}')


# ---- 2. exact structure ---------------------------------------------------------------------------------------------
def _sign_rows(G, E, seed):
    """Rows from {+-1}^E: norms sqrt(E) (E = 64, 256: exact, as are their reciprocals), cosines k/E exact. Image row i
    is text row i with 30-50 % of its signs flipped: d_i in [0, 0.4], a mixed active set."""
    g = torch.Generator().manual_seed(seed)
    txt = torch.randint(0, 2, (G, E), generator=g).double() * 2 - 1
    frac = 0.3 + 0.2 * torch.rand(G, 1, generator=g, dtype=torch.float64)
    flip = torch.rand(G, E, generator=g, dtype=torch.float64) < frac
    img = torch.where(flip, -txt, txt)
    w = torch.tensor([0.25, 0.5, 1.0], dtype=torch.float64)[torch.randint(0, 3, (G,), generator=g)]
    return img, txt, w


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('B,G,E,row0', [(32, 96, 64, 32), (40, 168, 256, 64)])
def test_exact_structure_has_no_fence(B, G, E, row0, dtype):
    """Every hinge argument is (0.2 E or 0.4 w E + an integer) / E with 0.2 E and 0.4 w E (w in {1/4, 1/2, 1}) off the
    integer lattice by >= 0.2: |z| >= 0.2 / E >> delta, the fence set is empty, so the active counts EQUAL float64's and
    the gradients match to float32 rounding with no allowance."""
    img, txt, w = _sign_rows(G, E, 7 + E)
    for name, margin in R.CLASSES:
        for fix_norm in (True, False):
            dcount, count, count64 = compare_with_float64(
                img, txt, w if name.startswith('Adaptive') else None, margin, fix_norm, B, row0, dtype,
                f'exact {name} fix_norm={fix_norm} E={E} {dtype}', expect_no_fence=True)
            assert torch.equal(count.long(), count64.long())
            share = float(count64.sum()) / (2 * B * (G - 1))
            assert 0.05 < share < 0.95, share


# ---- 3. reproducibility ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_bit_reproducible_and_independent_of_the_slab_split(dtype):
    G, E = 200, 256
    img, txt, w = R.make_inputs(G, E, 321)
    first = run_kernels(img, txt, w, 0.4, True, G, 0, dtype)
    for _ in range(9):
        again = run_kernels(img, txt, w, 0.4, True, G, 0, dtype)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
    for W in (2, 4):                                   # B = 100, 50: rows sit in other tile slots than in the one-slab run
        B = G // W
        parts = [run_kernels(img, txt, w, 0.4, True, B, r * B, dtype, coef=1.0 / (2 * G * (G - 1))) for r in range(W)]
        assert torch.equal(torch.cat([p[1] for p in parts], 1), first[1])          # hinge [2,B]
        assert torch.equal(torch.cat([p[2] for p in parts], 1), first[2])          # count [2,B]
        assert torch.equal(torch.cat([p[3] for p in parts]), first[3])             # dimg
        assert torch.equal(torch.cat([p[4] for p in parts]), first[4])             # dtxt


# ---- 4. the reference's own numbers on the device ---------------------------------------------------------------------
@pytest.mark.parametrize('name', [n for n, _ in R.CLASSES])
@pytest.mark.parametrize('fix_norm', [True, False])
def test_classes_match_reference_fixture(name, fix_norm):
    """tests/golden/max_margin_loss.pt, single process, through the public classes. The fixture's smallest |hinge
    argument| (>= 1e-4) exceeds delta: no term is on the fence, the active counts are float64's."""
    from lavila.models import loss
    fx = load_golden('max_margin_loss.pt')
    want = fx['single'][(name, fix_norm)]
    G, E, margin = fx['single_G'], fx['E'], fx['margins'][name]
    assert fx['gap'] > delta_of(torch.float32, E)
    img, txt, w = (t.float() for t in R.make_inputs(G, E, fx['seed']))
    li, lt = img.to(DEV).requires_grad_(True), txt.to(DEV).requires_grad_(True)
    crit = getattr(loss, name)(margin=margin, fix_norm=fix_norm).cuda()
    out = crit({'image_embed': li, 'text_embed': lt}, w.to(DEV))
    assert list(out) == fx['output_keys']
    out['loss'].backward()
    wd = w if name.startswith('Adaptive') else None
    _, count64 = R.slab_forward(img, txt, R.slab_prepare(img, txt, wd, margin), G, 0, False)
    assert torch.equal(run_kernels(img, txt, wd, margin, fix_norm, G, 0, torch.float32)[2], count64)
    assert abs(out['loss'].item() - want['loss']) <= 2 * delta_of(torch.float32, E)
    for got, ref in ((li.grad, want['dimg']), (lt.grad, want['dtxt'])):
        assert got.dtype == torch.float32
        assert (got.cpu() - ref).abs().max() <= 1e-3 * ref.abs().max()


# ---- 5. edge cases ----------------------------------------------------------------------------------------------------
def test_rows_under_the_norm_clamp_against_float64():
    """A zero image row and a tiny NON-zero text row (norm ~ 8e-10): both sit under the 1e-8 norm clamp (unit row =
    row / 1e-8, gradient g / 1e-8 without the projection; for the tiny row the projection would differ, so the clamp
    branch itself is under test). The clamped row is compared on its own scale, the others
    on theirs: its gradient is 1e8 times larger."""
    B, G, E, row0 = 24, 48, 64, 8
    img, txt, w = R.make_inputs(G, E, 55)
    img[10] = 0
    txt[13] = 1e-10 * torch.randn(E, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    assert 0 < txt[13].float().norm() < 1e-8
    for name, margin in R.CLASSES:
        wd = w if name.startswith('Adaptive') else None
        delta = delta_of(torch.float32, E)
        _, hinge, count, dimg, dtxt = run_kernels(img, txt, wd, margin, True, B, row0, torch.float32)
        i64, t64, w64, N, hinge64, count64, dimg64, dtxt64 = float64_slab(img, txt, wd, margin, True, B, row0, torch.float32)
        f_t, f_v = R.fence_masks(i64, t64, margin, w64, delta)
        assert int(f_t.sum() + f_v.sum()) == 0            # seed chosen on the float64 side alone
        assert torch.equal(count.long(), count64.long())
        assert torch.isfinite(dimg).all() and torch.isfinite(dtxt).all()
        assert dimg64[10 - row0].abs().max() > 1e3 * dimg64[0].abs().max()          # the clamped rows really are huge
        assert dtxt64[13 - row0].abs().max() > 1e3 * dtxt64[0].abs().max()
        for got, want, zero in ((dimg, dimg64, 10 - row0), (dtxt, dtxt64, 13 - row0)):
            normal = torch.ones(B, dtype=torch.bool)
            normal[zero] = False
            scale = torch.where(normal, want[normal].abs().max(), want[zero].abs().max())[:, None]
            err = (got.double() - want).abs() / scale
            assert (err <= 2e-6).all(), float(err.max())
        assert ((hinge.double() - hinge64).abs() <= delta * count64 + 1e-6).all()


def test_no_grad_path_runs_no_backward_kernel(monkeypatch):
    from lavila.models import loss
    from lavila_amd import ops
    calls = {'prepare': 0, 'fwd': 0, 'bwd': 0}
    for key in calls:
        real = getattr(ops, f'margin_loss_{key}_raw')

        def counted(*a, _real=real, _key=key, **k):
            calls[_key] += 1
            return _real(*a, **k)
        monkeypatch.setattr(ops, f'margin_loss_{key}_raw', counted)
    img, txt, w = (t.float().to(DEV) for t in R.make_inputs(64, 256, 9))
    crit = loss.AdaptiveMaxMarginRankingLoss().cuda()
    with torch.no_grad():                                   # validate_mir
        quiet = crit({'image_embed': img, 'text_embed': txt}, w)['loss']
    assert calls == {'prepare': 1, 'fwd': 1, 'bwd': 0} and not quiet.requires_grad
    li, lt = img.clone().requires_grad_(True), txt.clone().requires_grad_(True)
    out = crit({'image_embed': li, 'text_embed': lt}, w)
    assert torch.equal(out['loss'].detach(), quiet)
    out['loss'].backward()
    assert calls == {'prepare': 2, 'fwd': 2, 'bwd': 1}


def test_other_dtypes_compute_in_float32_and_return_input_dtypes():
    from lavila.models import loss
    img, txt, w = (t.float().to(DEV) for t in R.make_inputs(64, 256, 9))
    crit = loss.AdaptiveMaxMarginRankingLoss().cuda()
    with torch.no_grad():
        quiet = crit({'image_embed': img, 'text_embed': txt}, w)['loss']
    lh, lb = img.half().requires_grad_(True), txt.bfloat16().requires_grad_(True)
    mixed = crit({'image_embed': lh, 'text_embed': lb}, w)
    mixed['loss'].backward()
    assert lh.grad.dtype == torch.float16 and lb.grad.dtype == torch.bfloat16
    assert abs(mixed['loss'].item() - quiet.item()) < 1e-2


def test_unsupported_width_is_an_error_that_names_the_supported_ones():
    from lavila.models import loss
    from lavila_amd._cabi import HipExtensionError
    img, txt, w = (t.float().to(DEV) for t in R.make_inputs(64, 256, 9))
    crit = loss.AdaptiveMaxMarginRankingLoss().cuda()
    with pytest.raises(HipExtensionError, match='64, 128, 256 and 512'):
        crit({'image_embed': img[:, :96].contiguous(), 'text_embed': txt[:, :96].contiguous()}, w)


def test_empty_slab_is_not_an_error_at_the_c_abi():
    from lavila_amd import ops
    img, txt, _ = (t.float().to(DEV) for t in R.make_inputs(64, 256, 9))
    prep = ops.margin_loss_prepare_raw(img, txt, None, 0.2)
    hinge, count = ops.margin_loss_fwd_raw(img, txt, prep, 0, 0, False)
    assert hinge.shape == (2, 0) and ops.margin_loss_bwd_raw(img, txt, prep, torch.ones(1, device=DEV), 1.0, 0, 0)[0].shape == (0, 256)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_graph_capture_replays_eager_bit_for_bit(dtype):
    """The three entry points allocate nothing and never synchronise: forward + backward of the adaptive loss captured in
    a hipGraph, replayed on new data, equal eager execution on that data bit for bit."""
    from lavila.models import loss
    G, E = 96, 256
    img, txt, w = R.make_inputs(G, E, 1)
    i_static = img.to(dtype).to(DEV).requires_grad_(True)
    t_static = txt.to(dtype).to(DEV).requires_grad_(True)
    w_static = w.float().to(DEV)
    crit = loss.AdaptiveMaxMarginRankingLoss(margin=0.4, fix_norm=True).cuda()

    def step():
        i_static.grad = None
        t_static.grad = None
        out = crit({'image_embed': i_static, 'text_embed': t_static}, w_static)['loss']
        out.backward()
        return out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_static = step()
    gi_static, gt_static = i_static.grad, t_static.grad
    img2, txt2, w2 = R.make_inputs(G, E, 2)
    with torch.no_grad():
        i_static.copy_(img2.to(dtype))
        t_static.copy_(txt2.to(dtype))
        w_static.copy_(w2.float())
    graph.replay()
    torch.cuda.synchronize()
    got = (loss_static.clone(), gi_static.clone(), gt_static.clone())
    eager = step()
    torch.cuda.synchronize()
    assert torch.equal(got[0], eager) and torch.equal(got[1], i_static.grad) and torch.equal(got[2], t_static.grad)
    assert got[1].dtype == dtype and got[1].abs().max() > 0
    want = R.dense_loss(img2.to(dtype).double(), txt2.to(dtype).double(), 0.4, w2.float().double(), True)
    assert abs(got[0].item() - want.item()) <= 2 * delta_of(dtype, E)


# ---- 6. a fine-tune step of a tiny dual encoder ---------------------------------------------------------------------
def test_finetune_step_of_tiny_clip_vs_oracle():
    """model(video, tokens, norm_embed=True) -> MaxMarginRankingLoss -> backward against oracle.clip_forward + the dense
    restatement's autograd on the CPU, at smoke()'s bars (1e-3 on the loss and on one parameter gradient). Then the same
    step under bf16 autocast: every block rounds ~10 intermediate tensors to bf16 (unit roundoff 2^-8), so the unit
    embeddings carry a relative error of about 2^-8 * sqrt(10 * depth) each; a cosine then moves by at most e_img + e_txt
    and a hinge argument m - d_i + x by twice that. The loss is a mean of 1-Lipschitz functions of those arguments:
    |loss_bf16 - loss_f32| <= 2 * (e_img + e_txt)."""
    from helpers import build_model
    from oracle import oracle as O
    from lavila.models.loss import MaxMarginRankingLoss
    c = dict(img=32, patch=16, frames=2, dim=128, depth=2, heads=2, t_width=128, t_heads=2, t_layers=2, vocab=512,
             embed=64, batch=8, gated=False)
    model = build_model(c)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    w = O.procedural_weights(shapes, seed=3)
    model.load_state_dict(w)
    model.cuda().train()
    video, tokens = O.synthetic_batch(c['batch'], c['frames'], c['img'], seed=5)
    tokens = tokens.clone()
    tokens[:, 1:31] = tokens[:, 1:31] % 510 + 1
    tokens[:, 0], tokens[:, 31] = 510, 511
    crit = MaxMarginRankingLoss(margin=0.2, fix_norm=True).cuda()
    out = model(video.cuda(), tokens.cuda(), norm_embed=True)
    ld = crit(out)
    ld['loss'].backward()
    torch.cuda.synchronize()
    wo = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in w.items()}
    oo = O.clip_forward(video, tokens, wo, c['heads'], c['t_heads'], norm_embed=True)
    lo = R.dense_loss(oo['image_embed'], oo['text_embed'], 0.2, None, True)
    lo.backward()
    # the oracle's own active set must not hinge on a near-zero argument (a property of the CPU side alone)
    z_t, z_v = R.hinge_arguments(oo['image_embed'].detach(), oo['text_embed'].detach(), 0.2)
    gap = min(z[~z.isnan()].abs().min().item() for z in (z_t, z_v))
    gk = 'visual.blocks.0.timeattn.qkv.weight'
    err_l = abs(ld['loss'].item() - lo.item())
    err_g = (dict(model.named_parameters())[gk].grad.cpu() - wo[gk].grad).abs().max().item()
    print(f'fine-tune step: loss {ld["loss"].item():.6f} oracle {lo.item():.6f} |d loss| {err_l:.2e} |d grad| {err_g:.2e} '
          f'(max |grad| {wo[gk].grad.abs().max().item():.2e}) smallest |hinge argument| {gap:.2e}')
    assert gap > 1e-3, gap
    assert wo[gk].grad.abs().max() > 0
    assert err_l < 1e-3 and err_g < 1e-3
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out16 = model(video.cuda(), tokens.cuda(), norm_embed=True)
        l16 = crit(out16)['loss']
    l16.backward()
    torch.cuda.synchronize()
    # At ~0.07 on a loss of ~0.2 this bound only catches a grossly wrong bf16 path: the step is a finiteness and smoke check
    # of the autocast plumbing; the bf16 arithmetic itself is checked at kernel level above.
    e = 2.0 ** -8 * (10 * c['depth']) ** 0.5 + 2.0 ** -8 * (10 * c['t_layers']) ** 0.5
    print(f'bf16 autocast: loss {l16.item():.6f} |d loss| {abs(l16.item() - lo.item()):.2e} (bound {2 * e:.2e})')
    assert torch.isfinite(l16) and abs(l16.item() - lo.item()) <= 2 * e
