"""GPU (-m gpu): the narrator's criterion on its kernels (csrc/caption_loss.hip: lvl_token_xent_fwd / _reduce / _bwd)
against the float64 restatement of tests/caption_loss_reference.py ON THE SAME ROUNDED INPUTS, which
tests/test_caption_loss_cpu.py pins to the reference's own outputs. Integer outputs (pred, correct, counted) and the exact
zeros must be EQUAL; only lse / nll / gradient values get a tolerance, derived in `bounds` from the kernels' own
summation order and exponential and printed by every test."""
import math
from types import SimpleNamespace

import pytest
import torch

from conftest import load_golden
import caption_loss_reference as R
from caption_loss_reference import EPS, LN2, LOG2E, NAN, bounds, check_rows, nan_like, run_raw      # noqa: F401

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = [torch.float32, torch.bfloat16]
IDS = ['f32', 'bf16']
def test_derived_bound_at_gpt2_vocabulary_is_under_1e_4():
    for dt in DTYPES:
        b = bounds(dt, 50257, 16.0)
        print(f'{dt}: lse {b[0]:.3e} nll {b[1]:.3e} rel_p {b[2]:.3e} rel_out {b[3]:.3e}')
        assert b[0] < 1e-4 and b[1] < 1e-4


def random_rows(rows, V, seed, scale=3.0, X=16.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(rows, V, generator=g)).clamp_(-X, X)


def random_labels(rows, V, pad, seed, pad_every=3):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, V, (rows,), generator=g)
    lab[::pad_every] = pad
    return lab


def strided_view(x, dtype, stride, offset, filler=(NAN, float('inf'))):
    """x [rows,V] placed at `offset` elements past a 16-byte aligned address with row stride `stride`; every element that
    is not a logit is NaN or +inf."""
    rows, V = x.shape
    flat = torch.empty(rows * stride + 16, dtype=dtype, device=DEV)
    assert flat.data_ptr() % 16 == 0
    flat[0::2] = filler[0]
    flat[1::2] = filler[1]
    view = flat[offset:offset + rows * stride].view(rows, stride)[:, :V]
    view.copy_(x.to(dtype))
    assert view.data_ptr() == flat.data_ptr() + offset * flat.element_size() and view.stride() == (stride, 1)
    return view


# ---- 1. kernels through the raw wrappers against float64 -----------------------------------------------------------
GPT2_V = 50257


@pytest.fixture(scope='module')
def gpt2_rows():
    x = random_rows(6, GPT2_V, 1, scale=4.0)
    lab = random_labels(6, GPT2_V, 0, 2, pad_every=4)
    x[1].clamp_(max=12.0)
    x[1, 123] = 15.5                                        # a correct row whatever the rounding (15.5 is a bf16 number)
    lab[1] = 123
    return x, lab


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('stride,offset', [(GPT2_V, 0), (GPT2_V + 7, 0), (GPT2_V + 7, 1), (GPT2_V + 7, 3)],
                         ids=['stride50257', 'padded_view', 'padded_view_off1', 'padded_view_off3'])
def test_gpt2_vocabulary_rows(gpt2_rows, stride, offset, dtype):
    """B=2, T=3 at V=50257. Row stride 50257: odd-aligned rows. Row stride 50264 through a [:, :50257] view of a buffer
    whose other columns are NaN / +inf (they are never read), the base 0, 1 and 3 elements past an aligned address."""
    x, lab = gpt2_rows
    view = x.to(dtype).to(DEV) if stride == GPT2_V else strided_view(x, dtype, stride, offset)
    out = check_rows(view, lab.to(DEV), 0, f'V=50257 stride={stride} off={offset} {dtype}', again=(offset == 0))
    assert int(out[3].sum()) >= 1 and int(out[4].sum()) == 4


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_vocabulary_sizes_around_every_boundary(dtype):
    """Below one 16-byte vector, one element either side of a vector (4 / 8), of one workgroup sweep (256 vectors: 1024 /
    2048) and of the four-sweep unrolled step (4096 / 8192). Row stride = V: the rows walk through every alignment."""
    for V in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193):
        x = random_rows(9, V, 100 + V)
        lab = random_labels(9, V, 0, 200 + V)
        check_rows(x.to(dtype).to(DEV), lab.to(DEV), 0, f'V={V} {dtype}')
        check_rows(strided_view(x, dtype, V + 3, 5), lab.to(DEV), 0, f'V={V} stride V+3 off 5 {dtype}')


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_rows_past_the_grid_cap(dtype):
    """The grid is capped at 2048 workgroups; 70 000 rows make every workgroup loop over 34 or 35 rows."""
    rows, V = 70000, 33
    x = random_rows(rows, V, 5)
    lab = random_labels(rows, V, 0, 6, pad_every=5)
    lse, nll, pred, correct, counted, _ = check_rows(x.to(dtype).to(DEV), lab.to(DEV), 0, f'rows=70000 V=33 {dtype}')
    # the reduce over many captions: B = 7000 > 256 lanes, T = 10
    from lavila_amd import ops
    B, T = 7000, 10
    res = ops.token_xent_reduce_raw(nll, correct, counted, B, T, out=nan_like((3,), torch.float32)).cpu().double()
    want = R.reduce3(nll.cpu(), correct.cpu(), counted.cpu(), B, T)
    n_add = T + math.ceil(B / 256) + 6 + 4 + 2                 # caption sum, lane chain, wave merge, waves, the division
    print(f'reduce B={B} T={T}: {res.tolist()} want {want.tolist()}')
    assert abs(res[0] - want[0]) <= n_add * EPS * want[0].abs()
    assert abs(res[1] - want[1]) <= 4 * EPS * want[1]
    # ppl_b = exp(s_b / n_b): s_b carries T roundings, the quotient one, expf 2 ulp at most; then the mean's additions
    per_caption = (nll.cpu().double().reshape(B, T).sum(1) / counted.cpu().reshape(B, T).sum(1)).abs().max().item()
    assert abs(res[2] - want[2]) <= ((T + 1) * EPS * per_caption + 4 * EPS + n_add * EPS) * want[2]


def test_float32_rows_with_huge_logits():
    """+-60000 in float32: nothing overflows; the bound scales with |x| (lse itself is a float32 of that size)."""
    V, rows = 3001, 6
    g = torch.Generator().manual_seed(3)
    x = torch.where(torch.rand(rows, V, generator=g) < 0.5, -60000.0, 60000.0)
    x[1] = random_rows(1, V, 4)[0]
    x[1, 17] = 60000.0
    x[2] = -60000.0
    x[2, V - 1] = 59990.0
    lab = torch.tensor([int(x[0].argmax()), 17, V - 1, 5, 0, 9])
    out = check_rows(x.to(DEV), lab.to(DEV), 0, 'huge f32', X=60000.0)
    assert torch.isfinite(out[0]).all() and torch.isfinite(out[5][:, :V]).all()


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_rows_with_minus_infinity(dtype):
    """Masked vocabulary entries: a leading run of -inf longer than a whole workgroup sweep (every lane's first vector,
    and more, is all -inf), a trailing run, scattered ones, and -inf everywhere but one entry."""
    V, rows = 5003, 6
    x = random_rows(rows, V, 8)
    x[0, :3000] = -math.inf
    x[1, 2000:] = -math.inf
    x[2, torch.rand(V, generator=torch.Generator().manual_seed(9)) < 0.5] = -math.inf
    x[3] = -math.inf
    x[3, 4001] = 2.5
    x[4, :9] = -math.inf
    lab = torch.tensor([3500, 7, 0, 4001, 100, 0])
    lab[2] = int(x[2].isfinite().nonzero()[5])
    out = check_rows(strided_view(x, dtype, V + 2, 1), lab.to(DEV), -100, f'-inf rows {dtype}')
    assert torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all() and not out[5][:, :V].isnan().any()
    assert out[2][3] == 4001 and abs(out[0][3].item() - 2.5) < 1e-5


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_exact_ties_keep_the_first_index(dtype):
    """The same top value at two indices on either side of a vector (float32 3|4, bf16 7|8), lane, wave (255|256,
    511|512) and workgroup-sweep (1023|1024, 2047|2048) boundary, at 0 and V-1, and three in one vector; rows are
    16-byte aligned (stride 5000) so the boundaries fall where named, then the same rows 3 elements off. The label on the
    first tied index is correct, on a later one it is not."""
    V = 5000
    pairs = [(0, V - 1), (3, 4), (7, 8), (255, 256), (511, 512), (1023, 1024), (2047, 2048), (4095, 4096), (16, 21)]
    x = random_rows(2 * len(pairs), V, 21).clamp_(max=4.0)
    lab = torch.empty(2 * len(pairs), dtype=torch.long)
    for k, (i, j) in enumerate(pairs):
        x[2 * k:2 * k + 2, [i, j]] = 9.0
        lab[2 * k], lab[2 * k + 1] = i, j
    x[-2:, 18] = 9.0
    for off in (0, 3):
        out = check_rows(strided_view(x, dtype, V, off), lab.to(DEV), -1, f'ties off={off} {dtype}')
        assert out[2].cpu().tolist() == [p[0] for p in pairs for _ in range(2)]
        assert out[3].cpu().tolist() == [1, 0] * len(pairs)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_pad_ids_and_out_of_range_labels(dtype):
    V, rows = 777, 8
    x = random_rows(rows, V, 31).to(dtype).to(DEV)
    for pad in (0, V - 1, -100):
        lab = torch.tensor([pad, 5, V - 1, 0, pad, 300, 1, pad])
        out = check_rows(x, lab.to(DEV), pad, f'pad={pad} {dtype}')
        assert out[4].cpu().tolist() == [int(v != pad) for v in lab.tolist()]
        assert torch.isfinite(out[1]).all()
    lab = torch.tensor([1, V, 2, -5, 0, 3, V + 100000, 4])                 # V and -5 (and beyond) are neither pad nor a class
    lse, nll, pred, correct, counted, grad = check_rows(x, lab.to(DEV), 0, f'out-of-range labels {dtype}')
    assert nll.isnan().cpu().tolist() == [False, True, False, True, False, False, True, False]
    assert grad[:, :V].isnan().all(dim=1).cpu().tolist() == [False, True, False, True, False, False, True, False]
    assert torch.isfinite(grad[[0, 2, 4, 5, 7]]).all() and torch.isfinite(lse).all()
    assert counted.cpu().tolist() == [1, 1, 1, 1, 0, 1, 1, 1] and correct[[1, 3, 6]].sum() == 0


def test_raw_wrappers_reject_what_the_kernels_cannot_take():
    from lavila_amd import ops
    from lavila_amd._cabi import HipExtensionError
    x = torch.randn(4, 16, device=DEV)
    lab = torch.zeros(4, dtype=torch.long, device=DEV)
    with pytest.raises(HipExtensionError):
        ops.token_xent_fwd_raw(x.t(), lab[:16].repeat(4), 0)                 # class stride 16
    with pytest.raises(HipExtensionError):
        ops.token_xent_fwd_raw(x.half(), lab, 0)
    with pytest.raises(HipExtensionError):
        ops.token_xent_fwd_raw(x, lab.int(), 0)
    with pytest.raises(HipExtensionError):
        ops.token_xent_fwd_raw(x.cpu(), lab.cpu(), 0)
    with pytest.raises(HipExtensionError):
        ops.token_xent_bwd_raw(x, lab, torch.zeros(4, device=DEV), torch.ones(1, device=DEV), 1.0, 0,
                               out=torch.empty(4, 17, device=DEV))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_graph_capture_replays_eager_bit_for_bit(dtype):
    """Forward, reduce and backward allocate nothing and never synchronise: captured as one chain in a hipGraph and
    replayed on new data, they equal eager execution on that data bit for bit."""
    from lavila_amd import ops
    B, T, V = 3, 5, 1001
    rows = B * T
    x_static = strided_view(random_rows(rows, V, 41), dtype, V, 1)
    lab_static = random_labels(rows, V, 0, 42).to(DEV)
    up = torch.tensor([0.5], device=DEV)
    fwd = tuple(nan_like((rows,), k) for k in (torch.float32, torch.float32, torch.int32, torch.int32, torch.int32))
    res, grad = nan_like((3,), torch.float32), nan_like((rows, R.padded(V)), dtype)

    def step(fwd, res, grad):
        lse, nll, pred, correct, counted = ops.token_xent_fwd_raw(x_static, lab_static, 0, out=fwd)
        ops.token_xent_reduce_raw(nll, correct, counted, B, T, out=res)
        ops.token_xent_bwd_raw(x_static, lab_static, lse, up, 1.0 / rows, 0, out=grad)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(fwd, res, grad)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(fwd, res, grad)
    x_static.copy_(random_rows(rows, V, 43).to(dtype))
    lab_static.copy_(random_labels(rows, V, 0, 44))
    for t in fwd + (res, grad):
        t.fill_(NAN if t.is_floating_point() else -1)
    graph.replay()
    torch.cuda.synchronize()
    fwd2 = tuple(nan_like((rows,), t.dtype) for t in fwd)
    res2, grad2 = nan_like((3,), torch.float32), nan_like((rows, R.padded(V)), dtype)
    step(fwd2, res2, grad2)
    torch.cuda.synchronize()
    for a, b in zip(fwd + (res, grad), fwd2 + (res2, grad2)):
        assert torch.equal(a, b)
    want = R.reduce3(*(t.cpu() for t in (fwd[1], fwd[3], fwd[4])), B, T)
    assert torch.isfinite(res).all() and abs(res[0].item() - want[0].item()) <= 1e-5 * want[0].item()
    assert grad.float().abs().max() > 0


# ---- 2. the module ---------------------------------------------------------------------------------------------------
def _crit(pad):
    from lavila.models.loss import CaptionLoss
    return CaptionLoss(tokenizer=SimpleNamespace(pad_token_id=pad))


def _rel(got, want):
    if math.isnan(want):
        return 0.0 if math.isnan(got) else math.inf
    return abs(got - want) / abs(want)


def _golden_input(case):
    logits = case['logits']
    if case['layout'] == 'permuted':
        logits = logits.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    return logits


@pytest.mark.parametrize('name', list(R.CASES))
def test_module_matches_reference_fixture_f32(name):
    """Every golden case in float32: loss, acc and ppl within 1e-3 relative of the reference's values (the project's
    parity bar); the gradient at the CPU suite's bars (rtol 1e-4, atol 1e-8: float32 reference against float64) plus the
    derived kernel bound."""
    fx = load_golden('caption_loss.pt')
    case = fx['cases'][name]
    cpu = _golden_input(case)
    B, V, T = cpu.shape
    leaf = torch.empty_strided(cpu.shape, cpu.stride(), device=DEV).copy_(cpu).requires_grad_(True)
    assert leaf.stride() == cpu.stride()
    out = _crit(case['pad'])({'text_tokens_logits': leaf, 'labels': case['labels'].to(DEV)})
    assert list(out) == fx['output_keys']
    for key, gkey in (('loss', 'loss'), ('caption_acc', 'acc'), ('ppl', 'ppl')):
        assert out[key].device.type == 'cuda' and out[key].dim() == 0 and out[key].dtype == torch.float32
        print(f'{name} {key}: {out[key].item():.6f} reference {case[gkey]:.6f}')
        assert _rel(out[key].item(), case[gkey]) <= 1e-3, key
    out['loss'].backward()
    assert leaf.grad.shape == leaf.shape and leaf.grad.dtype == torch.float32
    _, _, rel_p, rel_out = bounds(torch.float32, V, 16.0)
    assert cpu.abs().max() <= 16
    want = case['grad']
    p_over = want.abs() + 1.0 / (B * T)                                       # k p <= |g| + k
    tol = 1e-8 + 1e-4 * want.abs() + p_over * rel_p + want.abs() * rel_out
    err = (leaf.grad.cpu() - want).abs()
    print(f'{name} gradient err/tol {(err / tol).max().item():.3f}')
    assert (err <= tol).all()


@pytest.mark.parametrize('name', ['ragged_pad0', 'pad_is_7'])
def test_module_bf16_against_float64_of_the_rounded_inputs(name):
    fx = load_golden('caption_loss.pt')
    case = fx['cases'][name]
    cpu = _golden_input(case).bfloat16()
    B, V, T = cpu.shape
    leaf = torch.empty_strided(cpu.shape, cpu.stride(), dtype=torch.bfloat16, device=DEV).copy_(cpu).requires_grad_(True)
    out = _crit(case['pad'])({'text_tokens_logits': leaf, 'labels': case['labels'].to(DEV)})
    out['loss'].backward()
    want, gwant = R.loss_and_grad(cpu, case['labels'], case['pad'])
    _, nll_tol, rel_p, rel_out = bounds(torch.bfloat16, V, 16.0)
    n_add = T + 1 + 6 + 4
    # loss: every nll within nll_tol, the sum's roundings; ppl_b = exp(mean nll_b): relative exp(nll_tol) - 1 + roundings
    assert abs(out['loss'].item() - want[0].item()) <= nll_tol + n_add * EPS * want[0].item() + EPS * want[0].item()
    assert out['caption_acc'].item() == pytest.approx(want[1].item(), rel=4 * EPS)
    if math.isnan(want[2].item()):
        assert math.isnan(out['ppl'].item())
    else:
        worst_nll = 16 + math.log(V) + 16
        assert _rel(out['ppl'].item(), want[2].item()) <= math.expm1(nll_tol) + (T + 1) * EPS * worst_nll + (n_add + 5) * EPS
    assert leaf.grad.dtype == torch.bfloat16 and leaf.grad.shape == leaf.shape
    p64 = torch.exp(cpu.double() - torch.logsumexp(cpu.double(), dim=1, keepdim=True))
    tol = p64 / (B * T) * rel_p + gwant.abs() * rel_out + 2.0 ** -126
    err = (leaf.grad.cpu().double() - gwant).abs()
    print(f'{name} bf16: loss {out["loss"].item():.6f} float64 {want[0].item():.6f}; gradient err/tol {(err / tol).max().item():.3f}')
    assert (err <= tol).all()


def test_module_layouts_copies_and_dtypes(monkeypatch):
    """The permuted view and the [:, :V] view of a padded product reach the kernel in place (the pointer the forward
    wrapper receives is the caller's); a contiguous [B,V,T] is copied once into padded rows; float16 runs as float32 and
    gets a float16 gradient; no backward kernel runs under no_grad."""
    from lavila_amd import ops
    seen, calls = [], {'bwd': 0}
    real_fwd, real_bwd = ops.token_xent_fwd_raw, ops.token_xent_bwd_raw

    def fwd(logits, *a, **k):
        seen.append((logits.data_ptr(), logits.stride(0), logits.dtype))
        return real_fwd(logits, *a, **k)

    def bwd(*a, **k):
        calls['bwd'] += 1
        return real_bwd(*a, **k)

    monkeypatch.setattr(ops, 'token_xent_fwd_raw', fwd)
    monkeypatch.setattr(ops, 'token_xent_bwd_raw', bwd)
    logits, labels, pad = R.make_case('ragged_pad0')
    B, V, T = logits.shape
    crit = _crit(pad)
    base = logits.permute(0, 2, 1).contiguous().to(DEV)                      # [B,T,V]
    text = torch.cat([torch.full((B, 1), 9), labels], dim=1).to(DEV)
    with torch.no_grad():
        quiet = crit({'text_tokens_logits': base.permute(0, 2, 1), 'labels': text[:, 1:]})
    assert seen[-1] == (base.data_ptr(), V, torch.float32) and calls['bwd'] == 0 and not quiet['loss'].requires_grad
    wide = torch.full((B, T, R.padded(V)), NAN, device=DEV)
    wide[:, :, :V] = base
    out = crit({'text_tokens_logits': wide[:, :, :V].permute(0, 2, 1), 'labels': labels.to(DEV)})
    assert seen[-1] == (wide.data_ptr(), R.padded(V), torch.float32)
    assert torch.equal(out['caption_acc'], quiet['caption_acc']) and _rel(out['loss'].item(), quiet['loss'].item()) < 1e-6
    contiguous = base.permute(0, 2, 1).contiguous().requires_grad_(True)
    out = crit({'text_tokens_logits': contiguous, 'labels': labels.to(DEV)})
    assert seen[-1][0] != contiguous.data_ptr() and seen[-1][1:] == (R.padded(V), torch.float32)
    out['loss'].backward()
    assert calls['bwd'] == 1 and contiguous.grad.shape == contiguous.shape
    half = base.permute(0, 2, 1).half().requires_grad_(True)
    out = crit({'text_tokens_logits': half, 'labels': labels.to(DEV)})
    assert seen[-1][2] == torch.float32
    out['loss'].backward()
    assert half.grad.dtype == torch.float16 and half.grad.shape == half.shape
    want, _ = R.loss_and_grad(half.detach().cpu(), labels, pad)
    assert _rel(out['loss'].item(), want[0].item()) < 1e-5


# ---- 3. end to end: VCLM_HF.forward -> CaptionLoss --------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['freq1_gated', 'freq2_plain'])
def test_narrator_validation_numbers_match_reference(variant):
    """The narrator_decoder.pt model, run with VCLM_HF.forward under no_grad and then CaptionLoss, against the
    reference criterion on the reference's logits (tests/golden/caption_loss.pt).

    test_narrator_forward_matches_reference_f32 bounds every logit by d = 2e-3 + 1e-3 max|x|. lse moves by at most d and
    so does the label's logit: a nll moves by 2 d at most (+ the kernel's own nll_tol), the loss (a mean of nll over
    B*T with pads 0) by no more, and ppl_b = exp(mean of a caption's nll) by a factor exp(2 d + nll_tol) at most.
    The smallest top-2 gap of the reference's logits exceeds 2 d, so no argmax can flip: caption_acc is equal."""
    from test_gpu_narrator import _golden_model
    fx = load_golden('caption_loss.pt')['narrator'][variant]
    m, c, d, v, video, tok = _golden_model(variant)
    delta = 2e-3 + 1e-3 * fx['max_abs_logit']
    assert fx['gap'] > 2 * delta, (fx['gap'], delta)
    _, nll_tol, _, _ = bounds(torch.float32, d['vocab'], fx['max_abs_logit'] + delta)
    crit = _crit(tok.pad_token_id)
    assert crit.pad_id == fx['pad']
    with torch.no_grad():
        out = m(video, v['text'].to(DEV))
        for tag, labels in (('stored', out['labels']), ('hit', fx['labels_hit'].to(DEV))):
            res = crit({'text_tokens_logits': out['text_tokens_logits'], 'labels': labels})
            want = fx[tag]
            move = 2 * delta + nll_tol
            print(f'{variant} {tag}: loss {res["loss"].item():.5f} ({want["loss"]:.5f}) acc {res["caption_acc"].item():.4f} '
                  f'({want["acc"]:.4f}) ppl {res["ppl"].item():.3f} ({want["ppl"]:.3f}); allowed nll move {move:.4f}')
            assert abs(res['loss'].item() - want['loss']) <= move + 1e-6 * want['loss']
            assert _rel(res['ppl'].item(), want['ppl']) <= math.expm1(move) + 1e-6
            assert res['caption_acc'].item() == pytest.approx(want['acc'], rel=1e-6)
    assert fx['hit']['acc'] > 0
