"""Float64 restatement of the narrator's criterion (CaptionLoss, loss.py:220-253) in the row form of
csrc/caption_loss.hip, shared by tests/test_caption_loss_cpu.py (which pins it to the reference's own outputs,
tests/golden/caption_loss.pt) and tests/test_gpu_caption_loss.py (which measures the kernels against it).

Rows: x [rows, V] (row r = caption r // T, position r % T), labels [rows] int64.
  lse_r = log sum_j exp(x[r,j]);  nll_r = lse_r - x[r,label_r], 0 for a pad label, NaN for any other label outside [0,V);
  pred_r = FIRST index of the row maximum;  correct_r = (pred_r == label_r) & counted_r;  counted_r = label_r != pad.
  loss = sum(nll) / (B T);  acc = 100 sum(correct) / (sum(counted) + 1e-8);  ppl = mean_b exp(sum_t nll / sum_t counted).
  gradient [rows, Vp], Vp = V rounded up to 8: coef * upstream * (exp(x - lse) - onehot(label)); pad rows 0, rows with an
  out-of-range label NaN, columns [V, Vp) 0.
"""
import math

import torch

# synthetic cases of the golden file: name -> (B, T, V, pad_id, layout, seed, counted labels per caption)
# layout 'permuted': a [B,T,V] tensor seen as [B,V,T] (what VCLM_HF.forward returns); 'contiguous': a contiguous [B,V,T]
CASES = {
    'ragged_pad0': (4, 6, 37, 0, 'permuted', 11, (6, 3, 0, 1)),          # caption 2 is all pad
    'pad_is_7': (3, 5, 41, 7, 'contiguous', 12, (5, 2, 4)),
    'no_pad': (2, 4, 33, 0, 'permuted', 13, (4, 4)),
    'contiguous_ragged': (3, 7, 19, 0, 'contiguous', 14, (7, 1, 4)),
}


def padded(V):
    return (V + 7) // 8 * 8


def make_case(name):
    """(logits [B,V,T] float32 in the case's layout, labels [B,T] int64, pad_id)."""
    B, T, V, pad, layout, seed, keep = CASES[name]
    g = torch.Generator().manual_seed(seed)
    rows = 3.0 * torch.randn(B, T, V, generator=g)
    labels = torch.randint(0, V - 1, (B, T), generator=g)
    labels = labels + (labels >= pad).long()                    # any class but the pad id
    top = rows.argmax(dim=2)                                    # every third position is predicted right
    labels[:, ::3] = torch.where(top != pad, top, labels)[:, ::3]
    for b, n in enumerate(keep):
        labels[b, n:] = pad
    logits = rows.permute(0, 2, 1)
    return (logits if layout == 'permuted' else logits.contiguous()), labels, pad


def rows_of(logits):
    """[B,V,T] -> [B*T, V] float64."""
    B, V, T = logits.shape
    return logits.detach().double().permute(0, 2, 1).reshape(B * T, V)


def rows_forward(x, labels, pad_id):
    """x [rows,V] (evaluated in float64), labels [rows] -> lse f64, nll f64, pred i32, correct i32, counted i32."""
    x = x.double()
    rows, V = x.shape
    labels = labels.reshape(-1).long()
    lse = torch.logsumexp(x, dim=1)
    top = x.max(dim=1, keepdim=True).values
    cols = torch.arange(V).expand(rows, V)
    pred = torch.where(x == top, cols, torch.full_like(cols, V)).min(dim=1).values
    counted = labels != pad_id
    valid = counted & (labels >= 0) & (labels < V)
    picked = x.gather(1, torch.where(valid, labels, torch.zeros_like(labels))[:, None])[:, 0]
    nll = torch.where(valid, lse - picked, torch.full_like(lse, float('nan')))
    nll = torch.where(counted, nll, torch.zeros_like(nll))
    correct = (pred == labels) & counted
    return lse, nll, pred.int(), correct.int(), counted.int()


def reduce3(nll, correct, counted, B, T):
    """[3] float64 = {loss, caption_acc, ppl}."""
    nll = nll.double().reshape(B, T)
    n = counted.reshape(B, T).sum(1).double()
    loss = nll.sum() / (B * T)
    acc = 100.0 * correct.sum().double() / (counted.sum().double() + 1e-8)
    ppl = torch.exp(nll.sum(1) / n).mean()
    return torch.stack([loss, acc, ppl])


def rows_backward(x, labels, lse, upstream, coef, pad_id):
    """[rows, Vp] float64."""
    x = x.double()
    rows, V = x.shape
    labels = labels.reshape(-1).long()
    k = coef * upstream.double().reshape(())
    counted = labels != pad_id
    valid = counted & (labels >= 0) & (labels < V)
    g = torch.exp(x - lse.double()[:, None])
    g[valid, labels[valid]] -= 1.0
    g = k * g
    g[~counted] = 0.0
    g[counted & ~valid] = float('nan')
    out = torch.zeros(rows, padded(V), dtype=torch.float64)
    out[:, :V] = g
    return out


def loss_and_grad(logits, labels, pad_id):
    """The whole criterion on [B,V,T] logits: ([3] float64, gradient [B,V,T] float64 of the loss)."""
    B, V, T = logits.shape
    x, lab = rows_of(logits), labels.reshape(-1)
    lse, nll, _, correct, counted = rows_forward(x, lab, pad_id)
    g = rows_backward(x, lab, lse, torch.ones(()), 1.0 / (B * T), pad_id)
    return reduce3(nll, correct, counted, B, T), g.view(B, T, -1)[:, :, :V].permute(0, 2, 1)


class Hooks:
    """The three kernel hooks of lavila_amd.loss.CaptionLoss on the CPU (float64 inside, the kernels' output dtypes)."""
    seen = None                                              # the `rows` view the last forward hook received

    def _token_forward(self, rows, labels, pad_id):
        type(self).seen = rows
        lse, nll, pred, correct, counted = rows_forward(rows, labels, pad_id)
        return lse.float(), nll.float(), pred, correct, counted

    def _token_reduce(self, nll, correct, counted, B, T):
        return reduce3(nll, correct, counted, B, T).float()

    def _token_backward(self, rows, labels, lse, upstream, coef, pad_id):
        return rows_backward(rows, labels, lse, upstream, coef, pad_id).to(rows.dtype)


# ---- the kernels against this module (GPU tests: test_gpu_caption_loss.py, test_gpu_large_operands.py) ----------------------
DEV = 'cuda'
EPS = 2.0 ** -24                      # unit roundoff of float32
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
NAN = float('nan')


def bounds(dtype, V, X):
    """Bounds for rows of V finite-or-minus-infinity logits with finite |x| <= X, inputs identical on both sides.

    Forward. A lane carries sum_j 2^(t_j), t_j = fma(x_j, log2e, -M) with an integer M, and raising M rescales by an
    exact power of two, so the only errors are
      * of a term: the float32 constant log2e (relative 2^-25: X log2e 2^-25 on the exponent), the one rounding of the
        fma (EPS |t|, |t| <= 2 X log2e + 1), v_exp_f32 (1 ulp = 2^-23 relative): relative ln2 * (exponent error) + 2^-23;
      * of the additions: W - 1 inside a 16-byte vector of W elements, one per vector step of the lane (ceil(V / W / 256)
        of them), 2 for the scalar head and tail, 6 levels of the wave merge, 4 waves: n_add roundings, n_add * EPS.
    lse = (M + log2(sum)) * ln2: v_log_f32 (1 ulp of a |log2 sum| <= 16), the addition, the constant ln2 (2^-25) and the
    product: 16 ln2 2^-23 + 3 EPS |lse|, |lse| <= X + ln V. nll adds the rounding of lse - x[label].
    Backward. p = 2^fma(x, log2e, c), c = -lse log2e: the term error again with |t| <= (L + X) log2e, the two roundings of
    c (1.5 EPS L log2e) and the forward's own error of lse; then (p - onehot) * k, two roundings, and ONE rounding to
    the output dtype (bf16 carries 8 significant bits: half an ulp is 2^-8 relative at most). Returned: (lse_tol, nll_tol, rel_p, rel_out)."""
    W = 4 if dtype == torch.float32 else 8
    L = X + math.log(V)
    n_add = (W - 1) + math.ceil(math.ceil(V / W) / 256) + 2 + 6 + 4
    term = LN2 * (X * LOG2E * 2.0 ** -25 + EPS * (2 * X * LOG2E + 1)) + 2.0 ** -23
    lse_tol = term + n_add * EPS + 16 * LN2 * 2.0 ** -23 + 3 * EPS * L
    nll_tol = lse_tol + EPS * (L + X)
    rel_p = LN2 * (X * LOG2E * 2.0 ** -25 + EPS * (L + X) * LOG2E + 1.5 * EPS * L * LOG2E) + 2.0 ** -23 + lse_tol
    rel_out = 2 * EPS + (0.0 if dtype == torch.float32 else 2.0 ** -8)
    return lse_tol, nll_tol, rel_p, rel_out


def nan_like(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device=DEV) if dtype.is_floating_point else \
        torch.full(shape, -12345, dtype=dtype, device=DEV)


def run_raw(view, labels, pad, up, coef):
    """The three kernels through the raw wrappers into NaN-prefilled out= buffers."""
    from lavila_amd import ops
    rows, V = view.shape
    outs = (nan_like((rows,), torch.float32), nan_like((rows,), torch.float32), nan_like((rows,), torch.int32),
            nan_like((rows,), torch.int32), nan_like((rows,), torch.int32))
    lse, nll, pred, correct, counted = ops.token_xent_fwd_raw(view, labels, pad, out=outs)
    grad = ops.token_xent_bwd_raw(view, labels, lse, up, coef, pad, out=nan_like((rows, padded(V)), view.dtype))
    torch.cuda.synchronize()
    return lse, nll, pred, correct, counted, grad


def check_rows(view, labels, pad, tag, X=16.0, coef=0.37, upstream=1.7, again=False):
    """view: [rows, V] device view (any row stride / base alignment), labels [rows] int64 on the device."""
    rows, V = view.shape
    dtype = view.dtype
    up = torch.tensor([upstream], device=DEV)
    lse, nll, pred, correct, counted, grad = run_raw(view, labels, pad, up, coef)
    x64, lab = view.cpu().double(), labels.cpu()
    lse64, nll64, pred64, correct64, counted64 = rows_forward(x64, lab, pad)
    g64 = rows_backward(x64, lab, lse64, up.cpu(), coef, pad)
    lse_tol, nll_tol, rel_p, rel_out = bounds(dtype, V, X)
    assert x64[x64.isfinite()].abs().max() <= X
    # integers: equal
    assert torch.equal(pred.cpu(), pred64), (tag, (pred.cpu() != pred64).nonzero()[:4])
    assert torch.equal(correct.cpu(), correct64) and torch.equal(counted.cpu(), counted64), tag
    # lse, nll
    d_lse = (lse.cpu().double() - lse64).abs().max().item()
    ok = ~nll64.isnan()
    assert torch.equal(nll.cpu().isnan(), ~ok), tag                                   # NaN exactly where the label is out of range
    d_nll = (nll.cpu().double() - nll64)[ok].abs().max().item() if ok.any() else 0.0
    assert (nll.cpu()[counted64 == 0] == 0).all() and not torch.signbit(nll.cpu()[counted64 == 0]).any(), tag
    # gradient: NaN rows, exact zeros, values
    g = grad.cpu()
    Vp = padded(V)
    assert tuple(g.shape) == (rows, Vp)
    bits = g.view(torch.int32 if dtype == torch.float32 else torch.int16)
    assert (bits[:, V:] == 0).all(), f'{tag}: pad columns are not bitwise zero'
    assert (bits[counted64 == 0] == 0).all(), f'{tag}: pad rows are not bitwise zero'
    bad = g64[:, :V].isnan().any(dim=1)
    assert torch.equal(g[:, :V].isnan().all(dim=1), bad) and torch.equal(g[:, :V].isnan().any(dim=1), bad), tag
    p64 = torch.exp(x64 - lse64[:, None])
    tol = abs(coef * upstream) * p64 * rel_p + g64[:, :V].abs() * rel_out + 2.0 ** -126
    err = (g[:, :V].double() - g64[:, :V]).abs()
    live = ~bad
    worst = (err[live] / tol[live]).max().item() if live.any() else 0.0
    print(f'{tag}: |d lse| {d_lse:.2e} (tol {lse_tol:.2e}) |d nll| {d_nll:.2e} (tol {nll_tol:.2e}) '
          f'gradient err/tol {worst:.3f} (rel_p {rel_p:.2e}) max |g| {g64[:, :V][live].abs().max().item():.2e}')
    assert d_lse <= lse_tol and d_nll <= nll_tol, tag
    assert worst <= 1.0, tag
    if again:
        second = run_raw(view, labels, pad, up, coef)
        for a, b in zip((lse, nll, pred, correct, counted), second[:5]):
            assert torch.equal(a, b), tag
        assert torch.equal(bits.to(DEV), second[5].view(bits.dtype)), tag              # bitwise: NaN rows compare equal too
    return lse, nll, pred, correct, counted, grad
