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
