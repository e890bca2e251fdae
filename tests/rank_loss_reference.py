"""Max-margin ranking losses (lavila/models/loss.py:256-367), restated for the tests. Plain module, no test in it.

  dense_loss          the reference formulation (differentiable torch, any dtype; the tests use float64)
  hinge_arguments     the two [G,G] matrices of hinge arguments, float64: what decides the active set
  slab_prepare / slab_forward / slab_backward
                      the slab decomposition the kernels implement (lvl_margin_loss_*), float64 inside, written from
                      the closed-form gradient -- no autograd -- so that it checks the formula, and used as the CPU
                      stand-in for the kernel hooks of the loss classes on gloo
  make_inputs         the seeded input recipe of the tests (float64)
"""
import math

import torch

EPS = 1e-8


def make_inputs(G, E, seed):
    """Correlated pairs (cosines 0 .. 0.6), near-duplicate captions as in EK-100, un-normalised rows, weights in
    [0, 1): 40-46 % of the hinge terms are active."""
    g = torch.Generator().manual_seed(seed)
    f64 = dict(dtype=torch.float64, generator=g)
    txt = torch.randn(G, E, **f64)
    noise = torch.randn(G, E, **f64)
    rho = 0.6 * torch.rand(G, 1, **f64)
    img = rho * txt + torch.sqrt(1 - rho * rho) * noise
    k = G // 8
    if k:
        txt[G - k:] = txt[:k] + 0.3 * torch.randn(k, E, **f64)
    img = img * (0.5 + 2 * torch.rand(G, 1, **f64))
    txt = txt * 1.7
    w = torch.rand(G, **f64)
    return img, txt, w


def unit_rows(a):
    return a / a.norm(dim=1, keepdim=True).clamp_min(EPS)


def dense_loss(img, txt, margin, weight=None, fix_norm=True):
    """The reference's loss on the whole batch (loss.py:281-307 / 330-362), differentiable. The diagonal terms of
    fix_norm=False are relu(m_i - x_ii + x_ii) = relu(m_i): taken as such."""
    n = img.shape[0]
    x = unit_rows(txt) @ unit_rows(img).t()                    # x[i,j] = cos(txt_i, img_j)
    m = torch.full((n,), float(margin), dtype=x.dtype, device=x.device) if weight is None else margin * weight.to(x)
    c = (m - torch.diagonal(x))[:, None]
    off = ~torch.eye(n, dtype=torch.bool, device=x.device)
    total = (torch.relu(c + x) * off).sum() + (torch.relu(c + x.t()) * off).sum()
    if fix_norm:
        return total / (2 * n * (n - 1)) if n > 1 else total * float('nan')
    return (total + 2 * torch.relu(m).sum()) / (2 * n * n)


def hinge_arguments(img, txt, margin, weight=None):
    """z_txt[i,j] = c_i + x[i,j] (own text row i against image j), z_img[i,j] = c_i + x[j,i] (own image row i against
    text j), float64; the diagonals are set to NaN (handled analytically everywhere)."""
    img, txt = img.double(), txt.double()
    n = img.shape[0]
    x = unit_rows(txt) @ unit_rows(img).t()
    m = torch.full((n,), float(margin), dtype=torch.float64) if weight is None else margin * weight.double()
    c = (m - torch.diagonal(x))[:, None]
    z_txt, z_img = c + x, c + x.t()
    eye = torch.eye(n, dtype=torch.bool)
    return z_txt.masked_fill(eye, float('nan')), z_img.masked_fill(eye, float('nan'))


def slab_prepare(img_all, txt_all, weight_all, margin):
    """[7,G] float64 = {1/max(|img|,eps), 1/max(|txt|,eps), d, c, m, max(|img|,eps), max(|txt|,eps)} --
    lvl_margin_loss_prepare."""
    img, txt = img_all.double(), txt_all.double()
    den_img, den_txt = img.norm(dim=1).clamp_min(EPS), txt.norm(dim=1).clamp_min(EPS)
    inv_img, inv_txt = 1.0 / den_img, 1.0 / den_txt
    d = (img * txt).sum(1) * inv_txt * inv_img
    m = torch.full_like(d, float(margin)) if weight_all is None else margin * weight_all.double()
    return torch.stack([inv_img, inv_txt, d, m - d, m, den_img, den_txt])


def _slab_scores(img_all, txt_all, prep, B, row0):
    img, txt = img_all.double(), txt_all.double()
    vh, th = img * prep[0][:, None], txt * prep[1][:, None]
    G = img.shape[0]
    own = slice(row0, row0 + B)
    x_t = th[own] @ vh.t()                 # [B,G] own text rows against all images: x[i,j]
    x_v = vh[own] @ th.t()                 # [B,G] own image rows against all texts: x[j,i]
    off = torch.ones(B, G, dtype=torch.bool)
    off[torch.arange(B), torch.arange(row0, row0 + B)] = False
    return vh, th, x_t, x_v, off


def slab_forward(img_all, txt_all, prep, B, row0, with_diag):
    """hinge [2,B] float64, count [2,B] int32 -- lvl_margin_loss_fwd."""
    _, _, x_t, x_v, off = _slab_scores(img_all, txt_all, prep, B, row0)
    c = prep[3][row0:row0 + B, None]
    hinge, count = [], []
    for x in (x_t, x_v):
        z = c + x
        act = (z > 0) & off
        hinge.append((z * act).sum(1))
        count.append(act.sum(1))
    hinge = torch.stack(hinge)
    if with_diag:
        hinge = hinge + torch.relu(prep[4][row0:row0 + B])[None]
    return hinge, torch.stack(count).to(torch.int32)


def slab_backward(img_all, txt_all, prep, upstream, coef, B, row0):
    """coef * upstream * d(sum of all hinge terms)/d(raw local rows) from the closed form:
         g_t[i] = sum_{j!=i} ([c_i + x_ij > 0] + [c_j + x_ij > 0]) v^_j - cnt_i v^_i        (unit-row gradient)
         g_v[i] = sum_{j!=i} ([c_i + x_ji > 0] + [c_j + x_ji > 0]) t^_j - cnt_i t^_i
       then (g - (g.u^) u^) / |u| for rows above the norm clamp and g / eps below -- lvl_margin_loss_bwd."""
    vh, th, x_t, x_v, off = _slab_scores(img_all, txt_all, prep, B, row0)
    own = slice(row0, row0 + B)
    c_own, c_all = prep[3][own, None], prep[3][None, :]
    s_t = (((c_own + x_t > 0) & off).double() + ((c_all + x_t > 0) & off).double())
    s_v = (((c_own + x_v > 0) & off).double() + ((c_all + x_v > 0) & off).double())
    cnt = (((c_own + x_t > 0) & off).sum(1) + ((c_own + x_v > 0) & off).sum(1)).double()[:, None]
    g_t = s_t @ vh - cnt * vh[own]
    g_v = s_v @ th - cnt * th[own]
    out = []
    for g, uh, inv, den in ((g_v, vh[own], prep[0][own, None], prep[5][own, None]),
                            (g_t, th[own], prep[1][own, None], prep[6][own, None])):
        clamped = den <= EPS
        proj = g - (g * uh).sum(1, keepdim=True) * uh
        out.append(torch.where(clamped, g, proj) * inv)
    k = coef * upstream.double().reshape(())
    return (k * out[0]).contiguous(), (k * out[1]).contiguous()          # dimg, dtxt


def slab_loss_and_grads(img, txt, margin, weight, fix_norm, W=1):
    """The whole loss and the raw-row gradients from W slabs (what the W ranks compute), float64."""
    G = img.shape[0]
    B = G // W
    N = 2 * G * (G - 1) if fix_norm else 2 * G * G
    prep = slab_prepare(img, txt, weight, margin)
    one = torch.ones(1, dtype=torch.float64)
    total, dimg, dtxt = 0.0, [], []
    for r in range(W):
        hinge, _ = slab_forward(img, txt, prep, B, r * B, not fix_norm)
        total = total + hinge.sum()
        gi, gt = slab_backward(img, txt, prep, one, 1.0 / N if N else math.nan, B, r * B)
        dimg.append(gi)
        dtxt.append(gt)
    return total / N, torch.cat(dimg), torch.cat(dtxt)


# (B, G, E, row0) of the GPU kernel tests and the seed of each; the CPU suite bounds the share of near-zero hinge
# arguments ("fence" terms) of exactly these problems
GPU_PROBLEMS = (
    (37, 100, 256, 23),        # B and G not multiples of 16, row0 > 0
    (16, 64, 64, 48),
    (24, 72, 128, 0),
    (20, 48, 512, 16),
    (64, 256, 256, 64),
    (256, 2048, 256, 512),     # the fine-tune's shape on 8 ranks
)
GPU_SEED0 = 100
CLASSES = (('MaxMarginRankingLoss', 0.2), ('AdaptiveMaxMarginRankingLoss', 0.4))


def fence_masks(img, txt, margin, weight, delta):
    """Boolean [G,G] masks of the hinge terms whose float64 argument is within delta of zero (diagonals False)."""
    z_t, z_v = hinge_arguments(img, txt, margin, weight)
    return z_t.abs() < delta, z_v.abs() < delta


def fence_per_index(f_t, f_v):
    """F_i: the fence terms that involve index i -- as the own row (it moves cnt_i and its own sums) or as the column."""
    return f_t.sum(1) + f_v.sum(1) + f_t.sum(0) + f_v.sum(0)
