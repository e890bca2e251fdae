"""Contrastive (InfoNCE) loss of the dual encoder behind the reference interface
(`lavila/models/loss.py`: gather_features :18-43, CLIPLoss :46-118, SSLCLIPLoss :121-217) and the max-margin ranking
losses of the retrieval fine-tune (sim_matrix :256-264, MaxMarginRankingLoss :267-312, AdaptiveMaxMarginRankingLoss
:315-367; see _MarginRankingFn), and the narrator's criterion (CaptionLoss :220-253; see _CaptionFn).

Same constructor, same `criterion(outputs) -> {'loss','clip_loss','clip_acc'}` contract, same numbers.
The plan is MI355X-first instead of a translation of the reference's NCCL call pattern:

  reference (vissl path)                         here
  ------------------------------------------    -----------------------------------------------------
  2 x all_gather (img, txt), list + cat          1 x all_gather_into_tensor of [B, 2E] (img | txt)
  every rank computes the full G x G logits      each rank computes its two [B, G] slabs (its rows of
  and both cross-entropies (O(G^2) per rank)     logits_per_image and of logits_per_text): O(G^2 / W)
  backward: 2 x all_reduce of [W,B,E] grads      backward: none -- one tiny all_gather of the 2B row
  (+ slice own rank)                             LSEs (+3 partial sums) in forward makes the local
                                                 gradient computable from the gathered embeddings alone

Gradient convention (pinned by tests/golden/clip_loss_multirank.pt): with
`use_vissl=True` the reference hands each rank W x d(global loss)/d(local embeddings) (GatherLayer
backward sums W identical copies; DDP's 1/W averaging restores the true gradient); with the default
`gather_features` path it hands 1 x. Both are reproduced. d(loss)/d(logit_scale) is the full global
derivative on every rank in both modes, as in the reference.

What is gathered, in which dtype, and `row0` is written once, in `_Exchange` (tests/test_loss_exchange_cpu.py).
"""
import torch
import torch.distributed as dist
import torch.nn as nn

from . import ops
from .distributed_utils import all_gather_rows


class _Exchange:
    """The batch exchange every loss below makes in forward: one rank-ordered gather of the local rows as [img | txt]
    (`extra` given: as float32 [img | txt | extra], the per-row indicator / weight riding along as the last column), then
    -- behind the slab kernels -- `gather_record`. W = 1 issues no collective. Holds B, E, G, W, row0 and img_all,
    txt_all, extra_all ([G], float32 off the wire; the caller's own tensor on one rank)."""

    def __init__(self, image_embed, text_embed, W, rank, extra=None):
        B, E = image_embed.shape
        # compute dtype: the embeddings' common dtype when the kernels take it, float32 otherwise
        dt = image_embed.dtype if (image_embed.dtype == text_embed.dtype and
                                   image_embed.dtype in (torch.float32, torch.bfloat16)) else torch.float32
        img, txt = image_embed.detach().to(dt), text_embed.detach().to(dt)
        if W > 1:
            cols = [img, txt] if extra is None else [img.float(), txt.float(), extra.float()[:, None]]
            both = all_gather_rows(torch.cat(cols, dim=1))                     # [G, 2E (+1)], rank-ordered
            img_all, txt_all = both[:, :E].to(dt).contiguous(), both[:, E:2 * E].to(dt).contiguous()
            extra = None if extra is None else both[:, 2 * E]
        else:
            img_all, txt_all = img.contiguous(), txt.contiguous()
        self.B, self.E, self.G, self.W, self.row0 = B, E, img_all.shape[0], W, (rank * B if W > 1 else 0)
        self.img_all, self.txt_all = img_all, txt_all
        self.extra_all = None if extra is None else extra.contiguous()

    def gather_record(self, part, lse=None):
        """W > 1: one gather of this rank's [1, n] record [lse (2B) | part]. Returns the row LSEs of all ranks as [2, G]
        (None without `lse`) and the ranks' partial sums [W, len(part)]."""
        allp = all_gather_rows((part if lse is None else torch.cat([lse.reshape(-1), part]))[None])
        if lse is None:
            return None, allp
        n = 2 * self.B
        return allp[:, :n].reshape(self.W, 2, self.B).permute(1, 0, 2).reshape(2, self.G).contiguous(), allp[:, n:]


class _ContrastiveFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, image_embed, text_embed, logit_scale, crit):
        x = _Exchange(image_embed, text_embed, crit.world_size, crit.rank)
        B, G, W, row0, img_all, txt_all = x.B, x.G, x.W, x.row0, x.img_all, x.txt_all
        scale = logit_scale.detach().float().reshape(1).contiguous()

        stats, argmax = crit._slab_forward(img_all, txt_all, scale, B, row0)   # [2,B,4] f32, [2,B] i32
        lse, diag, expect = stats[..., 0], stats[..., 1], stats[..., 2]
        labels = torch.arange(row0, row0 + B, device=argmax.device, dtype=torch.int32)
        part = torch.stack([(lse - diag).sum(), (expect - diag).sum(),
                            (argmax[0] == labels).sum().float()])
        # local_loss (loss.py:86-88, 99-100; only on the gather_features path): every rank's loss is the mean over
        # ITS rows of the two slabs -- exactly what _slab_forward produced -- and is not averaged over ranks
        local = bool(crit.local_loss) and W > 1 and not crit.use_vissl
        if W > 1 and (not local or crit.gather_with_grad):
            lse_all, parts = x.gather_record(part, lse)                        # [1, 2B+3] per rank
            sums = parts.sum(0)
        elif W > 1:                            # local rows only: the kernel reads nothing but the own entries
            lse_all = lse.new_zeros(2, G)
            lse_all[:, row0:row0 + B] = lse
            sums = part
        else:
            lse_all, sums = lse.contiguous(), part
        if local:
            sums = part
            loss = part[0] / (2 * B)
            acc = 100.0 * part[2] / B
        else:
            loss = sums[0] / (2 * G)
            acc = 100.0 * sums[2] / G
        ctx.save_for_backward(img_all, txt_all, lse_all, scale, sums)
        ctx.cfg = (B, G, row0, W, crit, image_embed.dtype, text_embed.dtype, logit_scale.dtype)
        ctx.local = local
        ctx.mark_non_differentiable(acc)
        crit._last_pred = argmax[0]
        return loss, acc

    @staticmethod
    def backward(ctx, dloss, dacc):
        img_all, txt_all, lse_all, scale, sums = ctx.saved_tensors
        B, G, row0, W, crit, idt, tdt, sdt = ctx.cfg
        up = dloss.detach().float().reshape(1).contiguous()
        if ctx.local:
            # with gather_with_grad the all-gather's backward sums, on the owner of a row, the column terms of EVERY
            # rank's local loss (each weighted 1/(2B)): rows + columns over the global batch, as in the vissl path;
            # without it the gathered rows are constants and only the row terms of the own loss remain.
            # ASSUMPTION (holds for loss.backward() and any rank-uniform loss scaling such as GradScaler): every rank
            # feeds the same upstream gradient `dloss` -- this rank's value stands in for the other ranks' in the column
            # terms, which is what lets the backward run without a collective. Per-rank loss weights would need the
            # reference's torch.distributed.nn.all_gather backward instead.
            dimg, dtxt = crit._slab_backward(img_all, txt_all, lse_all, scale, up, 1.0 / (2 * B), B, row0,
                                             rows_only=not crit.gather_with_grad)
            dscale = up[0] * sums[1] / (2 * B) / scale[0]
            return dimg.to(idt), dtxt.to(tdt), dscale.to(sdt), None
        mult = float(W) if (crit.use_vissl or crit.gather_with_grad) else 1.0
        dimg, dtxt = crit._slab_backward(img_all, txt_all, lse_all, scale, up, mult / (2 * G), B, row0)
        dscale = up[0] * sums[1] / (2 * G) / scale[0]
        return dimg.to(idt), dtxt.to(tdt), dscale.to(sdt), None


class CLIPLoss(nn.Module):
    """Symmetric InfoNCE over the global batch -- loss.py:46-118."""

    def __init__(self, use_vissl=False, local_loss=False, gather_with_grad=False, cache_labels=False, rank=0,
                 world_size=1):
        super().__init__()
        self.use_vissl = use_vissl
        self.local_loss = local_loss
        self.gather_with_grad = gather_with_grad
        self.cache_labels = cache_labels
        self.rank = rank
        self.world_size = world_size
        # cache state (kept for interface parity; labels are implicit in the slab kernel: row0 + i)
        self.prev_num_logits = 0
        self.labels = {}
        self._last_pred = None

    # -- kernel hooks (tests override these two with the CPU oracle to exercise the collectives on gloo) ---
    def _slab_forward(self, img_all, txt_all, scale, B, row0):
        stats, argmax, _ = ops.clip_loss_fwd_raw(img_all, txt_all, scale, B, row0, want_logits=False)
        return stats, argmax

    def _slab_backward(self, img_all, txt_all, lse_all, scale, upstream, coef, B, row0, rows_only=False):
        return ops.clip_loss_bwd_raw(img_all, txt_all, lse_all, scale, upstream, coef, B, row0, rows_only)

    def forward(self, outputs):
        image_features = outputs['image_embed']
        text_features = outputs['text_embed']
        logit_scale = outputs['logit_scale']
        if self.world_size > 1 and not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError('CLIPLoss(world_size>1) needs an initialised torch.distributed process group')
        if self.world_size > 1 and self.use_vissl and self.local_loss:
            # the reference builds GLOBAL logits on the vissl path and then offsets the labels by num_logits * rank
            # (loss.py:74-79,99-100): out-of-range targets, an error there as well. Not silently turned into the
            # global loss here.
            raise NotImplementedError('CLIPLoss(use_vissl=True, local_loss=True) on several ranks indexes labels out of '
                                      'range in the reference (loss.py:99-100); not reproduced')
        loss, acc = _ContrastiveFn.apply(image_features, text_features, logit_scale, self)
        return {'loss': loss, 'clip_loss': loss, 'clip_acc': acc}

    @torch.no_grad()
    def debug_slabs(self, outputs):
        """Parity-test helper: this rank's scaled logits slabs [2,B,G] (f32), row predictions and labels
        (int64, global column indices) -- what loss.py:78-79,96-105,113 materialise."""
        x = _Exchange(outputs['image_embed'], outputs['text_embed'], self.world_size, self.rank)
        B, row0, img_all, txt_all = x.B, x.row0, x.img_all, x.txt_all
        scale = outputs['logit_scale'].detach().float().reshape(1).contiguous()
        _, argmax, logits = ops.clip_loss_fwd_raw(img_all, txt_all, scale, B, row0, want_logits=True)
        labels = torch.arange(row0, row0 + B, device=img_all.device, dtype=torch.long)
        return {'logits': logits, 'pred': argmax.long(), 'labels': labels}


def gather_features(image_features, text_features, local_loss=False, gather_with_grad=False, rank=0, world_size=1):
    """loss.py:18-43 for API completeness (the loss above does not need it)."""
    from .distributed_utils import GatherLayer
    if gather_with_grad:
        return GatherLayer.apply(image_features), GatherLayer.apply(text_features)
    B = image_features.shape[0]
    all_img, all_txt = all_gather_rows(image_features.detach()), all_gather_rows(text_features.detach())
    if not local_loss:
        all_img = torch.cat([all_img[:rank * B], image_features, all_img[(rank + 1) * B:]], 0)
        all_txt = torch.cat([all_txt[:rank * B], text_features, all_txt[(rank + 1) * B:]], 0)
    return all_img, all_txt


class _SSLContrastiveFn(torch.autograd.Function):
    """Slab-parallel SSLCLIPLoss: same exchange plan as _ContrastiveFn (one fused all-gather of [img|txt|ind], one
    small all-gather of row LSEs + partial sums, no backward collective)."""

    @staticmethod
    def forward(ctx, image_embed, text_embed, logit_scale, scale_pseudo, indicators, crit):
        dev = image_embed.device
        x = _Exchange(image_embed, text_embed, crit.world_size, crit.rank, indicators.detach().to(dev).reshape(-1))
        B, G, W, row0, img_all, txt_all = x.B, x.G, x.W, x.row0, x.img_all, x.txt_all
        ind_all = (x.extra_all.round() if W > 1 else x.extra_all).to(torch.int32).contiguous()
        real, pseudo = logit_scale.detach().float().reshape(()), scale_pseudo.detach().float().reshape(())
        scales3 = torch.stack([pseudo, torch.sqrt(pseudo * real), real]).contiguous()

        stats, argmax = crit._slab_forward(img_all, txt_all, ind_all, scales3, B, row0)     # [2,B,8], [2,B]
        lse, diag_l, diag_z = stats[..., 0], stats[..., 1], stats[..., 5]
        ind_loc = ind_all[row0:row0 + B]
        labels = torch.arange(row0, row0 + B, device=dev, dtype=torch.int32)
        ok = (argmax[0] == labels)
        bucket_diag = 2 * ind_loc                                                            # mask of (i,i)
        ds = [(stats[..., 2 + k] - diag_z * (bucket_diag == k).float()[None]).sum() for k in range(3)]
        part = torch.stack([(lse - diag_l).sum(), ds[0], ds[1], ds[2], ok.sum().float(),
                            (ok & (ind_loc == 1)).sum().float(), (ok & (ind_loc == 0)).sum().float()])
        if W > 1:
            lse_all, parts = x.gather_record(part, lse)                                    # [1, 2B+7] per rank
            sums = parts.sum(0)
        else:
            lse_all, sums = lse.contiguous(), part
        num_gt = (ind_all == 1).sum().float()
        num_pseudo = (ind_all == 0).sum().float()
        loss = sums[0] / (2 * G)
        acc = 100.0 * sums[4] / G
        acc_gt = 100.0 * sums[5] / num_gt
        acc_pseudo = 100.0 * sums[6] / num_pseudo
        ctx.save_for_backward(img_all, txt_all, ind_all, lse_all, scales3, sums)
        ctx.cfg = (B, G, row0, W, crit, image_embed.dtype, text_embed.dtype, logit_scale.dtype, scale_pseudo.dtype)
        ctx.mark_non_differentiable(acc, acc_gt, acc_pseudo, num_gt, num_pseudo)
        return loss, acc, acc_gt, acc_pseudo, num_gt, num_pseudo

    @staticmethod
    def backward(ctx, dloss, *unused):
        img_all, txt_all, ind_all, lse_all, scales3, sums = ctx.saved_tensors
        B, G, row0, W, crit, idt, tdt, sdt, pdt = ctx.cfg
        mult = float(W) if crit.use_vissl else 1.0
        up = dloss.detach().float().reshape(1).contiguous()
        dimg, dtxt = crit._slab_backward(img_all, txt_all, ind_all, lse_all, scales3, up, mult / (2 * G), B, row0)
        pseudo, geo, real = scales3[0], scales3[1], scales3[2]
        d0, d1, d2 = (up[0] * sums[1 + k] / (2 * G) for k in range(3))     # d loss / d scales3[k]
        dreal = d2 + d1 * 0.5 * geo / real                                   # d sqrt(p r)/dr = sqrt(p r) / (2 r)
        dpseudo = d0 + d1 * 0.5 * geo / pseudo
        return dimg.to(idt), dtxt.to(tdt), dreal.to(sdt), dpseudo.to(pdt), None, None


class SSLCLIPLoss(nn.Module):
    """InfoNCE with per-pair temperature for pseudo-labelled narrations -- loss.py:121-217. `forward(outputs,
    gt_indicators)`; same constructor, same output dict (loss, clip_loss, num_gt, num_pseudo, clip_acc, clip_acc_gt,
    clip_acc_pseudo) and the learnable `logit_scale_pseudo` parameter."""

    def __init__(self, use_vissl=False, local_loss=False, gather_with_grad=False, cache_labels=False, rank=0,
                 world_size=1, scale_init=0.08, freeze_scale=False):
        super().__init__()
        import numpy as np
        self.use_vissl = use_vissl
        self.local_loss = local_loss          # ignored on one rank, as in the reference; see forward() for W > 1
        self.gather_with_grad = gather_with_grad
        self.cache_labels = cache_labels
        self.rank = rank
        self.world_size = world_size
        self.logit_scale_pseudo = nn.Parameter(torch.ones([]) * np.log(1 / scale_init))
        if freeze_scale:
            self.logit_scale_pseudo.requires_grad = False
        self.prev_num_logits = 0
        self.labels = {}

    # -- kernel hooks (tests override these two with the CPU oracle to exercise the collectives on gloo) ---
    def _slab_forward(self, img_all, txt_all, ind_all, scales3, B, row0):
        stats, argmax, _ = ops.ssl_clip_loss_fwd_raw(img_all, txt_all, ind_all, scales3, B, row0)
        return stats, argmax

    def _slab_backward(self, img_all, txt_all, ind_all, lse_all, scales3, upstream, coef, B, row0):
        return ops.ssl_clip_loss_bwd_raw(img_all, txt_all, ind_all, lse_all, scales3, upstream, coef, B, row0)

    def forward(self, outputs, gt_indicators):
        if self.world_size > 1:
            if not self.use_vissl:
                raise NotImplementedError      # as the reference (loss.py:167-168)
            if self.local_loss:
                # the reference offsets the labels by num_logits * rank although its vissl logits are already global
                # (loss.py:185-186): out-of-range targets, an error there too
                raise NotImplementedError('SSLCLIPLoss(local_loss=True) on several ranks indexes labels out of range '
                                          'in the reference (loss.py:185-186); not reproduced')
            if not (dist.is_available() and dist.is_initialized()):
                raise RuntimeError('SSLCLIPLoss(world_size>1) needs an initialised torch.distributed process group')
        loss, acc, acc_gt, acc_pseudo, num_gt, num_pseudo = _SSLContrastiveFn.apply(
            outputs['image_embed'], outputs['text_embed'], outputs['logit_scale'], self.logit_scale_pseudo.exp(),
            gt_indicators, self)
        return {'loss': loss, 'clip_loss': loss, 'num_gt': num_gt.reshape(1).long().cpu(),
                'num_pseudo': num_pseudo.reshape(1).long().cpu(), 'clip_acc': acc, 'clip_acc_gt': acc_gt,
                'clip_acc_pseudo': acc_pseudo}


def sim_matrix(a, b, eps=1e-8):
    """loss.py:256-264 for API completeness (the losses below never build the matrix)."""
    unit = [t / t.norm(dim=1, keepdim=True).clamp_min(eps) for t in (a, b)]
    return unit[0] @ unit[1].t()


class _MarginRankingFn(torch.autograd.Function):
    """Slab-parallel max-margin ranking loss (loss.py:267-367).

      reference                                         here
      ----------------------------------------------    -------------------------------------------------------
      2-3 x gather_from_all (img, txt, weight)          1 x all_gather_rows of [img | txt | w]
      every rank: the G x G cosine matrix, four G^2     each rank: its rows of both directions, two [B,G] sweeps
      index-selected copies, a nonzero (host sync)      that never reach HBM; no host sync
      backward: all_reduce of [W,B,E] per gather        backward: none -- the thresholds c_j of all rows come from
                                                        the gathered rows, so the local gradient needs no other
                                                        rank's result; one tiny gather of the partial sums in forward

    Gradient convention: as on the vissl path of CLIPLoss, GatherLayer.backward sums W identical copies, so each rank
    receives W x d(global loss)/d(its local rows). `weight` receives no gradient (the drivers pass data, not parameters).
    """

    @staticmethod
    def forward(ctx, image_embed, text_embed, weight, crit):
        from .distributed_utils import is_distributed_training_run
        W = dist.get_world_size() if is_distributed_training_run() else 1
        rank = dist.get_rank() if W > 1 else 0
        w = None if weight is None else weight.detach().to(image_embed.device).float().reshape(-1)
        if w is not None and w.shape[0] != image_embed.shape[0]:
            raise ValueError(f'weight has {w.shape[0]} entries for {image_embed.shape[0]} pairs')
        x = _Exchange(image_embed, text_embed, W, rank, w)
        B, G, row0, img_all, txt_all, w_all = x.B, x.G, x.row0, x.img_all, x.txt_all, x.extra_all
        N = 2 * G * (G - 1) if crit.fix_norm else 2 * G * G

        prep = crit._slab_prepare(img_all, txt_all, w_all, crit.margin)                          # [7,G] f32
        hinge, _ = crit._slab_forward(img_all, txt_all, prep, B, row0, not crit.fix_norm)    # [2,B] f32, [2,B] i32
        part = hinge.sum().reshape(1)
        total = x.gather_record(part)[1].sum() if W > 1 else part.sum()                      # [1, 1] per rank
        loss = total / N                                 # G = 1 with fix_norm: 0 / 0 = NaN, the reference's empty mean
        ctx.save_for_backward(img_all, txt_all, prep)
        ctx.cfg = (B, row0, W, N, crit, image_embed.dtype, text_embed.dtype)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        img_all, txt_all, prep = ctx.saved_tensors
        B, row0, W, N, crit, idt, tdt = ctx.cfg
        up = dloss.detach().float().reshape(1).contiguous()
        coef = float(W) / N if N else float('nan')
        dimg, dtxt = crit._slab_backward(img_all, txt_all, prep, up, coef, B, row0)
        return dimg.to(idt), dtxt.to(tdt), None, None


class MaxMarginRankingLoss(nn.Module):
    """Bidirectional max-margin ranking loss over the global batch -- loss.py:267-312. Same constructor, same
    `forward(outputs, weight=None)` (the weight is ignored, as there), same output dict. Whether the batch is
    gathered is decided as in the reference (`is_distributed_training_run()`), not by constructor arguments."""

    adaptive = False

    def __init__(self, margin=0.2, fix_norm=True):
        super().__init__()
        self.fix_norm = fix_norm
        self.loss = nn.MarginRankingLoss(margin)         # attribute parity (loss.py:272); carries no state
        self.margin = margin

    # -- kernel hooks (tests override these three with the CPU restatement to exercise the collectives on gloo) ---
    def _slab_prepare(self, img_all, txt_all, weight_all, margin):
        return ops.margin_loss_prepare_raw(img_all, txt_all, weight_all, margin)

    def _slab_forward(self, img_all, txt_all, prep, B, row0, with_diag):
        return ops.margin_loss_fwd_raw(img_all, txt_all, prep, B, row0, with_diag)

    def _slab_backward(self, img_all, txt_all, prep, upstream, coef, B, row0):
        return ops.margin_loss_bwd_raw(img_all, txt_all, prep, upstream, coef, B, row0)

    def forward(self, outputs, weight=None):
        if self.adaptive and weight is None:
            raise ValueError('AdaptiveMaxMarginRankingLoss needs the per-pair `weight` (forward(outputs, weight)): its '
                             'margin is margin * weight')
        loss = _MarginRankingFn.apply(outputs['image_embed'], outputs['text_embed'],
                                      weight if self.adaptive else None, self)
        return {'loss': loss, 'max_margin_loss': loss}


class AdaptiveMaxMarginRankingLoss(MaxMarginRankingLoss):
    """The same loss with the per-pair margin `margin * weight_i` -- loss.py:315-367."""

    adaptive = True

    def __init__(self, margin=0.4, fix_norm=True):
        super().__init__(margin=margin, fix_norm=fix_norm)


class _CaptionFn(torch.autograd.Function):
    """Token cross-entropy of the narrator in row form (loss.py:220-253).

      reference                                            here
      -----------------------------------------------      ------------------------------------------------------
      F.cross_entropy(reduction='none') on [B,V,T]:         one pass over each of the B*T rows: lse, the label's
      log-softmax image of the logits, then a gather         logit, the first argmax (csrc/caption_loss.hip)
      a Python loop over B with an argmax of [V,T] each      one small reduce kernel: loss, caption_acc, ppl, on
      and B host read-backs for ppl                          the device, no read-back
      backward: softmax image kept from forward              backward: softmax recomputed from the logits and the
                                                             saved per-row lse, written once in the logits' dtype

    Saved for backward: the logits themselves (no copy when they arrive as the permuted view VCLM_HF.forward returns),
    the labels and lse."""

    @staticmethod
    def forward(ctx, logits, labels, crit):
        B, V, T = logits.shape
        if tuple(labels.shape) != (B, T):
            raise ValueError(f'labels {tuple(labels.shape)} for logits {tuple(logits.shape)}: want [B, T] and [B, V, T]')
        x = logits.detach()
        in_place = (x.dtype in (torch.float32, torch.bfloat16) and x.stride(1) == 1 and x.stride(2) >= V and
                    x.stride(0) == T * x.stride(2))
        if in_place:                                     # [B,V,T] view of [B*T, >= V] rows: read where it lies
            rows = x.as_strided((B * T, V), (x.stride(2), 1), x.storage_offset())
        else:                                            # any other layout or dtype: one copy into padded rows
            dt = x.dtype if x.dtype in (torch.float32, torch.bfloat16) else torch.float32
            buf = torch.empty(B * T, (V + 7) // 8 * 8, dtype=dt, device=x.device)
            buf.view(B, T, -1)[:, :, :V].copy_(x.permute(0, 2, 1))
            rows = buf[:, :V]
        lab = labels.detach().to(device=x.device, dtype=torch.int64).reshape(-1)   # a [B,T] copy of text[:, 1:] at most
        lse, nll, _, correct, counted = crit._token_forward(rows, lab, crit.pad_id)
        res = crit._token_reduce(nll, correct, counted, B, T)                        # [3] f32
        loss, acc, ppl = res[0], res[1], res[2]
        ctx.save_for_backward(logits if in_place else rows, lab, lse)
        ctx.cfg = (B, V, T, in_place, crit, logits.dtype)
        ctx.mark_non_differentiable(acc, ppl)
        return loss, acc, ppl

    @staticmethod
    def backward(ctx, dloss, *unused):
        kept, lab, lse = ctx.saved_tensors
        B, V, T, in_place, crit, dtype = ctx.cfg
        rows = kept.as_strided((B * T, V), (kept.stride(2), 1), kept.storage_offset()) if in_place else kept
        up = dloss.detach().float().reshape(1).contiguous()
        grad = crit._token_backward(rows, lab, lse, up, 1.0 / (B * T), crit.pad_id)   # [B*T, Vp], the rows' dtype
        grad = grad.view(B, T, -1)[:, :, :V].permute(0, 2, 1)                          # [B, V, T] view of it
        return grad.to(dtype), None, None


class CaptionLoss(nn.Module):
    """Teacher-forced token cross-entropy, token accuracy and perplexity of the narrator -- loss.py:220-253. Same
    constructor (the pad id is read from `tokenizer.pad_token_id`, so a tokenizer is required, as there), same
    `forward(outputs)` on {'text_tokens_logits': [B, V, T], 'labels': [B, T]} (what VCLM_HF.forward returns), same
    output keys.

    Departures: `loss` / `caption_loss` are 0-dim float32 whatever the logits' dtype; `caption_acc` and `ppl` are
    non-differentiable 0-dim float32 tensors ON THE LOGITS' DEVICE (the reference assembles `ppl` from B `.item()`
    read-backs into a CPU tensor; the drivers only call `.item()` on it). A label that is neither the pad id nor inside
    [0, V) makes the loss NaN where torch raises a device assertion. float16 logits are computed in float32."""

    def __init__(self, pad_id=0, tokenizer=None):
        super().__init__()
        self.pad_id = pad_id
        self.tokenizer = tokenizer
        self.pad_id = tokenizer.pad_token_id

    # -- kernel hooks (tests override these three with the CPU restatement to exercise the host logic) ---
    def _token_forward(self, rows, labels, pad_id):
        return ops.token_xent_fwd_raw(rows, labels, pad_id)

    def _token_reduce(self, nll, correct, counted, B, T):
        return ops.token_xent_reduce_raw(nll, correct, counted, B, T)

    def _token_backward(self, rows, labels, lse, upstream, coef, pad_id):
        return ops.token_xent_bwd_raw(rows, labels, lse, upstream, coef, pad_id)

    def forward(self, outputs):
        loss, acc, ppl = _CaptionFn.apply(outputs['text_tokens_logits'], outputs['labels'], self)
        return {'loss': loss, 'caption_loss': loss, 'caption_acc': acc, 'ppl': ppl}
