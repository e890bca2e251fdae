"""Device-side clip ingest: decoded uint8 frames [B,F,H,W,3] -> the float clip [B,3,F,S,S] the models start from, or
straight to the patch matrix of the first GEMM (lvl_clip_ingest / lvl_clip_ingest_patches, csrc/clip_ingest.hip).

The reference drivers build the clip per sample on CPU workers (main_pretrain.py:269-283):
`Permute([3,0,1,2])` -> `RandomResizedCrop(S, scale=(0.5, 1.0))` (training) or `Resize(S)` + `CenterCrop(S)`
(evaluation) -> `NormalizeVideo(mean, std)`, on float frames that hold the integers 0..255 as decoded, followed by the
default collate's `torch.stack`. Here the dataset hands over the uint8 frames and ONE int32 block per clip,
`{top, left, h, w, Ry, Rx, sy, sx}`: the region [top, top+h) x [left, left+w) of every frame is resized bilinearly to
Ry x Rx, the S x S window at (sy, sx) of that is taken and, if flip[b], mirrored along x. RandomResizedCrop is
Ry = Rx = S, sy = sx = 0; Resize + CenterCrop is region = frame, (Ry, Rx) = the resized extent, (sy, sx) = the crop origin.

What is restated is torchvision 0.11.2 (the reference's pin) ON TENSORS: bilinear, half-pixel centres,
align_corners=False, NO antialiasing -- F.interpolate(mode='bilinear', align_corners=False) on the cropped region.
Antialiased resizing (the default of newer torchvision releases) is not built. Neither torchvision nor the reference is
imported. Out of scope: colour jitter, per-frame boxes, sources of mixed resolution in one batch, variable F.

The arithmetic (include/lavila_hip.h, DESIGN.md "Clip ingest") has one definition on the device and one here
(`_axis`, `_restate`): float32, every operation rounded on its own, so CPU tensors and device tensors give the same
bits.
"""
import math

import torch
import torch.nn as nn

from . import _cabi as C

# (mean, std) of the reference drivers, in 0..255 units: main_pretrain.py:269-271 (the OpenAI CLIP statistics, every
# CLIP_OPENAI_* / VCLM_OPENAI_* model) and the ImageNet statistics of the other towers
OPENAI_MEAN_STD = ((108.3272985, 116.7460125, 104.09373615000001), (68.5005327, 66.6321579, 70.32316305))
IMAGENET_MEAN_STD = ((123.675, 116.28, 103.53), (58.395, 57.12, 57.375))

_DTYPE_CODES = {torch.float32: C.LVL_F32, torch.bfloat16: C.LVL_BF16, torch.float16: C.LVL_F16}


# --------------------------------------------------------------------------------------------------
# parameter blocks (host side)
# --------------------------------------------------------------------------------------------------
def whole_frame_params(B, H, W, S):
    """The whole frame resized to S x S."""
    return torch.tensor([[0, 0, H, W, S, S, 0, 0]] * B, dtype=torch.int32).reshape(B, 8)


def random_resized_crop_params(B, H, W, S, scale=(0.5, 1.0), ratio=(3 / 4, 4 / 3), generator=None):
    """One block per clip, torchvision 0.11.2's RandomResizedCrop.get_params restated: up to 10 attempts with the area
    uniform in `scale` (as a fraction of the frame) and the aspect log-uniform in `ratio`, w = round(sqrt(area * ar)),
    h = round(sqrt(area / ar)), accepted if it fits, then a uniform integer origin; after the attempts the central
    fallback with the ratio clamp. Drawn on the host from a torch CPU generator."""
    area = H * W
    log_ratio = torch.log(torch.tensor(ratio))
    out = torch.empty(B, 8, dtype=torch.int32)
    for b in range(B):
        for _ in range(10):
            target_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=generator).item()
            aspect = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1], generator=generator)).item()
            w = int(round(math.sqrt(target_area * aspect)))
            h = int(round(math.sqrt(target_area / aspect)))
            if 0 < w <= W and 0 < h <= H:
                i = torch.randint(0, H - h + 1, size=(1,), generator=generator).item()
                j = torch.randint(0, W - w + 1, size=(1,), generator=generator).item()
                break
        else:
            in_ratio = float(W) / float(H)
            if in_ratio < min(ratio):
                w = W
                h = int(round(w / min(ratio)))
            elif in_ratio > max(ratio):
                h = H
                w = int(round(h * max(ratio)))
            else:
                w, h = W, H
            i, j = (H - h) // 2, (W - w) // 2
        out[b] = torch.tensor([i, j, h, w, S, S, 0, 0], dtype=torch.int32)
    return out


def resize_center_crop_params(B, H, W, S):
    """The evaluation chain Resize(S) + CenterCrop(S) of torchvision 0.11.2: the short side goes to S, the long side to
    int(S * long / short); the crop origin is round((R - S) / 2) (Python's round, as there)."""
    short, long = (W, H) if W <= H else (H, W)
    new_long = int(S * long / short)
    Rx, Ry = (S, new_long) if W <= H else (new_long, S)
    sy, sx = int(round((Ry - S) / 2.0)), int(round((Rx - S) / 2.0))
    return torch.tensor([[0, 0, H, W, Ry, Rx, sy, sx]] * B, dtype=torch.int32).reshape(B, 8)


def validate_params(params, B, H, W, S):
    """The [B, 8] int32 host image of the blocks, or ValueError naming the first malformed one. The kernel forces every
    block into the frame for memory safety, so a wrong block has to be stopped here."""
    p = torch.as_tensor(params)
    if p.is_cuda:
        raise ValueError('clip ingest: parameter blocks are host tensors (they are validated before the launch); got a '
                         f'tensor on {p.device}')
    if p.dtype.is_floating_point or p.dtype == torch.bool or tuple(p.shape) != (B, 8):
        raise ValueError(f'clip ingest: params must be integers of shape ({B}, 8) = {{top, left, h, w, Ry, Rx, sy, sx}} '
                         f'per clip, got {p.dtype} {tuple(p.shape)}')
    p = p.to(torch.int64)
    for b, (top, left, h, w, Ry, Rx, sy, sx) in enumerate(p.tolist()):
        what = None
        if h < 1 or w < 1 or Ry < 1 or Rx < 1:
            what = 'h, w, Ry and Rx must be at least 1'
        elif top < 0 or left < 0 or top + h > H or left + w > W:
            what = f'the region leaves the {H} x {W} frame'
        elif sy < 0 or sx < 0 or sy + S > Ry or sx + S > Rx:
            what = f'the {S} x {S} window leaves the resized extent {Ry} x {Rx}'
        elif max(Ry, Rx) >= 1 << 24:
            what = 'resized extents are below 2^24 (exact in float32)'
        if what:
            raise ValueError(f'clip ingest: block {b} = {[top, left, h, w, Ry, Rx, sy, sx]}: {what}')
    return p.to(torch.int32).contiguous()


def _check_frames(frames):
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[-1] != 3:
        raise ValueError('clip ingest: frames are uint8 [B, F, H, W, 3] (RGB, channel last, as decoded), got '
                         f'{getattr(frames, "dtype", type(frames))} {tuple(getattr(frames, "shape", ()))}')
    if frames.numel() and (frames.stride(4) != 1 or frames.stride(3) != 3):
        raise ValueError(f'clip ingest: pixels must be 3 contiguous bytes (strides {frames.stride()}); clip, frame and row '
                         'strides are free')


def _host_flip(flip, B):
    if flip is None:
        return None
    f = torch.as_tensor(flip)
    if tuple(f.shape) != (B,):
        raise ValueError(f'clip ingest: flip holds one flag per clip, shape ({B},), got {tuple(f.shape)}')
    return (f != 0).to(torch.int32)


# --------------------------------------------------------------------------------------------------
# the restatement in plain torch (CPU tensors): the same operations in the same order, each rounded to float32
# --------------------------------------------------------------------------------------------------
def _axis(n, R, idx):
    """(i0, i1, lam) of the output indices idx (already offset by the window) of an axis resized from n to R."""
    scale = torch.tensor(float(n), dtype=torch.float32) / torch.tensor(float(R), dtype=torch.float32)
    s = scale * (idx.to(torch.float32) + 0.5) - 0.5
    s = s.clamp(min=0)
    i0 = s.to(torch.int64).clamp(max=n - 1)
    i1 = (i0 + 1).clamp(max=n - 1)
    return i0, i1, s - i0.to(torch.float32)


def _restate(frames, params, flip, S, mean, std):
    """frames u8 [B,F,H,W,3] (any device torch runs on), validated host blocks -> float32 [B,3,F,S,S]."""
    B, Fr = frames.shape[:2]
    dev = frames.device
    mean_t = torch.tensor(mean, dtype=torch.float32, device=dev)
    std_t = torch.tensor(std, dtype=torch.float32, device=dev)
    out = torch.empty(B, 3, Fr, S, S, dtype=torch.float32, device=dev)
    o = torch.arange(S)
    for b, (top, left, h, w, Ry, Rx, sy, sx) in enumerate(params.tolist()):
        xs = S - 1 - o if (flip is not None and int(flip[b])) else o          # the window is mirrored: flip after the crop
        y0, y1, ly = (t.to(dev) for t in _axis(h, Ry, o + sy))
        x0, x1, lx = (t.to(dev) for t in _axis(w, Rx, xs + sx))
        region = frames[b, :, top:top + h, left:left + w, :].to(torch.float32)          # [F, h, w, 3]
        r0, r1 = region[:, y0], region[:, y1]                                             # [F, S, w, 3]
        lx, ly = lx.view(1, 1, S, 1), ly.view(1, S, 1, 1)
        wx, wy = 1 - lx, 1 - ly
        upper = wx * r0[:, :, x0] + lx * r0[:, :, x1]
        lower = wx * r1[:, :, x0] + lx * r1[:, :, x1]
        v = wy * upper + ly * lower                                                       # [F, S, S, 3]
        out[b] = ((v - mean_t) / std_t).permute(3, 0, 1, 2)
    return out


# --------------------------------------------------------------------------------------------------
# device launches
# --------------------------------------------------------------------------------------------------
def _require_frames_on_device(frames):
    if not frames.is_cuda or frames.is_contiguous():
        C.require_device(frames)          # raises for host tensors and for another device than the current one
    elif frames.device.index != torch.cuda.current_device():
        C.require_device(frames.new_empty(1))


def _source_args(frames):
    B, Fr, H, W, _ = frames.shape
    return B, Fr, H, W, frames.stride(0), frames.stride(1), frames.stride(2)


class PendingClip:
    """A clip that has not been computed: the uint8 frames, the blocks and the statistics. It answers what the model entry
    points ask of their input (`shape` (B,3,F,S,S), `ndim` / `dim()`, `device`, `is_cuda`, `dtype` float32) and is turned
    into the patch matrix by `ops.patchify` in one kernel, without the float clip ever existing; `materialize(dtype)` gives
    that clip."""

    def __init__(self, frames, params, flip, crop_size, mean, std):
        _check_frames(frames)
        B, Fr, H, W, _ = frames.shape
        self.frames = frames
        self.crop_size = int(crop_size)
        self.params = validate_params(whole_frame_params(B, H, W, crop_size) if params is None else params, B, H, W,
                                      self.crop_size)
        self.flip = _host_flip(flip, B)
        self.mean, self.std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
        self.shape = torch.Size((B, 3, Fr, self.crop_size, self.crop_size))
        self._device_blocks = None

    ndim = 5
    dtype = torch.float32
    requires_grad = False

    def dim(self):
        return 5

    def size(self, d=None):
        return self.shape if d is None else self.shape[d]

    @property
    def device(self):
        return self.frames.device

    @property
    def is_cuda(self):
        return self.frames.is_cuda

    def _blocks(self):
        """(params, flip) on the frames' device, copied once"""
        if self._device_blocks is None:
            dev = self.frames.device
            self._device_blocks = (self.params.to(dev), None if self.flip is None else self.flip.to(dev))
        return self._device_blocks

    def materialize(self, dtype=torch.float32):
        """The clip [B,3,F,S,S]: lvl_clip_ingest on device frames, the plain-torch restatement on host frames."""
        if dtype not in _DTYPE_CODES:
            raise ValueError(f'clip ingest: float32, bfloat16 or float16, got {dtype}')
        S = self.crop_size
        if not self.frames.is_cuda:
            return _restate(self.frames, self.params, self.flip, S, self.mean, self.std).to(dtype)
        _require_frames_on_device(self.frames)
        B, Fr, H, W, cs, fs, rs = _source_args(self.frames)
        params, flip = self._blocks()
        out = torch.empty(B, 3, Fr, S, S, dtype=dtype, device=self.frames.device)
        C.check(C.lib().lvl_clip_ingest(C.ptr(self.frames), C.ptr(params), C.ptr(flip), C.ptr(out), B, Fr, H, W, S, cs, fs,
                                        rs, *self.mean, *self.std, _DTYPE_CODES[dtype], C.stream_ptr()), 'lvl_clip_ingest')
        return out

    def patches(self, patch, dtype, ld=None):
        """-> [B, F*N, ld]: what ops.patchify gives for materialize(), columns 3*P*P .. ld zero (lvl_clip_ingest_patches)."""
        _require_frames_on_device(self.frames)
        B, Fr, H, W, cs, fs, rs = _source_args(self.frames)
        S = self.crop_size
        ld = 3 * patch * patch if ld is None else int(ld)
        params, flip = self._blocks()
        out = torch.empty(B, Fr * (S // patch) ** 2 if patch > 0 else 0, ld, dtype=dtype, device=self.frames.device)
        C.check(C.lib().lvl_clip_ingest_patches(C.ptr(self.frames), C.ptr(params), C.ptr(flip), C.ptr(out), B, Fr, H, W, S,
                                                patch, ld, cs, fs, rs, *self.mean, *self.std, C.dtype_code(out),
                                                C.stream_ptr()), 'lvl_clip_ingest_patches')
        return out

    def __repr__(self):
        return f'PendingClip(shape={tuple(self.shape)}, frames={tuple(self.frames.shape)} on {self.frames.device})'


def refuse_pending(x, who):
    """Entry points that cannot take a PendingClip say so (TypeError) instead of failing somewhere inside."""
    if isinstance(x, PendingClip):
        raise TypeError(f'{who} does not take a PendingClip (channel-major [B,3,F,S,S], not computed yet): materialize it '
                        'first, `clip = pending.materialize()`')


class ClipIngest(nn.Module):
    """uint8 frames [B,F,H,W,3] -> the clip [B,3,F,S,S] exactly as the reference's transform chain followed by torch.stack
    hands it to the model (module docstring): crop / resize (bilinear, align_corners=False, NOT antialiased -- torchvision
    0.11.2 on tensors), optional flip, (x - mean) / std. On device frames one HIP kernel, on host frames the same
    arithmetic in plain torch. `pending()` defers the work to the model's patch gather."""

    def __init__(self, crop_size, mean=OPENAI_MEAN_STD[0], std=OPENAI_MEAN_STD[1]):
        super().__init__()
        self.crop_size = int(crop_size)
        if self.crop_size < 2 or self.crop_size % 2:
            raise ValueError(f'ClipIngest: crop_size must be even (patches are even), got {crop_size}')
        self.mean, self.std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
        if len(self.mean) != 3 or len(self.std) != 3 or not all(s > 0 and math.isfinite(s) for s in self.std):
            raise ValueError('ClipIngest: mean and std are three numbers each, std positive')

    def pending(self, frames, params=None, flip=None):
        return PendingClip(frames, params, flip, self.crop_size, self.mean, self.std)

    def forward(self, frames, params=None, flip=None, dtype=torch.float32):
        """params: [B, 8] host integers (None: the whole frame resized to S x S); flip: [B] flags or None."""
        return self.pending(frames, params, flip).materialize(dtype)

    def extra_repr(self):
        return f'crop_size={self.crop_size}, mean={self.mean}, std={self.std}'
