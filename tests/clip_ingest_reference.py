"""References for the clip ingest (lavila_amd/ingest.py, csrc/clip_ingest.hip): a float64 oracle with exact source
coordinates, the float32 restatement of the reference's transform chain through F.interpolate, a gather-based copy of it
that takes injected faults, the derived error bound and the case table shared by the CPU and the GPU tests.

What is restated is torchvision 0.11.2 (the reference's pin) on tensors: `resized_crop` / `resize` are
F.interpolate(mode='bilinear', align_corners=False) without antialiasing on the cropped region, `CenterCrop` a slice,
`NormalizeVideo` (x - mean) / std. torchvision is not installed here and is not imported.

A block is {top, left, h, w, Ry, Rx, sy, sx}: region [top, top+h) x [left, left+w) resized to Ry x Rx, the S x S window at
(sy, sx) of that, mirrored along x if flip[b].
"""
import functools

import torch
import torch.nn.functional as F

MEAN_STD = {
    'openai': ((108.3272985, 116.7460125, 104.09373615000001), (68.5005327, 66.6321579, 70.32316305)),
    'imagenet': ((123.675, 116.28, 103.53), (58.395, 57.12, 57.375)),
}


# ---- float64 oracle -----------------------------------------------------------------------------------------------
def _exact_axis(n, R, idx):
    """Source coordinate s = n/R * (o + 1/2) - 1/2 = (n (2 o + 1) - R) / (2 R), clamped at 0, from INTEGERS: i0 is an
    integer division and lam one float64 division of two exact integers (no float32 anywhere)."""
    num = (n * (2 * idx.to(torch.int64) + 1) - R).clamp(min=0)
    i0 = torch.div(num, 2 * R, rounding_mode='floor').clamp(max=n - 1)
    lam = (num - i0 * 2 * R).to(torch.float64) / float(2 * R)
    i1 = (i0 + 1).clamp(max=n - 1)
    return i0, i1, lam


def oracle64(frames, params, flip, S, mean, std):
    """frames u8 [B,F,H,W,3] -> float64 [B,3,F,S,S]"""
    B, Fr = frames.shape[:2]
    out = torch.empty(B, 3, Fr, S, S, dtype=torch.float64)
    o = torch.arange(S)
    m = torch.tensor(mean, dtype=torch.float32).double()          # the statistics ARE float32 numbers
    s = torch.tensor(std, dtype=torch.float32).double()
    for b, (top, left, h, w, Ry, Rx, sy, sx) in enumerate(torch.as_tensor(params).tolist()):
        xs = S - 1 - o if (flip is not None and int(flip[b])) else o
        y0, y1, ly = _exact_axis(h, Ry, o + sy)
        x0, x1, lx = _exact_axis(w, Rx, xs + sx)
        reg = frames[b, :, top:top + h, left:left + w, :].double()
        r0, r1 = reg[:, y0], reg[:, y1]
        lx, ly = lx.view(1, 1, S, 1), ly.view(1, S, 1, 1)
        v = (1 - ly) * ((1 - lx) * r0[:, :, x0] + lx * r0[:, :, x1]) + ly * ((1 - lx) * r1[:, :, x0] + lx * r1[:, :, x1])
        out[b] = ((v - m) / s).permute(3, 0, 1, 2)
    return out


# ---- the reference chain in float32 -----------------------------------------------------------------------------------
def restate_interpolate(frames, params, flip, S, mean, std):
    """Permute -> crop + resize (F.interpolate) -> window -> flip -> normalise, per sample, then stack: float32 [B,3,F,S,S]"""
    m = torch.tensor(mean, dtype=torch.float32).view(3, 1, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(3, 1, 1, 1)
    out = []
    for b, (top, left, h, w, Ry, Rx, sy, sx) in enumerate(torch.as_tensor(params).tolist()):
        x = frames[b].permute(3, 0, 1, 2).float()[:, :, top:top + h, left:left + w]
        x = F.interpolate(x, size=(Ry, Rx), mode='bilinear', align_corners=False)[:, :, sy:sy + S, sx:sx + S]
        if flip is not None and int(flip[b]):
            x = x.flip(-1)
        out.append((x - m) / s)
    return torch.stack(out)


FAULTS = ('no_half_pixel', 'align_corners', 'origin_off_by_one', 'flip_before_window')


def _f32_axis(n, R, idx, fault):
    n_t, R_t = torch.tensor(float(n)), torch.tensor(float(R))
    if fault == 'align_corners':
        s = ((n_t - 1) / (R_t - 1) if R > 1 else torch.tensor(0.)) * idx.float()
    elif fault == 'no_half_pixel':
        s = (n_t / R_t) * idx.float()
    else:
        s = (n_t / R_t) * (idx.float() + 0.5) - 0.5
    s = s.clamp(min=0)
    i0 = s.long().clamp(max=n - 1)
    return i0, (i0 + 1).clamp(max=n - 1), (s - i0.float()).clamp(0, 1)


def restate_gather(frames, params, flip, S, mean, std, fault=None):
    """A float32 copy of the chain written with gathers, so that one of FAULTS can be put into it; fault=None is the
    chain itself (and has to stay inside the bound, or a rejection would prove nothing)."""
    assert fault is None or fault in FAULTS
    B, Fr, H, W, _ = frames.shape
    m, s = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    out = torch.empty(B, 3, Fr, S, S)
    o = torch.arange(S)
    for b, (top, left, h, w, Ry, Rx, sy, sx) in enumerate(torch.as_tensor(params).tolist()):
        if fault == 'origin_off_by_one':
            top, left = (top + 1 if top + 1 + h <= H else top - 1), (left + 1 if left + 1 + w <= W else left - 1)
            top, left = max(top, 0), max(left, 0)
        fl = flip is not None and int(flip[b])
        if fl and fault == 'flip_before_window':
            xi = Rx - 1 - (o + sx)                  # the resized image is mirrored, THEN the window is cut
        else:
            xi = (S - 1 - o if fl else o) + sx
        y0, y1, ly = _f32_axis(h, Ry, o + sy, fault)
        x0, x1, lx = _f32_axis(w, Rx, xi, fault)
        reg = frames[b, :, top:top + h, left:left + w, :].float()
        r0, r1 = reg[:, y0], reg[:, y1]
        lx, ly = lx.view(1, 1, S, 1), ly.view(1, S, 1, 1)
        v = (1 - ly) * ((1 - lx) * r0[:, :, x0] + lx * r0[:, :, x1]) + ly * ((1 - lx) * r1[:, :, x0] + lx * r1[:, :, x1])
        out[b] = ((v - m) / s).permute(3, 0, 1, 2)
    return out


# ---- the bound --------------------------------------------------------------------------------------------------------
def bound(ref64, params, std, dtype=torch.float32):
    """Elementwise bound on |out - ref64|, [B,3,F,S,S], derived in pixel units:
    a float32 coordinate differs from the exact one by at most 3 * 2^-24 * (n + 1); the interpolant is continuous in the
    coordinate with slope <= 255 per axis; the four-term sum adds at most 8 roundings of a value <= 255. So
    E_pix = 255 * 2 * 3 * 2^-24 * (n_max + 1) + 255 * 8 * 2^-24, and the output bound is E_pix / std_c + 2^-22 |ref|
    (subtraction and division), plus 2^-8 |ref| for bf16 or 2^-11 |ref| + 2^-24 for fp16 (one rounding to the format)."""
    p = torch.as_tensor(params)
    n_max = torch.maximum(p[:, 2], p[:, 3]).double().view(-1, 1, 1, 1, 1)
    e_pix = 255. * 2 * 3 * 2. ** -24 * (n_max + 1) + 255. * 8 * 2. ** -24
    s = torch.tensor(std, dtype=torch.float32).double().view(1, 3, 1, 1, 1)
    bd = e_pix / s + 2. ** -22 * ref64.abs()
    if dtype == torch.bfloat16:
        bd = bd + 2. ** -8 * ref64.abs()
    elif dtype == torch.float16:
        bd = bd + 2. ** -11 * ref64.abs() + 2. ** -24
    else:
        assert dtype == torch.float32
    return bd


def worst_ratio(out, ref64, bd):
    """max |out - ref| / bound: inside the bound iff <= 1"""
    return ((out.double() - ref64).abs() / bd).max().item()


# ---- the case table ---------------------------------------------------------------------------------------------------
def _case(name, H, W, S, blocks, flip=None, stats='openai', exact=False):
    return {'name': name, 'H': H, 'W': W, 'S': S, 'params': torch.tensor(blocks, dtype=torch.int32), 'flip': flip,
            'stats': stats, 'exact': exact}


B, FRAMES = 3, 2

# Wherever every n / R is dyadic the interpolation is exact in float32 (coordinates, weights and every partial sum fit 24
# bits): extents 48, 96, 24, 72, 36, 12 for S = 48 and 28, 56, 14, 7, 42 for S = 28, with R != S along one axis (windows
# at sy, sx != 0) too.
EXACT_CASES = [
    _case('exact48_a', 97, 131, 48, [[3, 5, 48, 96, 48, 48, 0, 0], [10, 20, 24, 72, 48, 48, 0, 0],
                                      [40, 100, 36, 12, 48, 96, 0, 17]], flip=[0, 1, 1]),
    _case('exact48_b', 97, 131, 48, [[1, 83, 96, 48, 48, 48, 0, 0], [20, 0, 72, 24, 96, 48, 31, 0],
                                      [61, 119, 36, 12, 48, 48, 0, 0]], flip=None, stats='imagenet'),
    _case('exact28_a', 97, 131, 28, [[0, 0, 28, 56, 28, 28, 0, 0], [83, 124, 14, 7, 28, 28, 0, 0],
                                      [55, 3, 42, 14, 28, 56, 0, 11]], flip=[1, 0, 1], stats='imagenet'),
    _case('exact28_b', 37, 53, 28, [[9, 39, 28, 14, 28, 28, 0, 0], [30, 11, 7, 42, 28, 28, 0, 0],
                                     [23, 25, 14, 28, 56, 28, 20, 0]], flip=[0, 0, 1]),
]

# General cases: S = 28 and 48 (never a power of two there: every ratio would be dyadic and the error zero); the S = 64
# rows exist for the 16- and 32-pixel patches of the device tests.
GENERAL_CASES = [
    _case('mixed28', 97, 131, 28, [[13, 13, 82, 102, 28, 28, 0, 0], [0, 23, 97, 102, 28, 28, 0, 0],
                                    [31, 2, 51, 67, 28, 28, 0, 0]], flip=[1, 0, 1]),
    _case('mixed48', 97, 131, 48, [[5, 40, 77, 91, 48, 48, 0, 0], [0, 0, 97, 131, 48, 48, 0, 0],
                                    [44, 17, 53, 39, 48, 48, 0, 0]], flip=[0, 1, 0], stats='imagenet'),
    # one-pixel-wide, one-pixel-high and one-pixel regions (pure upscaling along that axis)
    _case('thin28', 97, 131, 28, [[5, 7, 20, 1, 28, 28, 0, 0], [50, 60, 1, 30, 28, 28, 0, 0], [96, 130, 1, 1, 28, 28, 0, 0]],
          flip=[1, 1, 0]),
    # the last row, the last column and the bottom-right corner of the frame
    _case('edge48', 37, 53, 48, [[36, 0, 1, 53, 48, 48, 0, 0], [0, 52, 37, 1, 48, 48, 0, 0], [28, 42, 9, 11, 48, 48, 0, 0]],
          flip=[0, 1, 1], stats='imagenet'),
    _case('upscale48', 37, 53, 48, [[3, 4, 20, 25, 48, 48, 0, 0], [0, 0, 37, 53, 48, 48, 0, 0], [11, 30, 13, 17, 48, 48, 0, 0]],
          flip=[1, 0, 0]),
    # 4 : 1 along x (112 -> 28, dyadic, and 113 -> 28, not), 97 -> 28 along y
    _case('down4_28', 97, 131, 28, [[0, 10, 97, 112, 28, 28, 0, 0], [0, 18, 97, 113, 28, 28, 0, 0],
                                     [2, 0, 95, 111, 28, 28, 0, 0]], flip=[0, 1, 0]),
    # Resize(S) + CenterCrop(S): landscape 97 x 131 -> 28 x 37 window at (0, 4); one block differs (window off centre)
    _case('eval28', 97, 131, 28, [[0, 0, 97, 131, 28, 37, 0, 4], [0, 0, 97, 131, 28, 37, 0, 4], [0, 0, 97, 131, 28, 37, 0, 9]],
          flip=None, stats='imagenet'),
    _case('eval48', 37, 53, 48, [[0, 0, 37, 53, 48, 68, 0, 10], [0, 0, 37, 53, 48, 68, 0, 10], [0, 0, 37, 53, 48, 68, 0, 0]],
          flip=[0, 1, 1]),
    _case('eval48_portrait', 131, 97, 48, [[0, 0, 131, 97, 64, 48, 8, 0]] * 3, flip=None),
    _case('mixed64', 97, 131, 64, [[13, 13, 82, 102, 64, 64, 0, 0], [0, 0, 97, 131, 64, 86, 0, 11],
                                    [96, 0, 1, 131, 64, 64, 0, 0]], flip=[1, 0, 1]),
    _case('mixed64_small', 37, 53, 64, [[0, 0, 37, 53, 64, 64, 0, 0], [7, 9, 5, 1, 64, 64, 0, 0],
                                         [0, 0, 37, 53, 91, 64, 27, 0]], flip=None, stats='imagenet'),
    # a source two pixels wide: below the width at which the kernels fetch a pixel pair with one 8-byte load
    _case('narrow_source28', 37, 2, 28, [[0, 0, 37, 2, 28, 28, 0, 0], [5, 1, 20, 1, 28, 28, 0, 0], [36, 0, 1, 2, 28, 28, 0, 0]],
          flip=[0, 1, 1]),
]

CASES = {c['name']: c for c in EXACT_CASES + GENERAL_CASES}
assert len(CASES) == len(EXACT_CASES) + len(GENERAL_CASES)


@functools.lru_cache(maxsize=None)
def case_frames(name):
    """uint8 [B, F, H, W, 3], seeded per case; shared and never written to"""
    c = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    return torch.randint(0, 256, (B, FRAMES, c['H'], c['W'], 3), dtype=torch.uint8, generator=g)


@functools.lru_cache(maxsize=None)
def case_oracle(name):
    c = CASES[name]
    mean, std = MEAN_STD[c['stats']]
    return oracle64(case_frames(name), c['params'], c['flip'], c['S'], mean, std)


def case_stats(name):
    return MEAN_STD[CASES[name]['stats']]
