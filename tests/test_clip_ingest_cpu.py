"""Clip ingest on the host (lavila_amd/ingest.py): the plain-torch path of ClipIngest and the F.interpolate restatement of
the reference chain against the float64 oracle with exact coordinates, the exact (dyadic) cases to the bit, four injected
faults, and the parameter blocks (RandomResizedCrop.get_params, Resize + CenterCrop, validation).

The bound (clip_ingest_reference.bound) is derived, not fitted: float32 coordinate error 3 * 2^-24 * (n + 1) times slope
255 on two axes, 8 roundings of a value <= 255, then the subtraction and the division. torch's own float32 path sits at
<= 0.23 of the pixel part of it (sources 97 x 131, S = 28 and 48, 400 random blocks)."""
import pytest
import torch
import torch.nn.functional as F

import clip_ingest_reference as R
from lavila_amd import ingest
from lavila_amd.ingest import (ClipIngest, IMAGENET_MEAN_STD, OPENAI_MEAN_STD, random_resized_crop_params,
                               resize_center_crop_params, validate_params)


def _ingest(name, dtype=torch.float32):
    c = R.CASES[name]
    mean, std = R.case_stats(name)
    return ClipIngest(c['S'], mean, std)(R.case_frames(name), c['params'], c['flip'], dtype=dtype)


def test_constants_are_the_reference_drivers_triples():
    assert (OPENAI_MEAN_STD, IMAGENET_MEAN_STD) == (R.MEAN_STD['openai'], R.MEAN_STD['imagenet'])
    assert 'antialias' in ClipIngest.__doc__.lower() and '0.11.2' in ClipIngest.__doc__


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_host_path_and_interpolate_restatement_inside_the_bound(name):
    c = R.CASES[name]
    mean, std = R.case_stats(name)
    ref = R.case_oracle(name)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        out = _ingest(name, dtype)
        assert out.dtype == dtype and tuple(out.shape) == (R.B, 3, R.FRAMES, c['S'], c['S'])
        w = R.worst_ratio(out, ref, R.bound(ref, c['params'], std, dtype))
        assert w <= 1.0, f'{name} {dtype}: ClipIngest at {w:.3f} of the bound'
    via = R.restate_interpolate(R.case_frames(name), c['params'], c['flip'], c['S'], mean, std)
    w = R.worst_ratio(via, ref, R.bound(ref, c['params'], std))
    assert w <= 1.0, f'{name}: F.interpolate chain at {w:.3f} of the bound'


@pytest.mark.parametrize('name', [c['name'] for c in R.EXACT_CASES])
def test_exact_cases_equal_interpolate_to_the_bit(name):
    c = R.CASES[name]
    mean, std = R.case_stats(name)
    via = R.restate_interpolate(R.case_frames(name), c['params'], c['flip'], c['S'], mean, std)
    assert any(int(b[4]) != c['S'] or int(b[5]) != c['S'] for b in c['params']), 'one block has R != S'
    assert torch.equal(_ingest(name), via)
    assert torch.equal(_ingest(name, torch.bfloat16), via.to(torch.bfloat16))
    assert torch.equal(_ingest(name, torch.float16), via.to(torch.float16))
    # and exact means exact: the float32 interpolation carries no error at all before the normalisation
    m = torch.tensor(mean, dtype=torch.float32).double().view(1, 3, 1, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).double().view(1, 3, 1, 1, 1)
    pix = R.case_oracle(name) * s + m
    got = (_ingest(name).double() * s + m)
    assert (got - pix).abs().max().item() < 1e-4


def test_gather_copy_without_a_fault_is_inside_the_bound():
    for name in sorted(R.CASES):
        c = R.CASES[name]
        mean, std = R.case_stats(name)
        ref = R.case_oracle(name)
        out = R.restate_gather(R.case_frames(name), c['params'], c['flip'], c['S'], mean, std)
        assert R.worst_ratio(out, ref, R.bound(ref, c['params'], std)) <= 1.0, name


@pytest.mark.parametrize('fault', R.FAULTS)
def test_injected_fault_is_rejected_by_the_bound(fault):
    # the cases in which the fault changes the arithmetic at all: a flip before the window only shows where a flipped block
    # has a window that is not centred in the resized extent
    caught = []
    for name in sorted(R.CASES):
        c = R.CASES[name]
        mean, std = R.case_stats(name)
        ref = R.case_oracle(name)
        out = R.restate_gather(R.case_frames(name), c['params'], c['flip'], c['S'], mean, std, fault=fault)
        if R.worst_ratio(out, ref, R.bound(ref, c['params'], std)) > 1.0:
            caught.append(name)
    if fault == 'flip_before_window':
        # differs from the chain exactly where a flipped block's window is not centred in the resized extent
        must = [n for n, c in R.CASES.items() if c['flip'] is not None and
                any(f and int(b[5]) - c['S'] != 2 * int(b[7]) for f, b in zip(c['flip'], c['params']))]
        assert len(must) >= 3
    elif fault == 'origin_off_by_one':
        # a region that is the whole frame has nowhere to move to
        must = [n for n, c in R.CASES.items() if any(int(b[2]) < c['H'] or int(b[3]) < c['W'] for b in c['params'])]
        assert len(must) >= len(R.CASES) - 3
    else:
        # every case has a block with n != R, where the fault moves the coordinate by a fraction of a pixel of random
        # content: tens of grey levels against a bound of 1e-3
        must = list(R.CASES)
    assert set(must) <= set(caught), (fault, sorted(set(must) - set(caught)))


# ---- parameter blocks -------------------------------------------------------------------------------------------------
def test_random_resized_crop_params_are_reproducible_and_inside_the_frame():
    H, W, S = 97, 131, 28
    a = random_resized_crop_params(64, H, W, S, generator=torch.Generator().manual_seed(5))
    b = random_resized_crop_params(64, H, W, S, generator=torch.Generator().manual_seed(5))
    c = random_resized_crop_params(64, H, W, S, generator=torch.Generator().manual_seed(6))
    assert a.dtype == torch.int32 and tuple(a.shape) == (64, 8)
    assert torch.equal(a, b) and not torch.equal(a, c)
    validate_params(a, 64, H, W, S)
    scale, ratio = (0.5, 1.0), (3 / 4, 4 / 3)
    for top, left, h, w, Ry, Rx, sy, sx in a.tolist():
        assert (Ry, Rx, sy, sx) == (S, S, 0, 0)
        assert 0 <= top and top + h <= H and 0 <= left and left + w <= W and h >= 1 and w >= 1
        # w = round(sqrt(area * ar)), h = round(sqrt(area / ar)): each within 1/2 of its real value, so the real rectangle
        # (w', h') with |w' - w| <= 1/2, |h' - h| <= 1/2 has its area in `scale` and its aspect in `ratio`
        lo_area, hi_area = (w - .5) * (h - .5), (w + .5) * (h + .5)
        assert hi_area >= scale[0] * H * W and lo_area <= scale[1] * H * W
        assert (w + .5) / (h - .5) >= ratio[0] and (w - .5) / (h + .5) <= ratio[1]
    assert len({tuple(r) for r in a.tolist()}) > 32          # one draw per clip, not one per batch


def test_random_resized_crop_params_take_the_central_fallback():
    # 8 x 400: an area of at least half the frame needs w = sqrt(1600 * ar) >= 34 rows of height -- no attempt fits
    p = random_resized_crop_params(5, 8, 400, 28, generator=torch.Generator().manual_seed(0))
    assert p.tolist() == [[0, (400 - 11) // 2, 8, 11, 28, 28, 0, 0]] * 5          # h = H, w = round(8 * 4/3)
    p = random_resized_crop_params(2, 400, 8, 28, generator=torch.Generator().manual_seed(0))
    assert p.tolist() == [[(400 - 11) // 2, 0, 11, 8, 28, 28, 0, 0]] * 2          # w = W, h = round(8 / (3/4))
    validate_params(p, 2, 400, 8, 28)


@pytest.mark.parametrize('H,W', [(97, 131), (131, 97), (77, 77), (37, 53)])
def test_resize_center_crop_params_match_resize_then_center_crop(H, W):
    S = 28
    p = resize_center_crop_params(2, H, W, S)
    top, left, h, w, Ry, Rx, sy, sx = p[0].tolist()
    assert (top, left, h, w) == (0, 0, H, W) and min(Ry, Rx) == S
    long, short = max(H, W), min(H, W)
    assert max(Ry, Rx) == int(S * long / short) and (Ry >= Rx) == (H >= W)
    assert (sy, sx) == (int(round((Ry - S) / 2.0)), int(round((Rx - S) / 2.0)))
    g = torch.Generator().manual_seed(H * 1000 + W)
    frames = torch.randint(0, 256, (2, 2, H, W, 3), dtype=torch.uint8, generator=g)
    mean, std = IMAGENET_MEAN_STD
    out = ClipIngest(S, mean, std)(frames, p)
    m, s = torch.tensor(mean).view(3, 1, 1, 1), torch.tensor(std).view(3, 1, 1, 1)
    want = torch.stack([(F.interpolate(frames[b].permute(3, 0, 1, 2).float(), size=(Ry, Rx), mode='bilinear',
                                       align_corners=False)[..., sy:sy + S, sx:sx + S] - m) / s for b in range(2)])
    ref = R.oracle64(frames, p, None, S, mean, std)
    bd = R.bound(ref, p, std)
    assert R.worst_ratio(want, ref, bd) <= 1.0 and R.worst_ratio(out, ref, bd) <= 1.0
    # index for index: moving the window by one pixel is far outside the bound
    if Ry > S or Rx > S:
        col, off, ext = (6, sy, Ry) if Ry > S else (7, sx, Rx)
        shifted = p.clone()
        shifted[:, col] = off + 1 if off + 1 + S <= ext else off - 1
        assert R.worst_ratio(ClipIngest(S, mean, std)(frames, shifted), ref, bd) > 1.0


def test_default_params_are_the_whole_frame():
    frames = R.case_frames('mixed28')
    ci = ClipIngest(28)
    assert torch.equal(ci(frames), ci(frames, torch.tensor([[0, 0, 97, 131, 28, 28, 0, 0]] * 3)))


@pytest.mark.parametrize('block,what', [
    ([0, 0, 0, 10, 28, 28, 0, 0], 'at least 1'), ([0, 0, 10, 0, 28, 28, 0, 0], 'at least 1'),
    ([0, 0, 10, 10, 0, 28, 0, 0], 'at least 1'), ([0, 0, 10, 10, 28, 0, 0, 0], 'at least 1'),
    ([-1, 0, 10, 10, 28, 28, 0, 0], 'leaves the 37 x 53 frame'), ([0, -1, 10, 10, 28, 28, 0, 0], 'leaves the 37 x 53 frame'),
    ([30, 0, 8, 10, 28, 28, 0, 0], 'leaves the 37 x 53 frame'), ([0, 50, 10, 4, 28, 28, 0, 0], 'leaves the 37 x 53 frame'),
    ([0, 0, 10, 10, 27, 28, 0, 0], 'window leaves'), ([0, 0, 10, 10, 28, 30, 0, 3], 'window leaves'),
    ([0, 0, 10, 10, 30, 28, -1, 0], 'window leaves'), ([0, 0, 10, 10, 40, 28, 13, 0], 'window leaves'),
])
def test_block_validation_rejects_malformed_blocks(block, what):
    good = [0, 0, 37, 53, 28, 28, 0, 0]
    frames = torch.zeros(2, 1, 37, 53, 3, dtype=torch.uint8)
    ci = ClipIngest(28)
    ci(frames, torch.tensor([good, good]))
    with pytest.raises(ValueError, match=what) as e:
        ci(frames, torch.tensor([good, block]))
    assert 'block 1' in str(e.value)
    with pytest.raises(ValueError, match=what):
        ci.pending(frames, torch.tensor([good, block]))


def test_argument_shapes_are_checked():
    ci = ClipIngest(28)
    good = torch.zeros(2, 1, 37, 53, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match='uint8'):
        ci(good.float())
    with pytest.raises(ValueError, match='uint8'):
        ci(good.permute(0, 4, 1, 2, 3))
    with pytest.raises(ValueError, match=r'\(2, 8\)'):
        ci(good, torch.zeros(3, 8, dtype=torch.int32))
    with pytest.raises(ValueError, match='flip'):
        ci(good, None, flip=[1, 0, 1])
    with pytest.raises(ValueError, match='even'):
        ClipIngest(27)


def test_pending_clip_answers_like_the_clip_and_materialises_nothing():
    c = R.CASES['mixed28']
    frames = R.case_frames('mixed28')
    ci = ClipIngest(28, *R.case_stats('mixed28'))
    pc = ci.pending(frames, c['params'], c['flip'])
    assert isinstance(pc, ingest.PendingClip)
    assert tuple(pc.shape) == (3, 3, 2, 28, 28) and pc.ndim == 5 and pc.dim() == 5
    assert pc.device == frames.device and pc.is_cuda is False and pc.dtype == torch.float32
    assert pc.frames is frames
    assert torch.equal(pc.materialize(), ci(frames, c['params'], c['flip']))
    assert torch.equal(pc.materialize(torch.bfloat16), ci(frames, c['params'], c['flip'], dtype=torch.bfloat16))


def test_host_pending_clip_is_refused_by_the_model_entry_points():
    """no CPU fallback: the message is require_device's; frame-major entry points and the graphed step say `materialize`"""
    from lavila_amd import _cabi, ops
    from lavila_amd.graph_step import GraphedTrainStep
    pc = ClipIngest(28).pending(torch.zeros(1, 2, 37, 53, 3, dtype=torch.uint8))
    with pytest.raises(_cabi.HipExtensionError, match='need a ROCm device tensor'):
        ops.patchify(pc, 14, torch.float32)
    with pytest.raises(TypeError, match='materialize'):
        ops.patchify(pc, 14, torch.float32, frame_major=True)
    with pytest.raises(TypeError, match='materialize'):
        GraphedTrainStep.__call__(None, pc, None)
