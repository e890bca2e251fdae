"""lvl_clip_ingest / lvl_clip_ingest_patches through the raw C ABI against the float64 oracle, the host restatement and
lvl_patchify (clip_ingest_reference.py holds the oracle, the bound and the case table).

Sources are 37 x 53 and 97 x 131: odd widths, so rows are not 4-byte aligned. B = 3, F = 2, S in {28, 48, 64},
P in {14, 16, 32} (and 12: the 4-pixel store path)."""
import functools

import pytest
import torch

import clip_ingest_reference as R

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
# kIngestMaxBlocks * kIngestBlock of csrc/clip_ingest.hip: the launchers cap the grid at 8192 workgroups of 256 threads;
# a launch with more items than that walks the rest with a grid stride
GRID_CAP_THREADS = 8192 * 256
EINVAL = -22


def _C():
    from lavila_amd import _cabi
    return _cabi


def _code(dtype):
    C = _C()
    return {torch.float32: C.LVL_F32, torch.bfloat16: C.LVL_BF16, torch.float16: C.LVL_F16}[dtype]


def _dev(t):
    return None if t is None else torch.as_tensor(t, dtype=torch.int32).cuda()


def _strides(frames):
    return frames.stride(0), frames.stride(1), frames.stride(2)


def clip_launch(frames, params, flip, S, stats, dtype, strides=None, guard=64, check=True):
    """frames: device u8 [B,F,H,W,3] view (any clip / frame / row strides). The output is NaN-filled with `guard` elements
    of NaN on both sides, which have to come back untouched."""
    C = _C()
    B, Fr, H, W, _ = frames.shape
    mean, std = stats
    n = B * 3 * Fr * S * S
    buf = torch.full((n + 2 * guard,), float('nan'), dtype=dtype, device='cuda')
    out = buf[guard:guard + n]
    rc = C.lib().lvl_clip_ingest(C.ptr(frames), C.ptr(params), C.ptr(flip), C.ptr(out), B, Fr, H, W, S,
                                 *(strides or _strides(frames)), *mean, *std, _code(dtype), C.stream_ptr())
    if not check:
        return rc, buf
    C.check(rc, 'lvl_clip_ingest')
    assert bool(buf[:guard].isnan().all()) and bool(buf[guard + n:].isnan().all()), 'wrote outside the clip'
    return out.view(B, 3, Fr, S, S)


def patches_launch(frames, params, flip, S, P, ld, stats, dtype, strides=None, guard_rows=4, check=True):
    C = _C()
    B, Fr, H, W, _ = frames.shape
    mean, std = stats
    rows = B * Fr * (S // P) ** 2
    buf = torch.full((rows + 2 * guard_rows, ld), float('nan'), dtype=dtype, device='cuda')
    out = buf[guard_rows:guard_rows + rows]
    rc = C.lib().lvl_clip_ingest_patches(C.ptr(frames), C.ptr(params), C.ptr(flip), C.ptr(out), B, Fr, H, W, S, P, ld,
                                         *(strides or _strides(frames)), *mean, *std, _code(dtype), C.stream_ptr())
    if not check:
        return rc, buf
    C.check(rc, 'lvl_clip_ingest_patches')
    assert bool(buf[:guard_rows].isnan().all()) and bool(buf[guard_rows + rows:].isnan().all()), 'wrote into the guard rows'
    return out


def patchify_launch(clip, P, dtype):
    C = _C()
    B, Ch, Fr, H, W = clip.shape
    out = torch.full((B * Fr * (H // P) * (W // P), Ch * P * P), float('nan'), dtype=dtype, device='cuda')
    C.check(C.lib().lvl_patchify(C.ptr(clip), C.ptr(out), B, Ch, Fr, H, W, P, 0, _code(dtype), C.stream_ptr()), 'lvl_patchify')
    return out


@functools.lru_cache(maxsize=None)
def _device_case(name):
    c = R.CASES[name]
    return R.case_frames(name).cuda(), _dev(c['params']), _dev(c['flip'])


@functools.lru_cache(maxsize=None)
def _host_clip(name):
    """the host restatement (lavila_amd.ingest on CPU frames), float32; shared, never written to"""
    from lavila_amd.ingest import ClipIngest
    c = R.CASES[name]
    return ClipIngest(c['S'], *R.case_stats(name))(R.case_frames(name), c['params'], c['flip'])


def _gpu_clip(name, dtype):
    frames, params, flip = _device_case(name)
    return clip_launch(frames, params, flip, R.CASES[name]['S'], R.case_stats(name), dtype)


@pytest.mark.parametrize('name', [c['name'] for c in R.EXACT_CASES])
def test_exact_cases_equal_the_host_restatement_to_the_bit(name):
    want = _host_clip(name)
    for dtype in DTYPES:
        assert torch.equal(_gpu_clip(name, dtype).cpu(), want.to(dtype)), dtype


@pytest.mark.parametrize('name', [c['name'] for c in R.GENERAL_CASES])
def test_general_cases_inside_the_bound(name):
    """one-pixel-wide / -high regions, the last row and column, upscaling, 4:1 downscaling, a block and a flip per sample,
    null flip: the case table. The worst ratio to the bound is printed before it is asserted."""
    c = R.CASES[name]
    ref = R.case_oracle(name)
    for dtype in DTYPES:
        out = _gpu_clip(name, dtype).cpu()
        w = R.worst_ratio(out, ref, R.bound(ref, c['params'], R.case_stats(name)[1], dtype))
        print(f'{name} {dtype}: {w:.4f} of the bound')
        assert w <= 1.0, (name, dtype, w)


@pytest.mark.parametrize('name', [c['name'] for c in R.GENERAL_CASES])
def test_general_cases_equal_the_host_restatement_to_the_bit(name):
    """Host and device run the same float32 operations in the same order, each rounded on its own (the kernel file is
    compiled without contraction): not only the dyadic cases agree."""
    want = _host_clip(name)
    for dtype in DTYPES:
        got = _gpu_clip(name, dtype).cpu()
        bad = int((got != want.to(dtype)).sum())
        assert bad == 0, f'{name} {dtype}: {bad} of {got.numel()} elements differ'


def _strided_source(name, fill):
    """The case's frames laid out with gaps between rows, frames and clips (odd strides); every byte that no region covers --
    gaps included -- holds `fill`."""
    c = R.CASES[name]
    H, W = c['H'], c['W']
    rs = 3 * W + 5
    fs = H * rs + 7
    cs = R.FRAMES * fs + 11
    buf = torch.full((R.B * cs + 64,), fill, dtype=torch.uint8)
    view = buf.as_strided((R.B, R.FRAMES, H, W, 3), (cs, fs, rs, 3, 1), 1)          # the first pixel at an odd address
    src = R.case_frames(name)
    for b, (top, left, h, w, *_) in enumerate(c['params'].tolist()):
        view[b, :, top:top + h, left:left + w] = src[b, :, top:top + h, left:left + w]
    dev = buf.cuda()
    return dev.as_strided((R.B, R.FRAMES, H, W, 3), (cs, fs, rs, 3, 1), 1), (cs, fs, rs)


@pytest.mark.parametrize('name', ['mixed28', 'thin28', 'edge48', 'exact48_a', 'eval48', 'mixed64'])
def test_nothing_outside_the_region_is_read(name):
    c = R.CASES[name]
    _, params, flip = _device_case(name)
    P = {28: 14, 48: 16, 64: 32}[c['S']]
    outs = []
    for fill in (0x00, 0xFF):
        frames, strides = _strided_source(name, fill)
        outs.append((clip_launch(frames, params, flip, c['S'], R.case_stats(name), torch.float32, strides=strides),
                     patches_launch(frames, params, flip, c['S'], P, 3 * P * P, R.case_stats(name), torch.float32,
                                    strides=strides)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # and the strided launch computes what the contiguous one does
    assert torch.equal(outs[0][0], _gpu_clip(name, torch.float32))


def _patch_sizes(S):
    return {28: (14, 2), 48: (16, 12), 64: (16, 32)}[S]          # 14: one thread per patch row, 2: 2-pixel threads, 12: 4-pixel, 16 / 32: 8-pixel


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_patches_equal_patchify_of_the_float32_clip(name):
    c = R.CASES[name]
    frames, params, flip = _device_case(name)
    clip = _gpu_clip(name, torch.float32).contiguous()
    for P in _patch_sizes(c['S']):
        k = 3 * P * P
        for dtype in (torch.float32, torch.bfloat16):
            want = patchify_launch(clip, P, dtype)
            assert not bool(want.isnan().any())
            for ld in (k, (k // 64 + 1) * 64):
                got = patches_launch(frames, params, flip, c['S'], P, ld, R.case_stats(name), dtype)
                assert torch.equal(got[:, :k], want), (name, P, dtype, ld)
                assert ld == k or bool((got[:, k:] == 0).all()), 'pad columns are written as zeros'


def test_launches_past_the_grid_cap():
    """B = 1, F = 4100, S = 64: 4100 * 64 * 64 / 8 = 2,099,200 eight-pixel items, more than the 2,097,152 threads of the
    capped grid. The items past the cap are those of the last frames; S = 64 is dyadic, so the host restatement is exact."""
    from lavila_amd.ingest import ClipIngest
    Fr, H, W, S, P = 4100, 37, 53, 64, 16
    assert Fr * S * S // 8 > GRID_CAP_THREADS
    g = torch.Generator().manual_seed(77)
    few = torch.randint(0, 256, (1, 5, H, W, 3), dtype=torch.uint8, generator=g)
    pick = torch.arange(Fr) % 5
    frames = few[:, pick].contiguous()
    block = torch.tensor([[3, 2, 31, 50, 64, 80, 0, 13]], dtype=torch.int32)
    flip = torch.tensor([1], dtype=torch.int32)
    stats = R.MEAN_STD['openai']
    want5 = ClipIngest(S, *stats)(few, block, flip)                       # [1,3,5,S,S]
    clip = clip_launch(frames.cuda(), block.cuda(), flip.cuda(), S, stats, torch.float32)
    assert torch.equal(clip.cpu(), want5[:, :, pick])
    got = patches_launch(frames.cuda(), block.cuda(), flip.cuda(), S, P, 832, stats, torch.float32)
    want = patchify_launch(clip.contiguous(), P, torch.float32)
    assert torch.equal(got[:, :768], want) and bool((got[:, 768:] == 0).all())


def test_second_clip_more_than_2_31_bytes_into_the_source():
    name = 'mixed28'
    c = R.CASES[name]
    src = R.case_frames(name)[:2]
    H, W = c['H'], c['W']
    rs, fs = 3 * W, 3 * W * H
    cs = (1 << 31) + 4099
    buf = torch.zeros(cs + R.FRAMES * fs, dtype=torch.uint8, device='cuda')
    buf[:R.FRAMES * fs] = src[0].reshape(-1).cuda()
    buf[cs:] = src[1].reshape(-1).cuda()
    params, flip = _dev(c['params'][:2]), _dev(c['flip'][:2])
    frames = buf.as_strided((2, R.FRAMES, H, W, 3), (cs, fs, rs, 3, 1))
    clip = clip_launch(frames, params, flip, 28, R.case_stats(name), torch.float32, strides=(cs, fs, rs))
    pat = patches_launch(frames, params, flip, 28, 14, 640, R.case_stats(name), torch.bfloat16, strides=(cs, fs, rs))
    near = src.cuda()
    assert torch.equal(clip, clip_launch(near, params, flip, 28, R.case_stats(name), torch.float32))
    assert torch.equal(pat, patches_launch(near, params, flip, 28, 14, 640, R.case_stats(name), torch.bfloat16))
    assert torch.equal(clip.cpu(), _host_clip(name)[:2])
    del buf, frames
    torch.cuda.empty_cache()


@pytest.mark.parametrize('entry', ['clip', 'patches'])
def test_entry_points_capture_as_one_kernel_node(entry):
    from lavila_amd.graph_step import graph_node_types
    C = _C()
    name = 'mixed28'
    frames, params, flip = _device_case(name)
    mean, std = R.case_stats(name)
    B, Fr, H, W, _ = frames.shape
    if entry == 'clip':
        out = torch.full((B, 3, Fr, 28, 28), float('nan'), device='cuda')

        def run():
            C.check(C.lib().lvl_clip_ingest(C.ptr(frames), C.ptr(params), C.ptr(flip), C.ptr(out), B, Fr, H, W, 28,
                                            *_strides(frames), *mean, *std, C.LVL_F32, C.stream_ptr()), 'lvl_clip_ingest')
        eager = _gpu_clip(name, torch.float32)
    else:
        out = torch.full((B * Fr * 4, 640), float('nan'), dtype=torch.bfloat16, device='cuda')

        def run():
            C.check(C.lib().lvl_clip_ingest_patches(C.ptr(frames), C.ptr(params), C.ptr(flip), C.ptr(out), B, Fr, H, W, 28,
                                                    14, 640, *_strides(frames), *mean, *std, C.LVL_BF16, C.stream_ptr()),
                    'lvl_clip_ingest_patches')
        eager = patches_launch(frames, params, flip, 28, 14, 640, (mean, std), torch.bfloat16)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        run()
    assert graph_node_types(graph) == {'kernel': 1}
    assert bool(out.isnan().all()), 'capture must not run the kernel'
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.reshape(eager.shape), eager)


def test_library_refusals_launch_nothing():
    C = _C()
    name = 'mixed28'
    frames, params, flip = _device_case(name)
    stats = R.case_stats(name)
    cs, fs, rs = _strides(frames)

    def refused(rc, buf, what):
        assert rc == EINVAL, (what, rc)
        assert what in C.lib().lvl_last_error().decode(), (what, C.lib().lvl_last_error())
        torch.cuda.synchronize()
        assert bool(buf.isnan().all()), what

    refused(*patches_launch(frames, params, flip, 28, 16, 768, stats, torch.float32, check=False), 'multiple')   # S % P
    refused(*patches_launch(frames, params, flip, 28, 7, 147, stats, torch.float32, check=False), 'multiple')    # odd P
    refused(*patches_launch(frames, params, flip, 28, 14, 586, stats, torch.float32, check=False), 'ld=')        # ld < 3PP
    refused(*patches_launch(frames, params, flip, 28, 14, 589, stats, torch.float32, check=False), 'ld=')        # odd ld
    refused(*patches_launch(frames, params, flip, 28, 14, 588, stats, torch.float16, check=False), 'dtype')
    refused(*clip_launch(frames, params, flip, 27, stats, torch.float32, check=False), 'S even')
    refused(*clip_launch(frames, params, flip, 28, stats, torch.float32, strides=(cs, fs, rs - 1), check=False), 'strides')
    refused(*clip_launch(frames, params, flip, 28, stats, torch.float32, strides=(cs, fs - 1, rs), check=False), 'strides')
    refused(*clip_launch(frames, params, flip, 28, stats, torch.float32, strides=(cs - 1, fs, rs), check=False), 'strides')
    refused(*clip_launch(frames, params, flip, 28, (stats[0], (1.0, 0.0, 1.0)), torch.float32, check=False), 'std')
    refused(*clip_launch(frames, None, flip, 28, stats, torch.float32, check=False), 'null')
