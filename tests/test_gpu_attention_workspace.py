"""GPU (-m gpu): the attention kernels stay inside the workspaces the library reports (csrc/attn_internal.h: the CLS-row
workspace contract; lvl_workspace_floats, lvl_divided_attn_bwd_bias_ws) at the record counts where the contract binds: 64
partial records per (b, h) -- the cap --, 2, and the location-chunk counts on both sides of the chunk doubling of the time
kernels. Every family runs lvl_divided_attn_fwd / _bwd / _bwd_bias once on `ws` / `ws2` views of EXACTLY the reported size,
cut out of a larger tensor whose margins hold a canary, and once on workspaces eight times larger with other contents:
the canaries must be untouched and out, lse, dqkv and dbias bitwise equal between the two runs. The kernels never get
less than they ask for. Where the family writes dq column-sum partials into ws2 (the rider), the batch is raised until the
rider's rows are what sizes ws2."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MARGIN = 1 << 16            # floats on either side of an exact-size view (a multiple of 4: the view stays 16-byte aligned)
CANARY = 1234.5
SPACE, TIME = 0, 1


@contextlib.contextmanager
def stream_mode(mode):
    from lavila_amd import _cabi as C
    C.lib().lvl_debug_space_stream(mode)
    try:
        yield
    finally:
        C.lib().lvl_debug_space_stream(0)


class Guarded:
    """n floats with a canary margin on either side."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((MARGIN + n + MARGIN,), CANARY, dtype=torch.float32, device=DEV)
        self.view = self.buf[MARGIN:MARGIN + n]

    def intact(self):
        return bool((self.buf[:MARGIN] == CANARY).all() and (self.buf[MARGIN + self.n:] == CANARY).all())


def _rider_batch(mode, F, N, H, dt):
    """Smallest power-of-two batch at which the dq rider's rows size ws2 (1 if the family has none, or if that batch
    would need more than 2^29 qkv elements: F=4, N=513, H=12 would take 128 samples, its sibling N=512 gets its 64)."""
    from lavila_amd import _cabi as C
    floor = C.lib().lvl_workspace_floats(b'qkv_bias_grad', 0, H * 64)
    B = 1
    while B * (1 + F * N) * 3 * H * 64 <= 1 << 29:
        if C.lib().lvl_divided_attn_bwd_bias_ws(B, F, N, H, mode, dt) > floor:
            return B
        B *= 2
    return 1


def _run(qkv, dout, B, F, N, H, mode, exact):
    """fwd, bwd and bwd_bias on exact-size guarded workspaces, or on eight-fold ones filled with another value."""
    from lavila_amd import _cabi as C
    L = C.lib()
    T, D, dt = 1 + F * N, H * 64, C.dtype_code(qkv)
    sizes = {'fwd': L.lvl_workspace_floats(b'divided_attn_fwd', B * H, T),
             'bwd': L.lvl_workspace_floats(b'divided_attn_bwd', B * H, T),
             'ws2': L.lvl_divided_attn_bwd_bias_ws(B, F, N, H, mode, dt)}
    assert min(sizes.values()) > 0
    guards = {}

    def ws(kind):
        if exact:
            guards[kind] = Guarded(sizes[kind])
            return guards[kind].view
        return torch.full((8 * sizes[kind] + 4096,), -7.25, dtype=torch.float32, device=DEV)

    out = torch.zeros(B, T, D, dtype=qkv.dtype, device=DEV)
    lse = torch.zeros(B, H, T, dtype=torch.float32, device=DEV)
    dqkv, dqkv_b = torch.zeros_like(qkv), torch.zeros_like(qkv)
    dbias = torch.zeros(3 * D, dtype=torch.float32, device=DEV)
    st = C.stream_ptr()
    w = ws('fwd')
    C.check(L.lvl_divided_attn_fwd(C.ptr(qkv), C.ptr(out), C.ptr(lse), C.ptr(w), B, F, N, H, mode, dt, st), 'fwd')
    w = ws('bwd')
    C.check(L.lvl_divided_attn_bwd(C.ptr(qkv), C.ptr(out), C.ptr(dout), C.ptr(lse), C.ptr(dqkv), C.ptr(w), B, F, N, H,
                                   mode, dt, st), 'bwd')
    w, w2 = ws('bwd'), ws('ws2')
    C.check(L.lvl_divided_attn_bwd_bias(C.ptr(qkv), C.ptr(out), C.ptr(dout), C.ptr(lse), C.ptr(dqkv_b), C.ptr(w), None,
                                        C.ptr(dbias), C.ptr(w2), B, F, N, H, mode, dt, st), 'bwd_bias')
    torch.cuda.synchronize()
    for kind, g in guards.items():
        assert g.intact(), f'{kind}: a kernel wrote outside the {g.n} floats the library reported'
    return {'out': out, 'lse': lse, 'dqkv': dqkv, 'dqkv_bias': dqkv_b, 'dbias': dbias}


def _check(mode, F, N, H, dtype):
    from lavila_amd import _cabi as C
    dt = C.dtype_code(torch.empty(0, dtype=dtype))
    B = _rider_batch(mode, F, N, H, dt)
    g = torch.Generator(device=DEV).manual_seed(11 + F + N)
    T, D = 1 + F * N, H * 64
    qkv = torch.randn(B, T, 3 * D, generator=g, device=DEV).to(dtype)
    dout = torch.randn(B, T, D, generator=g, device=DEV).to(dtype)
    C.lib().lvl_debug_generic_attention_calls(1)
    exact = _run(qkv, dout, B, F, N, H, mode, True)
    roomy = _run(qkv, dout, B, F, N, H, mode, False)
    assert C.lib().lvl_debug_generic_attention_calls(1) == 0
    for k in exact:
        assert torch.equal(exact[k], roomy[k]), f'{k} depends on the workspace\'s size or contents'
    assert torch.equal(exact['dqkv'], exact['dqkv_bias'])
    assert bool(torch.isfinite(exact['dbias']).all()) and bool(torch.isfinite(exact['lse']).all())


SPACE_SHAPES = [(64, 16, 1), (2, 16, 1)]            # 64 records per (b, h): the cap; 2 records


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('F,N,H', SPACE_SHAPES)
def test_resident_space_kernels_stay_inside_their_workspaces(F, N, H, dtype):
    _check(SPACE, F, N, H, dtype)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('F,N,H', SPACE_SHAPES)
def test_streaming_space_kernels_stay_inside_their_workspaces(F, N, H, dtype):
    with stream_mode(1):
        _check(SPACE, F, N, H, dtype)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('N', [512, 513])           # 64 location chunks; the chunk doubles: 33
def test_register_tiled_time_kernels_stay_inside_their_workspaces(N, dtype):
    _check(TIME, 4, N, 12, dtype)


@pytest.mark.parametrize('N', [1024, 1025])         # 64 location chunks of 16; the chunk doubles: 33
def test_time_mfma_kernels_stay_inside_their_workspaces(N):
    _check(TIME, 8, N, 4, torch.bfloat16)
