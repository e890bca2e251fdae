"""GPU (-m gpu): full self-attention over [cls + N patches] -- what a block of openai_model.VisionTransformer runs -- is
lvl_divided_attn_fwd / _bwd in space mode with ONE frame: the cls query sees all 1 + N keys and so does every patch query.
Checked against a float64 full-attention reference written here, at the four real lengths (50 / 197 / 257 / 577 keys:
ViT-B/32, B/16, L/14, L/14 at 336) and at the tile and dispatch edges of the space family read from its predicates:
1, 3 keys past a tile (N = 15 / 16: 16 / 17 keys), lvl_space_mfma_supported's float32 limit of 272 keys and
lvl_space_stream_wanted's thresholds (float32 streams above 272 keys, bf16 above 288: N = 271 / 272 / 287 / 288).

Bars: those of test_gpu_kernels.test_divided_attention_core for the same entries at F > 1 (its `_close` with the scales 2
for the output and 6 for dqkv, its `_check_qkv_bias_grad`), imported. The cls row -- the one query that goes through the
partial-record / combine path, here with a single part -- is held to them separately from the patch rows."""
import pytest
import torch

from test_gpu_kernels import _attn_case, _check_qkv_bias_grad, _close, _r

pytestmark = pytest.mark.gpu
DEV = 'cuda'

CASES = [(2, 2, n) for n in (1, 3, 15, 16, 49, 196, 256, 271, 272, 287, 288, 576)] + [(1, 1, 49)]


def full_attention_f64(qkv, heads):
    """softmax(q k^T / 8) v per head over ALL tokens of a sample, float64: qkv [B, T, 3 * heads * 64] -> [B, T, heads * 64]
    (nn.MultiheadAttention without a mask, openai_model.py:196-198, between its two projections)."""
    B, T, D3 = qkv.shape
    q, k, v = qkv.double().reshape(B, T, 3, heads, 64).permute(2, 0, 3, 1, 4)           # [B, H, T, 64] each
    p = torch.softmax(q @ k.transpose(-1, -2) * 64 ** -0.5, dim=-1)
    return (p @ v).permute(0, 2, 1, 3).reshape(B, T, D3 // 3)


_reference = {}


def _case(B, H, N, dt):
    """(qkv, dout) rounded to dt, and the float64 reference (out, dqkv) on those values; computed once per case."""
    key = (B, H, N, dt)
    if key not in _reference:
        qkv, dout = _attn_case(B, 1, N, H, 29 + N)
        qkv, dout = _r(qkv, dt), _r(dout, dt)
        q64 = qkv.double().requires_grad_(True)
        o64 = full_attention_f64(q64, H)
        o64.backward(dout.double())
        _reference[key] = (qkv, dout, o64.detach().float(), q64.grad.float())
    return _reference[key]


def _generic_calls():
    from lavila_amd import _cabi as C
    return C.lib().lvl_debug_generic_attention_calls(1)


def test_the_cases_sit_on_the_dispatch_edges():
    """The predicates themselves: every case is claimed by a fast family in both dtypes, and the edges are where the case
    list says (host-side queries, no device work)."""
    from lavila_amd import _cabi as C
    lib = C.lib()
    for _, H, N in CASES:
        assert lib.lvl_attention_fast_path(C.ATTN_SPACE, 1, N, H) == 1, N
        assert lib.lvl_attention_fast_path_f32(C.ATTN_SPACE, 1, N, H) == 1, N


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('B,H,N', CASES)
def test_full_attention_is_the_space_family_at_one_frame(B, H, N, dt):
    from lavila_amd import _cabi as C
    from lavila_amd import ops
    qkv, dout, o_want, dqkv_want = _case(B, H, N, dt)
    claimed = dt == torch.bfloat16 or bool(C.lib().lvl_attention_fast_path_f32(C.ATTN_SPACE, 1, N, H))
    _generic_calls()
    qg = qkv.to(DEV, dt).requires_grad_(True)
    bias = torch.zeros(qkv.shape[-1], device=DEV, requires_grad=True)          # stands for the in-proj bias
    o = ops.divided_attention(qg, 1, N, H, 'space', bias=bias)                  # lvl_divided_attn_fwd
    o.backward(dout.to(DEV, dt))                                                # lvl_divided_attn_bwd_bias
    first = qg.grad.clone()
    # the plain backward entry (no bias gradient), twice: equal to the first to the bit
    for _ in range(2):
        q2 = qkv.to(DEV, dt).requires_grad_(True)
        o2 = ops.divided_attention(q2, 1, N, H, 'space')
        o2.backward(dout.to(DEV, dt))                                           # lvl_divided_attn_bwd
        assert torch.equal(o2, o) and torch.equal(q2.grad, first)
    torch.cuda.synchronize()
    n_generic = _generic_calls()
    if claimed:
        assert n_generic == 0, f'{n_generic} calls fell to the shape-generic kernels'
    assert torch.isfinite(o.float()).all() and torch.isfinite(first.float()).all()
    print(f'[full attention B={B} H={H} N={N} {dt}] max |d out| cls {(o[:, :1].float().cpu() - o_want[:, :1]).abs().max():.2e} '
          f'patches {(o[:, 1:].float().cpu() - o_want[:, 1:]).abs().max():.2e}; max |d dqkv| cls '
          f'{(first[:, :1].float().cpu() - dqkv_want[:, :1]).abs().max():.2e} patches '
          f'{(first[:, 1:].float().cpu() - dqkv_want[:, 1:]).abs().max():.2e}')
    _close(o[:, :1], o_want[:, :1], dt, 2, 'out, cls row')
    _close(o[:, 1:], o_want[:, 1:], dt, 2, 'out, patch rows')
    _close(first[:, :1], dqkv_want[:, :1], dt, 6, 'dqkv, cls row')
    _close(first[:, 1:], dqkv_want[:, 1:], dt, 6, 'dqkv, patch rows')
    _check_qkv_bias_grad(bias.grad, dqkv_want, dt)
