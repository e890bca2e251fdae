"""GPU: lvl_keymask_attn_fwd / _bwd (bidirectional attention whose keys are hidden per context by a byte mask) and the
erf GELU of lvl_act_fwd / _bwd / _inplace.

  * against the float64 restatement (tests/distilbert_reference.py): bf16 at 2^-7 of the largest magnitude (the bar of
    test_attn_rows_drop_* / test_cross_attn_rows_bwd), float32 at test_gpu_kernels.py::test_causal_attention_core's bars;
    packed-qkv strides and three tensors, the qrep = 1 row-0 form, prefix masks and masks with holes
  * hidden keys do not exist (rows scaled by +-2^40 change no bit), one-hot exactness, NULL mask == all-ones mask,
    run-to-run bit identity into NaN-prefilled outputs, the context without a visible key, the error codes

Every output buffer and the workspace are NaN-poisoned before each call."""
import ctypes
import math

import pytest
import torch

import distilbert_reference as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF = torch.bfloat16
NAN = float('nan')
F32_TOL = dict(atol=2e-4, rtol=2e-4)          # test_gpu_kernels.TOL[float32]; out: 2 x atol, gradients: 6 x atol


def _C():
    from lavila_amd import _cabi as C
    return C


def _off(t, elements):
    return ctypes.c_void_p(t.data_ptr() + elements * t.element_size())


def _rand(shape, g, dt, scale=1.0):
    """A dt-rounded random tensor: (device tensor, the same values in float64 on the CPU)."""
    t = (scale * torch.randn(*shape, generator=g)).to(dt)
    return t.to(DEV), t.double()


def _mask(contexts, Tk, kind, g):
    """uint8 [contexts, Tk]. 'prefix': visible counts drawn from {1, 15, 16, 17, Tk}; 'holes': random holes, key 0 of
    context 0 hidden, only the last key of the last context visible (where there is more than one context)."""
    m = torch.zeros(contexts, Tk, dtype=torch.uint8)
    if kind == 'prefix':
        counts = [n for n in (1, 15, 16, 17, Tk) if n <= Tk]
        for c in range(contexts):
            m[c, :counts[int(torch.randint(len(counts), (1,), generator=g))]] = 1
        return m
    m = (torch.rand(contexts, Tk, generator=g) < 0.6).to(torch.uint8)
    m[:, Tk // 2] = 1
    if Tk > 1:
        m[0, 0] = 0
    if contexts > 1:
        m[-1] = 0
        m[-1, Tk - 1] = 1
    return m


class _Problem:
    """Operands of one call in either layout. packed: qkv [contexts * Tk, 3D] (qrep == Tk), the thirds are q | k | v;
    separate: q [contexts * qrep, D], k and v [contexts, Tk, D]; row0: q is row 0 of every sample of a [contexts, Tk, D]
    tensor (qrep = 1, q_stride = Tk * D)."""

    def __init__(self, contexts, qrep, Tk, H, dt, layout, seed, scale=1.5):
        g = torch.Generator().manual_seed(seed)
        D = H * 64
        self.dims, self.dt, self.layout, self.D = (contexts, qrep, Tk, H), dt, layout, D
        if layout == 'packed':
            assert qrep == Tk
            self.qkv, x = _rand((contexts * Tk, 3 * D), g, dt, scale)
            self.q64, self.k64, self.v64 = (x[:, i * D:(i + 1) * D].reshape(contexts, Tk, D).clone() for i in range(3))
            self.strides = (3 * D, 3 * D, Tk * 3 * D)
        elif layout == 'row0':
            assert qrep == 1
            self.qfull, x = _rand((contexts, Tk, D), g, dt, scale)
            self.q64 = x[:, :1].clone()
            self.k, self.k64 = _rand((contexts, Tk, D), g, dt, scale)
            self.v, self.v64 = _rand((contexts, Tk, D), g, dt, scale)
            self.strides = (Tk * D, D, Tk * D)
        else:
            self.q, x = _rand((contexts * qrep, D), g, dt, scale)
            self.q64 = x.reshape(contexts, qrep, D)
            self.k, self.k64 = _rand((contexts, Tk, D), g, dt, scale)
            self.v, self.v64 = _rand((contexts, Tk, D), g, dt, scale)
            self.strides = (D, D, Tk * D)
        self.do, x = _rand((contexts * qrep, D), g, dt)
        self.do64 = x.reshape(contexts, qrep, D)
        self.g = g

    def pointers(self):
        D = self.D
        if self.layout == 'packed':
            return self.qkv.data_ptr(), _off(self.qkv, D), _off(self.qkv, 2 * D)
        if self.layout == 'row0':
            return self.qfull.data_ptr(), self.k.data_ptr(), self.v.data_ptr()
        return self.q.data_ptr(), self.k.data_ptr(), self.v.data_ptr()

    def run(self, mask):
        """One forward + backward through the raw entry points: (out, dq, dk, dv) on the CPU, each [contexts, rows, D]."""
        C = _C()
        contexts, qrep, Tk, H = self.dims
        D, dt = self.D, self.dt
        qs, kvs, kvc = self.strides
        qp, kp, vp = (ctypes.c_void_p(p) if isinstance(p, int) else p for p in self.pointers())
        out = torch.full((contexts * qrep, D), NAN, dtype=dt, device=DEV)
        if self.layout == 'packed':
            dqkv = torch.full((contexts * Tk, 3 * D), NAN, dtype=dt, device=DEV)
            dqp, dkp, dvp = C.ptr(dqkv), _off(dqkv, D), _off(dqkv, 2 * D)
        else:
            dq = torch.full((contexts, Tk, D) if self.layout == 'row0' else (contexts * qrep, D), NAN, dtype=dt, device=DEV)
            dk = torch.full((contexts, Tk, D), NAN, dtype=dt, device=DEV)
            dv = torch.full((contexts, Tk, D), NAN, dtype=dt, device=DEV)
            dqp, dkp, dvp = C.ptr(dq), C.ptr(dk), C.ptr(dv)
        n_ws = C.lib().lvl_workspace_floats(b'keymask_attn_bwd', contexts * qrep * H, Tk)
        assert n_ws == 2 * contexts * qrep * H
        ws = torch.full((n_ws + 64,), NAN, device=DEV)
        m = None if mask is None else mask.to(DEV).contiguous()
        code = C.dtype_code(out)
        C.check(C.lib().lvl_keymask_attn_fwd(qp, kp, vp, C.ptr(m), C.ptr(out), contexts, qrep, Tk, H, qs, kvs, kvc, Tk, code,
                                             C.stream_ptr()), 'lvl_keymask_attn_fwd')
        C.check(C.lib().lvl_keymask_attn_bwd(qp, kp, vp, C.ptr(m), C.ptr(self.do), dqp, dkp, dvp, C.ptr(ws), contexts, qrep, Tk,
                                             H, qs, kvs, kvc, Tk, code, C.stream_ptr()), 'lvl_keymask_attn_bwd')
        torch.cuda.synchronize()
        assert torch.isnan(ws[n_ws:]).all(), 'the backward wrote behind its declared workspace'
        if self.layout == 'packed':
            x = dqkv.cpu().reshape(contexts, Tk, 3 * D)
            got = (x[..., :D], x[..., D:2 * D], x[..., 2 * D:])
        elif self.layout == 'row0':
            assert torch.isnan(dq[:, 1:]).all(), 'rows of dq that the call does not address were written'
            got = (dq[:, :1].cpu(), dk.cpu(), dv.cpu())
        else:
            got = (dq.cpu().reshape(contexts, qrep, D), dk.cpu(), dv.cpu())
        return (out.cpu().reshape(contexts, qrep, D),) + tuple(t.contiguous() for t in got)

    def reference(self, mask):
        q, k, v = (t.clone().requires_grad_(True) for t in (self.q64, self.k64, self.v64))
        out = R.keymask_attention(q, k, v, mask, self.dims[3])
        out.backward(self.do64)
        return out.detach(), q.grad, k.grad, v.grad


def _check(got, want, dt, tag):
    names = ('out', 'dq', 'dk', 'dv')
    if dt == BF:
        r = [((g.double() - w).abs().max() / w.abs().max().clamp_min(1e-300)).item() for g, w in zip(got, want)]
        print(f'[keymask_attn {tag}] worst ratios ' + ' '.join(f'{n} {x:.2e}' for n, x in zip(names, r))
              + f' (bound {2.0 ** -7:.2e})')
        assert max(r) <= 2.0 ** -7, dict(zip(names, r))
    else:
        err = [(g.double() - w).abs().max().item() for g, w in zip(got, want)]
        print(f'[keymask_attn {tag}] float32 max abs error ' + ' '.join(f'{n} {x:.2e}' for n, x in zip(names, err)))
        for n, g, w, scale in zip(names, got, want, (2, 6, 6, 6)):
            torch.testing.assert_close(g.double(), w, atol=F32_TOL['atol'] * scale, rtol=F32_TOL['rtol'],
                                       msg=lambda m, n=n: f'{tag} {n}: {m}')


SHAPES = [(2, 1, 1), (3, 16, 2), (2, 17, 3), (2, 33, 2), (2, 77, 12), (1, 255, 2), (1, 256, 2), (1, 257, 1), (2, 300, 2)]


@pytest.mark.parametrize('kind', ['prefix', 'holes'])
@pytest.mark.parametrize('layout', ['packed', 'separate'])
@pytest.mark.parametrize('dt', [BF, torch.float32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('contexts,Tk,H', SHAPES)
def test_keymask_attention_against_float64(contexts, Tk, H, dt, layout, kind):
    """qrep = Tk. Two runs into NaN-prefilled buffers are bit-equal and NaN-free; hidden keys get exact zeros."""
    p = _Problem(contexts, Tk, Tk, H, dt, layout, seed=1000 + 7 * Tk + H)
    mask = _mask(contexts, Tk, kind, p.g)
    runs = [p.run(mask), p.run(mask)]
    for a, b in zip(*runs):
        assert torch.equal(a, b) and not torch.isnan(a).any()
    got = runs[0]
    hidden = mask == 0
    assert not got[2][hidden].any() and not got[3][hidden].any(), 'dk / dv rows of hidden keys must be exact zeros'
    if Tk > 1:
        assert got[3][~hidden].any()
    _check(got, p.reference(mask), dt, f'{contexts, Tk, H} {layout} {kind}')


@pytest.mark.parametrize('kind', ['prefix', 'holes', None])
@pytest.mark.parametrize('dt', [BF, torch.float32], ids=['bf16', 'f32'])
def test_keymask_attention_row0_form(dt, kind):
    """qrep = 1, q_stride = L * D: only position 0 of every sample asks (the last layer under CLIP_HF), Tk = 77."""
    contexts, Tk, H = 3, 77, 4
    p = _Problem(contexts, 1, Tk, H, dt, 'row0', seed=77)
    mask = None if kind is None else _mask(contexts, Tk, kind, p.g)
    got = p.run(mask)
    assert not any(torch.isnan(t).any() for t in got)
    _check(got, p.reference(mask), dt, f'row0 {kind}')


@pytest.mark.parametrize('layout', ['packed', 'separate'])
@pytest.mark.parametrize('dt', [BF, torch.float32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('contexts,Tk,H', [(3, 37, 2), (2, 256, 1), (2, 300, 1)])
def test_hidden_keys_do_not_exist(contexts, Tk, H, dt, layout):
    """k / v rows at hidden keys scaled by +-2^40 (finite, so the reference property 0 * x = 0 holds): out, dq and the
    dk / dv rows of visible keys equal the run with those rows zeroed bit for bit; dk / dv of hidden keys are exact zeros."""
    base = _Problem(contexts, Tk, Tk, H, dt, layout, seed=31 + Tk)
    mask = _mask(contexts, Tk, 'holes', base.g)
    hidden = (mask == 0).to(DEV)
    D = H * 64
    results = []
    for factor in (0.0, 2.0 ** 40):
        p = _Problem(contexts, Tk, Tk, H, dt, layout, seed=31 + Tk)
        sign = torch.where(torch.arange(Tk, device=DEV) % 2 == 0, factor, -factor)[None, :, None]
        if layout == 'packed':
            x = p.qkv.reshape(contexts, Tk, 3 * D)
            x[..., D:] = torch.where(hidden[..., None], (x[..., D:].float() * sign).to(dt), x[..., D:])
        else:
            for t in (p.k, p.v):
                t.copy_(torch.where(hidden[..., None], (t.float() * sign).to(dt), t))
        results.append(p.run(mask))
    zeroed, huge = results
    for name, a, b in zip(('out', 'dq', 'dk', 'dv'), zeroed, huge):
        assert torch.isfinite(b).all(), name
        assert torch.equal(a, b), f'{name} depends on the rows of hidden keys'
    assert not huge[2][mask == 0].any() and not huge[3][mask == 0].any()
    _check(zeroed, base.reference(mask), dt, f'hidden {contexts, Tk, H} {layout}')


def _pair_codes(T):
    """T distinct pairs (a, b), a < b < 64."""
    pairs = [(a, b) for a in range(64) for b in range(a + 1, 64)]
    assert T <= len(pairs)
    return torch.tensor(pairs[:T])


@pytest.mark.parametrize('B,H,T', [(2, 3, 77), (2, 2, 256)])
def test_keymask_attention_one_hot_exact(B, H, T):
    """tests/test_gpu_parity_bf16.py's _one_hot_problem with the target drawn from each SAMPLE's visible keys: q_t =
    k_target, keys are 64 (e_a + e_b) with distinct pairs, so the scaled score is 1024 on the target and <= 512 elsewhere:
    exp(-512) underflows to 0 in float32 and the softmax is exactly one-hot. v and dout hold small integers: every sum is
    exact whatever its order. out == v[target], dv == the scatter-add of dout, dq == dk == 0, by torch.equal."""
    C = _C()
    g = torch.Generator().manual_seed(11 + T)
    D = H * 64
    mask = _mask(B, T, 'holes', g)
    codes = _pair_codes(T)
    keys = torch.zeros(T, 64)
    keys[torch.arange(T), codes[:, 0]] = 64.0
    keys[torch.arange(T), codes[:, 1]] = 64.0
    target = torch.empty(B, H, T, dtype=torch.long)
    for b in range(B):
        cand = mask[b].nonzero().flatten()
        target[b] = cand[torch.randint(len(cand), (H, T), generator=g)]
    q = keys[target]                                                    # [B,H,T,64]
    k = keys[None, None].expand(B, H, T, 64)
    v = torch.randint(-4, 5, (B, H, T, 64), generator=g).float()
    dout = torch.randint(-3, 4, (B, H, T, 64), generator=g).float()
    pack = lambda x: x.permute(0, 2, 1, 3).reshape(B, T, D)             # noqa: E731
    qkv = torch.cat([pack(q), pack(k), pack(v)], -1).to(BF).to(DEV).reshape(B * T, 3 * D)
    do = pack(dout).to(BF).to(DEV).reshape(B * T, D)
    idx = target[..., None].expand(B, H, T, 64)
    out_want = pack(torch.gather(v, 2, idx))
    dv_want = pack(torch.zeros(B, H, T, 64).scatter_add_(2, idx, dout))
    out = torch.full((B * T, D), NAN, dtype=BF, device=DEV)
    dqkv = torch.full((B * T, 3 * D), NAN, dtype=BF, device=DEV)
    ws = C.workspace('keymask_attn_bwd', B * T * H, T, DEV)
    m = mask.to(DEV)
    args = (B, T, T, H, 3 * D, 3 * D, T * 3 * D, T, C.LVL_BF16, C.stream_ptr())
    C.check(C.lib().lvl_keymask_attn_fwd(C.ptr(qkv), _off(qkv, D), _off(qkv, 2 * D), C.ptr(m), C.ptr(out), *args), 'fwd')
    C.check(C.lib().lvl_keymask_attn_bwd(C.ptr(qkv), _off(qkv, D), _off(qkv, 2 * D), C.ptr(m), C.ptr(do), C.ptr(dqkv),
                                         _off(dqkv, D), _off(dqkv, 2 * D), C.ptr(ws), *args), 'bwd')
    gq = dqkv.float().cpu().reshape(B, T, 3 * D)
    assert torch.equal(out.float().cpu().reshape(B, T, D), out_want), 'forward: out[t] != v[target(t)] bit for bit'
    assert torch.equal(gq[..., 2 * D:], dv_want), 'backward: dv != scatter-add of dout over the targets'
    assert torch.count_nonzero(gq[..., :2 * D]) == 0, 'backward: dq / dk must be exactly zero for a one-hot softmax'
    assert torch.count_nonzero(dv_want[mask == 0]) == 0 and torch.count_nonzero(dv_want) > 0


@pytest.mark.parametrize('dt', [BF, torch.float32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('contexts,Tk,H', [(2, 33, 2), (1, 300, 1)])
def test_null_mask_is_the_all_ones_mask(contexts, Tk, H, dt):
    p = _Problem(contexts, Tk, Tk, H, dt, 'packed', seed=5)
    a, b = p.run(None), p.run(torch.ones(contexts, Tk, dtype=torch.uint8))
    for name, x, y in zip(('out', 'dq', 'dk', 'dv'), a, b):
        assert torch.equal(x, y) and not torch.isnan(x).any(), name
    _check(a, p.reference(None), dt, f'no mask {contexts, Tk, H}')


@pytest.mark.parametrize('dt', [BF, torch.float32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('Tk', [21, 130])
def test_context_without_a_visible_key_is_uniform(dt, Tk):
    """transformers fills hidden scores with the most negative finite value: with every key hidden all scores are equal
    and the row is uniform over the Tk keys. Finite, and at bar 1 against the restatement's uniform case."""
    contexts, H = 3, 2
    p = _Problem(contexts, Tk, Tk, H, dt, 'separate', seed=9)
    mask = _mask(contexts, Tk, 'prefix', p.g)
    mask[1] = 0
    got = p.run(mask)
    assert all(torch.isfinite(t).all() for t in got)
    want = p.reference(mask)
    mean_v = p.v64[1].mean(0, keepdim=True).expand(Tk, -1)
    assert torch.allclose(want[0][1], mean_v, atol=1e-12, rtol=0)           # the restatement's uniform case
    assert not got[1][1].any() and not got[2][1].any(), 'no gradient reaches the scores of a uniform row'
    _check(got, want, dt, f'empty context Tk={Tk}')


def test_keymask_attention_error_codes():
    """Tk = 0, misaligned pointers, bad strides and an unknown dtype return LVL_EINVAL without a launch."""
    C = _C()
    L = C.lib()
    H, Tk = 1, 8
    x = torch.full((Tk, 192), NAN, dtype=BF, device=DEV)
    out = torch.full((Tk, 64), 7.0, dtype=BF, device=DEV)
    ws = torch.zeros(64, device=DEV)
    q, k, v = C.ptr(x), _off(x, 64), _off(x, 128)

    def fwd(q=q, k=k, v=v, out=C.ptr(out), Tk=Tk, qs=192, kvs=192, dtype=C.LVL_BF16, mask=None, ms=Tk):
        return L.lvl_keymask_attn_fwd(q, k, v, mask, out, 1, max(Tk, 1) if Tk else 1, Tk, H, qs, kvs, Tk * 192, ms, dtype,
                                      C.stream_ptr())

    def bwd(dq=C.ptr(x), Tk=Tk, dtype=C.LVL_BF16, ws=C.ptr(ws)):
        return L.lvl_keymask_attn_bwd(q, k, v, None, C.ptr(out), dq, k, v, ws, 1, max(Tk, 1), Tk, H, 192, 192, Tk * 192, Tk,
                                      dtype, C.stream_ptr())
    EINVAL = -22
    assert fwd(Tk=0) == EINVAL and b'bad shape' in L.lvl_last_error()
    assert fwd(q=_off(x, 1)) == EINVAL and b'aligned' in L.lvl_last_error()
    assert fwd(out=_off(out, 3)) == EINVAL
    assert fwd(qs=196) == EINVAL and b'strides' in L.lvl_last_error()
    assert fwd(kvs=32) == EINVAL
    assert fwd(dtype=7) == EINVAL and b'dtype' in L.lvl_last_error()
    assert fwd(mask=C.ptr(ws), ms=Tk - 1) == EINVAL
    assert fwd(q=None) == EINVAL and b'null' in L.lvl_last_error()
    assert bwd(Tk=0) == EINVAL and bwd(dtype=7) == EINVAL and bwd(dq=_off(x, 2)) == EINVAL and bwd(ws=None) == EINVAL
    torch.cuda.synchronize()
    assert (out == 7.0).all() and torch.isnan(x).all(), 'a refused call launched something'
    assert L.lvl_keymask_attn_fwd(q, k, v, None, C.ptr(out), 0, 1, Tk, H, 192, 192, 0, Tk, C.LVL_BF16, C.stream_ptr()) == 0
    assert L.lvl_workspace_floats(b'keymask_attn_bwd', 0, 5) == 0


# ----------------------------------------------------------------------------------------------------------------------
# the exact (erf) GELU of DistilBERT's FFN through lvl_act_fwd / _bwd / _inplace
# ----------------------------------------------------------------------------------------------------------------------
def _gelu_erf_run(u, da):
    C = _C()
    a, du = torch.full_like(u, NAN), torch.full_like(u, NAN)
    which = C.ACT_GELU_ERF
    assert which == 2
    C.check(C.lib().lvl_act_fwd(C.ptr(u), C.ptr(a), u.numel(), which, C.dtype_code(u), C.stream_ptr()), 'lvl_act_fwd')
    C.check(C.lib().lvl_act_bwd(C.ptr(u), C.ptr(da), C.ptr(du), u.numel(), which, C.dtype_code(u), C.stream_ptr()), 'lvl_act_bwd')
    inplace = u.clone()
    C.check(C.lib().lvl_act_inplace(C.ptr(inplace), u.numel(), which, C.dtype_code(u), C.stream_ptr()), 'lvl_act_inplace')
    assert torch.equal(a, inplace)                       # the out-of-place forward is the inference kernel
    return a, du


def _gelu_erf64(u64, da64):
    u64 = u64.clone().requires_grad_(True)
    a64 = R.gelu_erf(u64)
    a64.backward(da64)
    # du = da (Phi(u) + u phi(u))
    phi = torch.exp(-0.5 * u64.detach() ** 2) / math.sqrt(2 * math.pi)
    cdf = 0.5 * (1 + torch.erf(u64.detach() / math.sqrt(2.0)))
    assert torch.allclose(u64.grad, da64 * (cdf + u64.detach() * phi), atol=1e-14, rtol=1e-12)
    return a64.detach(), u64.grad


def test_gelu_erf_bf16():
    """As tests/test_gpu_narrator_train.py::test_activation_derivatives: the same shape and 2^-7 bar."""
    g = torch.Generator().manual_seed(400)
    u, u64 = _rand((40, 3072), g, BF, 3.0)
    da, da64 = _rand((40, 3072), g, BF)
    a, du = _gelu_erf_run(u, da)
    a64, du64 = _gelu_erf64(u64, da64)
    r = [((x.double().cpu() - w).abs().max() / w.abs().max()).item() for x, w in ((a, a64), (du, du64))]
    print(f'[act gelu_erf] worst ratios forward {r[0]:.2e} derivative {r[1]:.2e} (bound {2.0 ** -7:.2e})')
    assert max(r) <= 2.0 ** -7, r
    # it is NOT gelu_new: the two differ by up to 5e-4 * |u|-ish, far above float32 round-off
    from oracle import oracle as O
    assert (O.gelu_new(u64) - a64).abs().max() > 1e-4


def test_gelu_erf_f32():
    """float32 against float64 at rtol 1e-5; atol 1e-6 covers the cancellation of 1 + erf(u / sqrt 2) in the left tail
    (|a| < 1e-3 there, erff is good to a few ulp of 1)."""
    g = torch.Generator().manual_seed(401)
    u, u64 = _rand((40, 3072), g, torch.float32, 3.0)
    da, da64 = _rand((40, 3072), g, torch.float32)
    a, du = _gelu_erf_run(u, da)
    a64, du64 = _gelu_erf64(u64, da64)
    print(f'[act gelu_erf f32] max abs error forward {(a.double().cpu() - a64).abs().max():.2e} '
          f'derivative {(du.double().cpu() - du64).abs().max():.2e}')
    torch.testing.assert_close(a.double().cpu(), a64, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(du.double().cpu(), du64, rtol=1e-5, atol=1e-6)
