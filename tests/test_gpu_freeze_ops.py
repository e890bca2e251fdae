"""GPU (-m gpu): the `needs_input_grad` matrix of the own autograd Functions (freeze_cases.py) and the column-sum token chain
with frozen ends.

Every row runs once with all inputs trainable, then with exactly one input frozen and with exactly one input trainable:

  * a frozen input has no gradient;
  * every wanted gradient and every output equals the all-trainable run's to the bit -- freezing an input may drop work, it
    must not change what the remaining work computes. Where the row says that the frozen run launches another kernel
    (`switch`), the named results are held to the float64 bound of that Function's own test
    (test_linear_layer_bf16_training_path: 3e-2 + 2e-2 |want| on bf16-rounded operands) in BOTH runs instead;
  * the launches through ops._wgrad, ops._wgrad_f32, ops.linear_tn_raw, ops.linear_tn_ragged_raw, ops.layernorm_apply_raw,
    ops.quickgelu_apply_raw and ops.vec_mat are exactly the row's: no weight-gradient GEMM for a frozen weight, no
    input-gradient GEMM for an input that wants none, no rebuild whose only reader is gone, no token product nobody reads.
"""
import pytest
import torch

import freeze_cases as FC

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _count(monkeypatch):
    from lavila_amd import ops
    counts = {}
    for fname in FC.COUNTED:
        def wrap(*a, _f=getattr(ops, fname), _n=fname, **k):
            counts[_n] = counts.get(_n, 0) + 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, fname, wrap)
    return counts


def _step(leaves, run, frozen, ups, counts):
    t = {k: v.detach().clone().requires_grad_(k not in frozen) for k, v in leaves.items()}
    counts.clear()
    outs = run(t)
    wanted = [(o, u) for o, u in zip(outs, ups) if o.requires_grad]
    assert wanted, 'no output of the run wants a gradient'
    torch.autograd.backward([o for o, _ in wanted], [u for _, u in wanted])
    torch.cuda.synchronize()
    res = {f'out{i}': o.detach() for i, o in enumerate(outs)}
    res.update({f'grad:{k}': v.grad for k, v in t.items()})
    return res, {fn: counts.get(fn, 0) for fn in FC.COUNTED}


def _switch_reference(case, leaves):
    """float64 y = x W^T + b (_LinearFn) / x W + b (_Conv1DFn) on the operands the kernels read: bf16-rounded x and W."""
    x = leaves['x'].double()
    w = leaves['weight'].bfloat16().double()
    w = w.t() if case.function == '_LinearFn' else w
    return x @ w + leaves['bias'].double()


_ROWS = [(c.name, dt) for c in FC.CASES for dt in c.dtypes]


@pytest.mark.parametrize('name,dtype', _ROWS, ids=[f'{n}-{d}' for n, d in _ROWS])
def test_needs_input_grad_matrix(name, dtype, monkeypatch):
    case = FC.BY_NAME[name]
    leaves, run = FC.build(case, dtype)
    assert tuple(leaves) == case.inputs
    counts = _count(monkeypatch)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        ups = [torch.randn(o.shape, generator=g).to(DEV, o.dtype) for o in run(leaves)]
    base, base_counts = _step(leaves, run, frozenset(), ups, counts)
    assert base_counts == FC.expected_launches(case, dtype, frozenset()), (base_counts, 'all trainable')
    for k in case.inputs:
        assert base[f'grad:{k}'] is not None and bool(torch.isfinite(base[f'grad:{k}'].float()).all()), k
        assert float(base[f'grad:{k}'].float().abs().max()) > 0, k
    for frozen in FC.patterns(case.inputs)[1:]:
        what = f'{name} {dtype}, frozen {sorted(frozen)}'
        got, got_counts = _step(leaves, run, frozen, ups, counts)
        assert got_counts == FC.expected_launches(case, dtype, frozen), (what, got_counts)
        switched = set(case.switch_results) if (frozen & set(case.switch)) else set()
        for key, want in base.items():
            if key.startswith('grad:') and key[5:] in frozen:
                assert got[key] is None, f'{what}: {key} is not None'
            elif key in switched:
                ref = _switch_reference(case, leaves)
                for which, val in (('frozen', got[key]), ('all-trainable', want)):
                    err = (val.double() - ref).abs()
                    assert bool((err <= 3e-2 + 2e-2 * ref.abs()).all()), f'{what}: {key} ({which} run) vs float64: {err.max().item()}'
            else:
                assert got[key] is not None, f'{what}: {key} is None'
                assert torch.equal(got[key], want), \
                    f'{what}: {key} differs from the all-trainable run in {int((got[key] != want).sum())} elements'


# ----------------------------------------------------------------------------------------------------------------------------------
# the column-sum token chain of SpaceTimeBlock.chain with frozen ends
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['space', 'time'])
@pytest.mark.parametrize('site', ['linear_with_token', 'residual_epilogue_then_pass'])
def test_token_chain_with_frozen_ends(mode, site, monkeypatch):
    """divided_attention(want_token=True) -> linear_with_token, and -> linear_residual_layer_norm -> add_layer_norm_pass, as
    in test_colsum_tokens_give_the_bias_gradient_without_reading_dout, with the qkv bias frozen, with the projection
    (weight and bias) frozen, and with both: frozen tensors get no gradient, every other gradient and both outputs equal
    the all-trainable run's to the bit. A frozen qkv bias ends the token's only reader; its products are still computed
    (the token itself wants a gradient as long as qkv does): the count is pinned at what the code does, see DESIGN.md."""
    from lavila_amd import ops
    B, Fr, N, H = 2, 4, 49, 4
    D, T = 64 * H, 1 + Fr * N
    g = torch.Generator().manual_seed(11)
    base = dict(qkv=(torch.randn(B, T, 3 * D, generator=g) * 1.2).to(DEV, torch.bfloat16), qbias=torch.zeros(3 * D, device=DEV),
                W=(torch.randn(D, D, generator=g) * D ** -0.5).to(DEV), pb=(0.1 * torch.randn(D, generator=g)).to(DEV),
                gam=(1 + 0.1 * torch.randn(D, generator=g)).to(DEV), bet=(0.1 * torch.randn(D, generator=g)).to(DEV),
                res=torch.randn(B, T, D, generator=g).to(DEV, torch.bfloat16),
                gam2=(1 + 0.1 * torch.randn(D, generator=g)).to(DEV), bet2=(0.1 * torch.randn(D, generator=g)).to(DEV),
                res2=torch.randn(B, T, D, generator=g).to(DEV, torch.bfloat16))
    ups = [torch.randn(B, T, D, generator=g).to(DEV, torch.bfloat16) for _ in range(3)]
    counts = _count(monkeypatch)

    def run(frozen):
        t = {k: v.detach().clone().requires_grad_(k not in frozen) for k, v in base.items()}
        counts.clear()
        o, tok = ops.divided_attention(t['qkv'], Fr, N, H, mode, bias=t['qbias'], want_token=True)
        assert tok is not None
        if site == 'linear_with_token':
            y, ty = ops.linear_with_token(o, t['W'], tok)
            assert ty is not None
            r, h = ops.add_layer_norm_pass(t['res'], y, t['pb'], t['gam'], t['bet'], 1e-6, ytoken=ty)
            outs = (r, h)
        else:
            s_, h = ops.linear_residual_layer_norm(o, t['W'], t['pb'], t['res'], t['gam'], t['bet'], 1e-6, xtoken=tok)
            r, h2 = ops.add_layer_norm_pass(t['res2'], h, None, t['gam2'], t['bet2'], 1e-6)
            outs = (s_, r, h2)
        torch.autograd.backward(list(outs), ups[:len(outs)])
        torch.cuda.synchronize()
        res = {f'out{i}': v.detach() for i, v in enumerate(outs)}
        res.update({k: v.grad for k, v in t.items()})
        return res, counts.get('vec_mat', 0), counts.get('_wgrad', 0), counts.get('linear_tn_raw', 0)

    used = set(base) - ({'gam2', 'bet2', 'res2'} if site == 'linear_with_token' else set())
    want, vm, wg, tn = run(frozenset())
    assert (vm, wg, tn) == (1, 1, 2)
    for k in used:
        assert want[k] is not None and bool(torch.isfinite(want[k].float()).all()), k
    assert float(want['qbias'][2 * D:].abs().max()) > 0
    for frozen in (frozenset(['qbias']), frozenset(['W', 'pb']), frozenset(['qbias', 'W', 'pb'])):
        got, vm_f, wg_f, tn_f = run(frozen)
        assert wg_f == int('W' not in frozen) and tn_f == 2, (sorted(frozen), wg_f, tn_f)
        assert vm_f == 1, (sorted(frozen), vm_f)
        for k, v in want.items():
            if k in frozen or k not in used and not k.startswith('out'):
                assert got[k] is None, (sorted(frozen), k)
            else:
                assert torch.equal(got[k], v), f'frozen {sorted(frozen)}: {k} differs from the all-trainable run'
