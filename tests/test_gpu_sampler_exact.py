"""GPU (-m gpu): lvl_sample_next_token (csrc/sampler.hip) against the float64 oracle of tests/sampler_reference.py --
the KEPT SET exactly and the DRAW exactly. The kernel returns only a token, so every case aims uniforms at the middle of
chosen entries' CDF intervals (each at least 1e-4 of the kept weight wide on either side: ten times the relative error of
the kernel's f32 sums) and asserts the very token; a dropped entry next to kept ones is probed where it WOULD sit if it
were kept. Rows are level-structured (a few bf16 values, many ties, permuted per row), top_p is solved so that the
number of boundary ties to drop is robust (sampler_reference.Case.check_margins: conditions on the inputs, checked on the
CPU in tests/test_sampler_reference_cpu.py), and each case restates the branch of the kernel it is built to reach and
asserts it from its inputs. No kernel debug output is read."""
import ctypes
import math

import numpy as np
import pytest
import torch

import sampler_reference as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
JUNK = (math.inf, math.nan, 1e4)            # what the padded columns [V, stride) hold, in turn
PER = 52                                    # entries per thread of the kernel's top-p pass


def _device_rows(rows64, extra_stride, junk):
    """[rows, V] view (bf16, on the device) of a [rows, V rounded up to 8 + extra_stride] tensor filled with `junk`."""
    rows, V = rows64.shape
    full = torch.full((rows, (V + 7) // 8 * 8 + extra_stride), junk, dtype=torch.float64)
    full[:, :V] = torch.from_numpy(rows64)
    b = full.bfloat16()
    assert torch.equal(b[:, :V].double(), full[:, :V])                      # the oracle sees what the kernel sees
    return b.to(DEV)[:, :V]


def _key(v):
    """The kernel's 16-bit key of a bf16 value, restated: values with the sign bit set take the two's complement of their
    bits (so -0 shares +0's key 0x8000: one level), the others their bits with the top bit set. Level 1 of the radix count
    is key >> 5, level 2 key & 31."""
    b = torch.tensor([v], dtype=torch.float64).bfloat16().view(torch.int16).item() & 0xffff
    return (-b & 0xffff) if b & 0x8000 else b | 0x8000


def _kth(case):
    return float(np.sort(case.sorted_row())[::-1][min(case.top_k, case.V) - 1])


def _l1_count_reaches_k_at_bucket_end(case):
    """The descending cumulative count over level-1 buckets equals top_k exactly at the bucket of the k-th value (the
    non-strict `>=` hit of find_boundary), the k-th value is the smallest key of that bucket's entries, in level-2 bucket
    0, and the next level down has level-2 bucket 31: a walk that went one bucket too far would keep it."""
    keys = np.array([_key(v) for v in case.levels])
    cnt = np.array(case.counts)
    k = _key(_kth(case))
    nxt = keys[keys < k].max()
    return cnt[keys >> 5 >= k >> 5].sum() == case.top_k and k & 31 == 0 and nxt & 31 == 31 and nxt >> 5 == (k >> 5) - 1


def _l2_count_reaches_k_exactly(case):
    """Inside the level-1 bucket of the k-th value the descending count reaches top_k exactly at its level-2 bucket (the
    `>=` of the level-2 walk), and the same level-1 bucket holds a lower level: a walk that went on would keep it."""
    keys = np.array([_key(v) for v in case.levels])
    cnt = np.array(case.counts)
    k = _key(_kth(case))
    return cnt[keys >= k].sum() == case.top_k and ((keys >> 5 == k >> 5) & (keys < k)).any()


def _nuc(case):
    x = case.sorted_row()
    v, r, cnt, xq, thr, p = R.nucleus(x, R.kept(x, case.top_k, None, case.T), case.top_p, case.T)
    return dict(v=v, r=r, cnt=cnt, vmax=v == x.max())


def _f32_weights_underflow(case, kept_too=False):
    """Most float32 weights are 0 (and, kept_too, so are some of the KEPT entries': they must never be drawn)."""
    x = case.sorted_row()
    w = np.exp(((x - x.max()) / case.T).astype(np.float32))
    return (w == 0).mean() > 0.5 and (not kept_too or (w[R.kept(x, case.top_k, case.top_p, case.T)] == 0).any())


# the branch each family is built to reach, from the inputs alone
BRANCH = {
    'k_l2_last': lambda c: _key(_kth(c)) & 31 == 31,
    'k_l2_first_l1_end': _l1_count_reaches_k_at_bucket_end,
    'k_l2_mid': lambda c: _key(_kth(c)) & 31 not in (0, 31)
    and sum(_key(v) >> 5 == _key(_kth(c)) >> 5 for v in c.levels) == 2,
    'k_l2_exact': _l2_count_reaches_k_exactly,
    'k_l2_exact_negative': lambda c: _l2_count_reaches_k_exactly(c) and all(_key(v) < 0x8000 for v in c.levels),
    'k_l1_end_negative': lambda c: _l1_count_reaches_k_at_bucket_end(c) and all(_key(v) < 0x8000 for v in c.levels),
    'k_tied_level_over_k': lambda c: c.counts[0] > c.top_k and _kth(c) == c.levels[0],
    'k_tied_level_over_k2': lambda c: c.counts[1] > c.top_k and _kth(c) == c.levels[1],
    'k_vm1_tied_min': lambda c: c.top_k == c.V - 1 and _kth(c) == c.levels[-1],
    'k330_V331': lambda c: c.top_k == c.V - 1 and _kth(c) > c.levels[-1],
    'k336_V331': lambda c: c.top_k == c.V + 5,
    'neg_k': lambda c: all(_key(v) < 0x8000 for v in c.levels) and _key(c.levels[0]) - _key(c.levels[1]) == 1,
    'neg_p': lambda c: all(_key(v) < 0x8000 for v in c.levels),
    'neg_kp': lambda c: all(_key(v) < 0x8000 for v in c.levels),
    'mix_k': lambda c: _key(0.0) == _key(-0.0) == 0x8000 and min(map(_key, c.levels)) < 0x8000 < max(map(_key, c.levels)),
    'mix_p': lambda c: _nuc(c)['v'] == 0.0,
    'mix_p_neg_boundary': lambda c: _key(_nuc(c)['v']) < 0x8000 and _nuc(c)['r'] == _nuc(c)['cnt'] - 1,
    'equal': lambda c: len(c.levels) == 1,
    'equal_k': lambda c: len(c.levels) == 1 and 1 < c.top_k < c.V,
    'equal_p_r0': lambda c: len(c.levels) == 1 and _nuc(c)['r'] == 0 and _key(c.levels[0]) < 0x8000,
    'equal_p_r1': lambda c: len(c.levels) == 1 and _nuc(c)['r'] == 1,
    'equal_p_rlast': lambda c: len(c.levels) == 1 and _nuc(c)['r'] == c.V - 1,
    'ulp_l1_edge_k': lambda c: _key(c.levels[0]) - _key(c.levels[1]) == 1 and _key(c.levels[0]) & 31 == 0,
    'ulp_l1_edge_p': lambda c: _key(c.levels[0]) - _key(c.levels[1]) == 1 and _nuc(c)['v'] == c.levels[1],
    'ulp_exponent_edge_kp': lambda c: _key(c.levels[0]) - _key(c.levels[1]) == 1 and c.levels[0] == 1.0
    and _kth(c) == _nuc(c)['v'] == c.levels[1],
    'p_r0': lambda c: _nuc(c)['r'] == 0,
    'p_r1': lambda c: _nuc(c)['r'] == 1,
    'p_rlast': lambda c: _nuc(c)['r'] == _nuc(c)['cnt'] - 1 and not _nuc(c)['vmax'],
    'p_bulk_boundary': lambda c: _nuc(c)['v'] == c.levels[-1] and _nuc(c)['r'] > 100,
    'p_max_rlast': lambda c: _nuc(c)['vmax'] and _nuc(c)['r'] == _nuc(c)['cnt'] - 1 > 0,
    'p_max_all_survive': lambda c: _nuc(c)['vmax'] and _nuc(c)['r'] == 0 and _nuc(c)['cnt'] > 1,
    # float32: 1 - top_p == 1, so thr == Z, floor((thr - below) / p) reaches cnt and only the clamp keeps the maximum
    'p_tiny_clamped': lambda c: np.float32(1) - np.float32(c.top_p) == np.float32(1) and _nuc(c)['vmax']
    and _nuc(c)['r'] == _nuc(c)['cnt'] - 1 > 0,
    'p_one': lambda c: c.top_p == 1.0,
    'p_none': lambda c: c.top_p is None and not c.top_k,
    'kp_straddle': lambda c: _kth(c) == _nuc(c)['v'] and 0 < _nuc(c)['r'] < _nuc(c)['cnt'] - 1
    and R.kept(c.sorted_row(), c.top_k, None, c.T).sum() > c.top_k,
    'kp_straddle_r0': lambda c: _kth(c) == _nuc(c)['v'] and _nuc(c)['r'] == 0,
    'kp_k_inside_p': lambda c: _kth(c) < _nuc(c)['v'],
    'k1_with_p': lambda c: c.top_k == 1 and c.counts[0] > 1,
    'T0.05_p': _f32_weights_underflow,
    'T0.05_none': lambda c: _f32_weights_underflow(c, kept_too=True),
    'T0.05_k': _f32_weights_underflow,
    'T50_p': lambda c: c.T == 50.0,
    'V53248_p': lambda c: c.V == PER * R.ST and R.chunk_of(c.V) == PER,
    'V53247_p': lambda c: c.V == PER * R.ST - 1 and c.V % 8 == 7,
    'V1025_kp': lambda c: R.chunk_of(c.V) == 2 and (c.V - 1) // 2 == 512,        # thread 512 owns one entry, the rest none
}


def _plan(case, x, v):
    """What one row is asked and what the oracle answers: [(kind, u, {acceptable tokens})]; v: the nucleus' boundary value."""
    keep = R.kept(x, case.top_k, case.top_p, case.T)
    cum = R.draw_interval(keep, x, case.T)
    plan = []
    for t in R.targets(x, keep, cum, v):
        u, half = R.u_for(t, cum)
        assert keep[t] and half >= R.HALF_WIDTH, (case.name, t, half)
        plan.append(('target', u, {t}))
    for u, t, j in R.probes(x, keep, cum, case.T):
        plan.append((f'probe of dropped {j}', u, {t}))
    rel = np.diff(np.concatenate([[0.0], cum])) / cum[-1]
    mass = np.nonzero(rel >= 1e-30)[0]                 # check_margins: the other kept weights are <= 1e-60 (0 in float32)
    plan.append(('u = 0', 0.0, {int(mass[0])}))                   # the first kept entry with nonzero mass
    # the last kept entry -- or the one float64 finds at 1 - 2^-24 when what follows it weighs less than that -- or the
    # first maximum, the documented fallback when u * (kept weight) rounds to the whole of it
    last = float(np.nextafter(np.float32(1), np.float32(0)))
    plan.append(('u = 1 - 2^-24', last, {int(mass[-1]), R.token_at(cum, last)[0], int(np.argmax(x))}))
    return keep, plan


def _ask(logits, case, plans, **kw):
    """One kernel call per plan column (row i gets its own column-c uniform; short plans repeat their first entry)."""
    from lavila_amd.narrator import sample_next_token
    cols = max(len(p) for p in plans)
    plans = [p + [p[0]] * (cols - len(p)) for p in plans]
    U = torch.tensor([[q[1] for q in p] for p in plans], dtype=torch.float64).float().to(DEV)
    got, first = [], None
    for c in range(cols):
        out = sample_next_token(logits, case.top_k, case.top_p, case.T, uniform=U[:, c].contiguous(), **kw)
        assert out is not None and out[0].shape == (len(plans), 1) and out[0].dtype == torch.int64
        first = out if first is None else first
        got.append(out[0][:, 0])
    got = torch.stack(got, 1).cpu().numpy()
    wrong = [(i, plans[i][c][0], f'u={plans[i][c][1]:.9g}', f'got {got[i, c]}', f'want {sorted(plans[i][c][2])}')
             for i in range(len(plans)) for c in range(cols) if int(got[i, c]) not in plans[i][c][2]]
    return got, wrong, first


@pytest.mark.parametrize('case', R.CASES, ids=repr)
def test_kept_set_and_draw_exact(case):
    if case.name in BRANCH:
        assert BRANCH[case.name](case), f'{case.name} does not reach the branch it is named for'
    rows64 = case.rows64()
    plans, keeps = [], []
    nuc = case.check_margins()
    for x in rows64:
        keep, plan = _plan(case, x, None if nuc is None else nuc['v'])
        keeps.append(keep)
        plans.append(plan)
    index = R.CASES.index(case)
    for junk in (JUNK if case.V <= 2048 else JUNK[index % 3:index % 3 + 1]):
        logits = _device_rows(rows64, case.extra_stride, junk)
        assert logits.stride(0) == (case.V + 7) // 8 * 8 + case.extra_stride
        got, wrong, (_, nll, cnt) = _ask(logits, case, plans)
        assert not wrong, (case.name, junk, len(wrong), wrong[:6])
        assert all(keeps[i][t] for i in range(case.rows) for t in got[i])               # nothing dropped is ever drawn
        want = torch.tensor([R.entropy(x) for x in rows64], dtype=torch.float64)
        torch.testing.assert_close(nll.double().cpu(), want, atol=2e-4, rtol=2e-4)
        assert torch.equal(cnt, torch.ones(case.rows, device=DEV))


def _explicit_rows(row):
    x = np.array(row, dtype=np.float64)
    rng = np.random.default_rng(5)
    return np.stack([x] + [x[rng.permutation(x.size)] for _ in range(7)])


@pytest.mark.parametrize('name,row,top_k,top_p,T', R.EXPLICIT, ids=[e[0] for e in R.EXPLICIT])
def test_signed_zero_and_minus_infinity_rows(name, row, top_k, top_p, T):
    """+0 and -0 are ONE level (transformers' `scores < kth`: top_k = 2 keeps five entries of the first row), and a -inf
    logit has weight 0: never drawn, and 0 log 0 = 0 in the entropy (1.4065 for the -inf row, not NaN)."""
    rows64 = _explicit_rows(row)
    case = type('Row', (), dict(name=name, V=8, top_k=top_k or 0, top_p=top_p, T=T, rows=len(rows64)))()
    v = None if top_p is None else R.nucleus(rows64[0], R.kept(rows64[0], top_k, None, T), top_p, T)[0]
    plans = [_plan(case, x, v)[1] for x in rows64]
    if name == 'signed_zero':
        assert R.kept(rows64[0], top_k, top_p, T).tolist() == [True, True, True, True, False, False, True, False]
        assert len([p for p in plans[0] if p[0] == 'target']) == 5
    for junk in JUNK:
        logits = _device_rows(rows64, 0, junk)
        if name.startswith('signed_zero'):
            assert (logits.view(torch.int16)[0, :3].cpu().int() & 0xffff).tolist() == [0, 0x8000, 0x8000]     # -0 got there
        got, wrong, (_, nll, cnt) = _ask(logits, case, plans)
        assert not wrong, (name, junk, wrong[:6])
        want = torch.tensor([R.entropy(x) for x in rows64], dtype=torch.float64)
        torch.testing.assert_close(nll.double().cpu(), want, atol=2e-4, rtol=2e-4)


def test_debug_output_changes_nothing():
    case = next(c for c in R.CASES if c.name == 'kp_straddle')
    rows64 = case.rows64()
    plans = [_plan(case, x, case.check_margins()['v'])[1] for x in rows64]
    logits = _device_rows(rows64, 0, JUNK[1])
    got, wrong, first = _ask(logits, case, plans)
    got_d, wrong_d, first_d = _ask(logits, case, plans, debug=True)
    assert not wrong and not wrong_d and np.array_equal(got, got_d)
    assert len(first_d) == 4 and all(torch.equal(a, b) for a, b in zip(first, first_d[:3]))


def _raw_call(logits, V, stride, rows, top_k, top_p, T, u, target=None, pad=-100, logits_ptr=None):
    """lvl_sample_next_token through the C ABI on result buffers with one guard element each."""
    from lavila_amd import _cabi as C
    nxt = torch.full((rows + 1,), -1, dtype=torch.int64, device=DEV)
    nll = torch.full((rows + 1,), math.nan, dtype=torch.float32, device=DEV)
    cnt = torch.full((rows + 1,), math.nan, dtype=torch.float32, device=DEV)
    rc = C.lib().lvl_sample_next_token(C.ptr(logits) if logits_ptr is None else ctypes.c_void_p(logits_ptr), stride, rows, V,
                                       T, top_k, top_p, C.ptr(u), C.ptr(target), pad, C.ptr(nxt), C.ptr(nll), C.ptr(cnt),
                                       None, C.stream_ptr())
    torch.cuda.synchronize()
    return rc, nxt, nll, cnt


@pytest.mark.parametrize('name', ['V5_kp', 'V1025_kp', 'p_rlast', 'V53248_kp'])
def test_result_buffers_are_written_up_to_rows_only(name):
    from lavila_amd.narrator import sample_next_token
    case = next(c for c in R.CASES if c.name == name)
    rows64 = case.rows64()
    logits = _device_rows(rows64, case.extra_stride, JUNK[1])
    u = torch.rand(case.rows, generator=torch.Generator().manual_seed(1)).to(DEV)
    want = sample_next_token(logits, case.top_k, case.top_p, case.T, uniform=u)
    rc, nxt, nll, cnt = _raw_call(logits, case.V, logits.stride(0), case.rows, min(case.top_k, case.V), case.top_p, case.T, u)
    assert rc == 0
    assert nxt[-1].item() == -1 and math.isnan(nll[-1].item()) and math.isnan(cnt[-1].item())
    assert torch.equal(nxt[:-1], want[0][:, 0]) and torch.equal(nll[:-1], want[1]) and torch.equal(cnt[:-1], want[2])
    for i in range(case.rows):
        assert R.kept(rows64[i], case.top_k, case.top_p, case.T)[nxt[i].item()]


def test_refusals():
    from lavila_amd import _cabi as C
    from lavila_amd.narrator import sample_next_token
    vmax = C.lib().lvl_sample_max_vocab()
    assert vmax == R.MAX_VOCAB == PER * R.ST
    V = vmax + 1
    logits = torch.zeros(2, (V + 7) // 8 * 8, dtype=torch.bfloat16, device=DEV)
    u = torch.full((2,), 0.5, device=DEV)
    assert sample_next_token(logits[:, :V], None, 0.9, 1.0, uniform=u) is None
    rc, nxt, nll, cnt = _raw_call(logits, V, logits.stride(0), 2, 0, 0.9, 1.0, u)
    assert rc == -38 and (nxt == -1).all() and torch.isnan(nll).all() and torch.isnan(cnt).all()
    rc, nxt, nll, cnt = _raw_call(logits, vmax, logits.stride(0), 2, 0, 0.9, 1.0, u)                 # the limit itself runs
    assert rc == 0 and nxt[-1].item() == -1 and (nxt[:-1] >= 0).all() and (nxt[:-1] < vmax).all()
    small = torch.zeros(4, 344, dtype=torch.bfloat16, device=DEV)
    for stride, ptr in ((340, None), (332, None), (336, small.data_ptr() + 2), (336, small.data_ptr() + 8)):
        rc, nxt, nll, cnt = _raw_call(small, 331, stride, 2, 0, 0.9, 1.0, u, logits_ptr=ptr)
        assert rc == -22 and (nxt == -1).all() and torch.isnan(nll).all(), (stride, ptr)
    assert _raw_call(small, 331, 328, 2, 0, 0.9, 1.0, u)[0] == -22                                   # stride < padded V
    rc, nxt, nll, cnt = _raw_call(small, 331, 344, 0, 0, 0.9, 1.0, u)
    assert rc == 0 and (nxt == -1).all() and torch.isnan(nll).all() and torch.isnan(cnt).all()
    assert C.lib().lvl_sample_next_token(None, 344, 0, 331, 1.0, 0, 0.9, None, None, -100, None, None, None, None,
                                         C.stream_ptr()) == 0


@pytest.mark.parametrize('name', ['p_r1', 'neg_kp', 'T0.05_none', 'V13_p', 'V53247_p'])
def test_perplexity_terms(name):
    """nll / counted against the float64 entropy and cross entropy (atol = rtol = 2e-4, the bound the suite already holds
    this output to): targets at the maximum, at the minimum, equal to pad, below 0 and beyond V - 1."""
    from lavila_amd.narrator import sample_next_token
    case = next(c for c in R.CASES if c.name == name)
    rows64 = case.rows64()
    logits = _device_rows(rows64, case.extra_stride, JUNK[0])
    u = torch.full((case.rows,), 0.5, device=DEV)
    pad = 3 % case.V
    target = []
    for i, x in enumerate(rows64):
        target.append([int(np.argmax(x)), int(np.argmin(x)), pad, case.V, -1, case.V - 1, case.V + 7][i % 7])
    _, nll, cnt = sample_next_token(logits, case.top_k, case.top_p, case.T, uniform=u)
    torch.testing.assert_close(nll.double().cpu(), torch.tensor([R.entropy(x) for x in rows64], dtype=torch.float64), atol=2e-4, rtol=2e-4)
    assert torch.equal(cnt, torch.ones_like(cnt))
    _, nll, cnt = sample_next_token(logits, case.top_k, case.top_p, case.T, target=torch.tensor(target, device=DEV),
                                    pad_id=pad, uniform=u)
    want = [R.xent(x, t, pad) for x, t in zip(rows64, target)]
    torch.testing.assert_close(nll.double().cpu(), torch.tensor([w[0] for w in want], dtype=torch.float64), atol=2e-4, rtol=2e-4)
    assert cnt.cpu().tolist() == [w[1] for w in want]
    assert {w[1] for w in want} == {0.0, 1.0}


def test_perplexity_terms_with_minus_infinity():
    """A -inf logit adds 0 to the entropy (torch.special.entr(softmax).sum() = 1.4065 for this row), and the cross entropy
    against it is +inf, as F.cross_entropy gives."""
    from lavila_amd.narrator import sample_next_token
    rows64 = _explicit_rows(R.NEG_INF[1])
    assert abs(R.entropy(rows64[0]) - 1.4065) < 1e-4
    logits = _device_rows(rows64, 8, JUNK[1])
    u = torch.full((len(rows64),), 0.5, device=DEV)
    _, nll, cnt = sample_next_token(logits, None, None, 1.0, uniform=u)
    torch.testing.assert_close(nll.double().cpu(), torch.tensor([R.entropy(x) for x in rows64], dtype=torch.float64), atol=2e-4, rtol=2e-4)
    target = [int(np.argmin(x)) if i % 2 else int(np.argmax(x)) for i, x in enumerate(rows64)]
    _, nll, cnt = sample_next_token(logits, None, None, 1.0, target=torch.tensor(target, device=DEV), uniform=u)
    want = torch.tensor([R.xent(x, t, -100)[0] for x, t in zip(rows64, target)], dtype=torch.float64)
    assert torch.isinf(want[1::2]).all() and torch.isfinite(want[::2]).all()
    torch.testing.assert_close(nll.double().cpu(), want, atol=2e-4, rtol=2e-4)
    assert torch.equal(cnt, torch.ones_like(cnt))


def test_draws_follow_the_kept_distribution():
    """20000 rows of one 64-entry, 3-level row, torch's uniforms: Pearson's chi-square of the drawn tokens against the
    oracle's renormalised kept probabilities stays under the 1 - 1e-6 quantile for (kept - 1) degrees of freedom, and no
    token outside the oracle's kept set is drawn."""
    from lavila_amd.narrator import sample_next_token
    n = 20000
    case = R.Case('dist', V=64, levels=[2.0, 1.5, 1.0], counts=[8, 16, 40], nucleus=('solve', 1, 5), T=0.8, rows=1, seed=77)
    x = case.rows64()[0]
    keep = R.kept(x, case.top_k, case.top_p, case.T)
    assert keep.sum() == 8 + 16 - 5
    cum = R.draw_interval(keep, x, case.T)
    p = np.diff(np.concatenate([[0.0], cum])) / cum[-1]
    logits = _device_rows(np.repeat(x[None], n, 0), 0, JUNK[0])
    torch.manual_seed(0)
    u = torch.rand(n, device=DEV)
    nxt, _, _ = sample_next_token(logits, case.top_k, case.top_p, case.T, uniform=u)
    obs = np.bincount(nxt[:, 0].cpu().numpy(), minlength=case.V).astype(np.float64)
    assert obs[~keep].sum() == 0
    chi2 = (((obs - n * p) ** 2)[keep] / (n * p[keep])).sum()
    assert chi2 < R.chi2_quantile_upper(1e-6, int(keep.sum()) - 1), chi2
