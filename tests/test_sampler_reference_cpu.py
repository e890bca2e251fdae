"""CPU: the float64 oracle of tests/sampler_reference.py is right. `kept` is held to transformers' own warpers
(Temperature -> TopK -> TopP, min_tokens_to_keep=1: the recipe narrator.py:368-389 builds for num_beams=1) applied to
float64 scores, on every case tests/test_gpu_sampler_exact.py runs; the cases' margin conditions hold (they are
conditions on the inputs, so they are checked here, without a kernel); entropy / cross entropy against torch."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sampler_reference as R


def _transformers_kept(x, top_k, top_p, T):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = torch.from_numpy(np.ascontiguousarray(x)).double()
    s = s[None] if s.dim() == 1 else s
    if T is not None and T != 1.0:
        s = TemperatureLogitsWarper(float(T))(None, s)
    if top_k:
        s = TopKLogitsWarper(top_k=int(top_k), min_tokens_to_keep=1)(None, s)
    if top_p is not None and top_p < 1.0:
        s = TopPLogitsWarper(top_p=float(top_p), min_tokens_to_keep=1)(None, s)
    return (s > -math.inf).numpy()


def _hold_to_transformers(x, top_k, top_p, T, what):
    ref = _transformers_kept(x, top_k, top_p, T)[0]
    own = R.kept(x, top_k, top_p, T) & (x > -math.inf)          # a -inf logit that nothing drops is "kept" with weight 0
    if top_k and min(int(top_k), x.size) == 1:
        # documented difference: greedy decoding takes the FIRST maximum (torch.argmax); the warpers keep its ties (top-p
        # then drops some of them, which ones is the sort's business)
        assert own.sum() == 1 and int(np.argmax(own)) == int(np.argmax(x)), what
        assert ref.any() and (x[ref] == x.max()).all() and (top_p is not None or ref[own].all()), what
        return
    assert own.sum() == ref.sum(), (what, int(own.sum()), int(ref.sum()))
    differ = np.nonzero(own != ref)[0]
    assert np.unique(x[differ]).size <= 1, (what, differ, x[differ])      # which ties go is the sort's business
    if differ.size:
        assert top_p is not None and x[differ][0] == R.nucleus(x, R.kept(x, top_k, None, T), top_p, T)[0], what


@pytest.mark.parametrize('case', R.CASES, ids=repr)
def test_kept_equals_transformers_warpers(case):
    rows = case.rows64()
    for i in range(case.rows if case.V <= 2048 else 2):
        _hold_to_transformers(rows[i], case.top_k, case.top_p, case.T, (case.name, i))


@pytest.mark.parametrize('name,row,top_k,top_p,T', R.EXPLICIT, ids=[e[0] for e in R.EXPLICIT])
def test_kept_on_signed_zero_and_minus_infinity(name, row, top_k, top_p, T):
    x = np.array(row, dtype=np.float64)
    _hold_to_transformers(x, top_k, top_p, T, name)
    if top_p is not None:                     # the same margin as the generated cases
        _, _, _, xq, thr, p = R.nucleus(x, R.kept(x, top_k, None, T), top_p, T)
        assert abs(xq - round(xq)) >= 0.25 and R.SUM_REL_ERR * thr / p <= 0.05


def test_signed_zeros_are_one_level_under_top_k():
    """TopKLogitsWarper compares `scores < kth`: +0 and -0 tie, so top_k = 2 keeps five entries of this row."""
    _, row, top_k, top_p, T = R.SIGNED_ZERO
    want = np.array([1, 1, 1, 1, 0, 0, 1, 0], dtype=bool)
    assert np.array_equal(_transformers_kept(np.array(row), top_k, top_p, T)[0], want)
    assert np.array_equal(R.kept(row, top_k, top_p, T), want)


def test_margin_conditions_hold_for_every_gpu_case():
    """|x - round(x)| >= 0.25 and 1e-5 thr / p_v <= 0.05 (Case.check_margins) for every case, none excluded; every case
    has targets at least HALF_WIDTH wide, the boundary's ties among them, and the nucleus finds the r it was solved for."""
    assert {c.V for c in R.CASES} >= {1, 5, 8, 13, 331, 1024, 1025, 50257, 53247, 53248}
    assert {c.T for c in R.CASES} >= {0.05, 0.7, 1.0, 50.0}
    probed = 0
    for case in R.CASES:
        m = case.check_margins()
        rows = case.rows64()
        assert all(np.array_equal(np.sort(r), np.sort(rows[0])) for r in rows)       # one multiset: one top_p fits all
        for x in rows[:3]:
            keep = R.kept(x, case.top_k, case.top_p, case.T)
            cum = R.draw_interval(keep, x, case.T)
            tg = R.targets(x, keep, cum, None if m is None else m['v'])
            assert tg and all(keep[t] and R.u_for(t, cum)[1] >= R.HALF_WIDTH for t in tg), case.name
            if m is not None:
                ties = np.nonzero(x == m['v'])[0]
                assert (~keep[ties[:m['r']]]).all() and keep[ties[m['r']:]].all() and int(ties[m['r']]) in tg, case.name
            for u, t, j in R.probes(x, keep, cum, case.T):
                assert not keep[j] and keep[t]
                probed += 1
        if m is not None and m['r'] > 0 and m['v'] != max(case.levels):
            # some row has a kept entry whose neighbour in index order is a dropped boundary tie, and aims at it
            found = 0
            for x in rows:
                keep = R.kept(x, case.top_k, case.top_p, case.T)
                tg = R.targets(x, keep, R.draw_interval(keep, x, case.T), m['v'])
                gone = np.nonzero(~keep & (x == m['v']))[0]
                found += sum(1 for t in tg if t - 1 in gone or t + 1 in gone)
            assert found, case.name
    assert probed > 200


def test_entropy_and_cross_entropy_against_torch():
    rows = [np.array(R.NEG_INF[1]), R.CASES[0].rows64()[0], R.CASES[-1].rows64()[0]]
    for x in rows:
        t = torch.from_numpy(x)
        assert abs(R.entropy(x) - torch.special.entr(F.softmax(t, dim=0)).sum().item()) < 1e-12
        for target in (0, x.size - 1, int(np.argmax(x)), int(np.argmin(x))):
            nll, cnt = R.xent(x, target, pad=-100)
            want = F.cross_entropy(t[None], torch.tensor([target])).item()
            assert cnt == 1.0 and (nll == want or abs(nll - want) < 1e-12)
        assert R.xent(x, 3 % x.size, pad=3 % x.size) == (0.0, 0.0) and R.xent(x, x.size, pad=-100) == (0.0, 0.0)
    assert abs(R.entropy(R.NEG_INF[1]) - 1.4065) < 1e-4


def test_chi_square_quantile():
    assert abs(R.chi2_quantile_upper(1e-6, 20) - 65.42068) < 1e-4              # tabulated (scipy.stats.chi2.isf)
    assert abs(R.chi2_quantile_upper(0.05, 3) - 7.814728) < 1e-5
