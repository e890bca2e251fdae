"""CPU: the shifted-row attention cases of attention_shift_cases.py -- their preconditions, the float32 kernel model
inside the derived bound on every case the GPU file uses, and the four faults the bound must reject.

Three preconditions are asked only where they can hold:
  * the whole palette (and with it rows of lse > +89 and lse < -89) of cases with at least 11 query rows: cls-only cases have
    B * H = 4 rows, rows attention with qrep = 1, 3, 4 has fewer than 11 per head;
  * lse < -89 under a RISING staircase only where some group tops out at 16 or less: +4 per 16 keys lifts every row of a
    larger group above -89, and the stair 0 and -4 cases of the same shape hold the low end;
  * the running maximum moves in at least nk / 16 - 1 key tiles under stair +4; under stair -4 it is the opposite property
    that matters (the first 64-key tile holds every row maximum) and that is what is asserted."""
import math

import pytest
import torch

import attention_shift_cases as SC

CASES = [(k, s, dt, st) for k, s, dt in SC.all_cases() for st in SC.STAIRS]
_id = lambda v: str(v).replace(' ', '').replace('torch.', '')          # noqa: E731


def _first_block(case):
    qidx, kidx, causal = case.blocks[0]
    return qidx, kidx, causal


def _scores(case, qidx, kidx, causal):
    """Reference scores of a block [B, H, G, nq, nk], -inf where the row does not see the key."""
    s = case.q[:, :, qidx] @ case.k[:, :, kidx].transpose(-1, -2) * SC.SCALE
    if causal:
        s = s.masked_fill(torch.ones(s.shape[-2:], dtype=torch.bool).triu(1), -math.inf)
    if case.vis is not None:
        s = s.masked_fill(~case.vis[:, kidx][:, None, :, None, :], -math.inf)
    return s


@pytest.mark.parametrize('kind,shape,dt,stair', CASES, ids=_id)
def test_case_preconditions_and_emulation_inside_bound(kind, shape, dt, stair):
    case = SC.make(kind, shape, dt, stair)
    # inputs representable; float32 cases: q and k bf16-exact
    for x in (case.q, case.k, case.v, case.dO):
        assert torch.equal(x.to(dt).double(), x)
    for x in (case.q, case.k):
        assert torch.equal(x.to(torch.bfloat16).double(), x)
    rows = case.query_rows()
    # every 16-row query tile of a group with at least 16 queries holds the whole palette
    for qidx, _, _ in case.blocks:
        for t in range(0, qidx.shape[1] - 15, 16):
            c = case.q[:, :, qidx[:, t:t + 16], 63]                                               # [B, H, G, 16]
            assert all(len(set(r.tolist())) == len(SC.PAL) for r in c.reshape(-1, 16)), 'a 16-row tile misses an entry'
    # rows far below and far above zero (the overflow masks see nothing otherwise)
    lse = case.ref['lse'][:, :, rows]
    shifts = set(case.q[:, :, rows, 63].reshape(-1).tolist())
    assert shifts == SC.row_shifts(kind, shape)
    assert len(rows) < 11 or shifts == set(SC.PAL), 'a case with 11 or more query rows misses a palette entry'
    if max(shifts) >= 96:
        assert lse.max() > 89
    # a rising staircase lifts every row by its top step: where no group tops out at 16 or less (more than 80 keys; more than
    # 4 frames of a time group) no row need stay below -89, and stairs 0 and -4 cover the low end of that shape
    fewest = min(1 if causal else kidx.shape[1] for _, kidx, causal in case.blocks)
    if min(shifts) == -120 and (stair <= 0 or stair * SC._step(kind, fewest - 1) <= 16):
        assert lse.min() < -89, f'no row with lse < -89 (min {lse.min().item()})'
    # the running maximum over 16-key tiles
    qidx, kidx, causal = _first_block(case)
    s = _scores(case, qidx, kidx, causal)
    nk = kidx.shape[1]
    if stair > 0 and kind != 'time':
        tiles = torch.stack([s[..., t:t + 16].max(-1).values for t in range(0, nk, 16)], -1)      # [B,H,G,nq,tiles]
        run = torch.cummax(tiles, -1).values
        changes = (run[..., 1:] > run[..., :-1]).sum(-1)
        seen = nk if case.vis is None else int(case.vis.sum(-1).max())                # most keys a row sees
        assert changes.max().item() >= seen // 16 - 1, f'the maximum moves in {changes.max().item()} of {seen // 16} tiles'
    if stair < 0 and nk > 64 and case.vis is None:
        assert bool((s.argmax(-1) < 64).all()), 'with stair -4 the first 64-key tile must hold every row maximum'
    if kind == 'keymask' and shape[3] == SC.HIDE_LOUD:
        hid = ~case.vis[:, None, None, :].expand(s.shape[0], s.shape[1], s.shape[3], nk)
        raw = (case.q @ case.k.transpose(-1, -2) * SC.SCALE)
        some = case.vis.any(-1)
        top_vis = raw.masked_fill(hid, -math.inf).max(-1).values[some]
        low_hid = raw.masked_fill(~hid, math.inf).min(-1).values[some]
        assert bool((low_hid > top_vis).all()), 'a hidden key does not outscore every visible key of its context'
        for n in ('dk', 'dv'):
            assert not case.ref[n].permute(0, 2, 1, 3)[~case.vis].any(), 'the reference gives a hidden key a gradient'
    # the kernel model stays inside the bound
    r = SC.ratios(case, SC.emulate(case))
    print(' '.join(f'{n} {x:.3f}' for n, x in r.items()))
    assert max(r.values()) <= 0.6, r


def _pick(pred):
    return [c for c in CASES if pred(*c)]


_keys = SC.group_keys


FAULT_CASES = _pick(lambda k, s, dt, st: k != 'keymask')


@pytest.mark.parametrize('kind,shape,dt,stair', _pick(lambda k, s, dt, st: k != 'keymask' and max(SC.row_shifts(k, s)) >= 96),
                         ids=_id)
def test_no_max_subtraction_is_rejected(kind, shape, dt, stair):
    """exp2 of an unshifted score of +96 or +120 overflows: the result is non-finite."""
    case = SC.make(kind, shape, dt, stair)
    got = SC.emulate(case, 'nomax')
    assert not all(torch.isfinite(x).all() for x in got.values())
    assert max(SC.ratios(case, got).values()) == math.inf


@pytest.mark.parametrize('kind,shape,dt,stair',
                         _pick(lambda k, s, dt, st: k in ('space', 'cross', 'mq') and _keys(k, s) % 16 != 0 and st <= 0
                               and min(SC.row_shifts(k, s)) == -120),
                         ids=_id)
def test_unmasked_padded_key_in_the_backward_is_rejected(kind, shape, dt, stair):
    """A padded key (zero row, score 0) that the backward's recomputation does not mask: P = exp2(-lse log2e) overflows on
    the rows with lse < -88.7, and inf * 0 reaches dq."""
    case = SC.make(kind, shape, dt, stair)
    assert case.ref['lse'].min() < -89
    got = SC.emulate(case, 'pad')
    assert not torch.isfinite(got['dq']).all()
    assert SC.ratios(case, got)['dq'] == math.inf


@pytest.mark.parametrize('kind,shape,dt,stair',
                         _pick(lambda k, s, dt, st: k in ('space', 'cross', 'mq', 'cls', 'causal') and _keys(k, s) > 64
                               and (st > 0 or (st == 0 and (_keys(k, s) - 1) % 64 >= 31))), ids=_id)
def test_stale_maximum_in_one_rescale_is_rejected(kind, shape, dt, stair):
    """The last key tile rescales the accumulators by the maximum before its own update. (With stair -4 the first tile
    holds every maximum and the factor is 1 either way, and with stair 0 a last tile of fewer than 32 keys rarely raises the
    maximum: those cases cannot see the fault and are not asked to.)"""
    case = SC.make(kind, shape, dt, stair)
    r = SC.ratios(case, SC.emulate(case, 'stale'))
    assert max(r.values()) > 1, r


@pytest.mark.parametrize('kind,shape,dt,stair', FAULT_CASES, ids=_id)
def test_perturbed_lse_is_rejected(kind, shape, dt, stair):
    """lse off by 2^-10 (float32) or 2^-4 (bf16): rejected on lse itself AND on a gradient computed from it."""
    case = SC.make(kind, shape, dt, stair)
    r = SC.ratios(case, SC.emulate(case, 'lse'))
    assert r['lse'] > 1 and max(r['dq'], r['dk'], r['dv']) > 1, r
