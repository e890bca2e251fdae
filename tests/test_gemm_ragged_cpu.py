"""CPU: host routing of the ragged-width GEMMs (widths in 64s that are not multiples of 256: GPT-2 XL's 1600 / 3200 / 4800
and the 320-wide test layout) -- the two predicates' truth table, the loud failure of the new entry point without a device,
and the weight-gradient plans: every earlier shape answers what it answered before the 160-family tiles existed."""
import pytest
import torch


# (rows, n_out, n_in) -> (_tn_ok, _tn_ragged_ok)
TRUTH = {
    # the base decoder and the towers: lvl_linear_tn as before (the ragged predicate holds too and is never asked)
    (2464, 768, 768): (True, True), (2464, 2304, 768): (True, True), (2464, 3072, 768): (True, True),
    (2464, 768, 3072): (True, True), (2464, 768, 2304): (True, True),
    # GPT-2 XL: c_attn, c_proj / q_attn, cross c_attn, c_fc forward, and the input gradients (N and K swapped)
    (2464, 4800, 1600): (False, True), (2464, 1600, 1600): (False, True), (2464, 3200, 1600): (False, True),
    (2464, 6400, 1600): (True, True), (2464, 1600, 6400): (False, True), (2464, 1600, 4800): (False, True),
    (2464, 1600, 3200): (False, True), (2464, 50432, 1600): (True, True), (2464, 1600, 50432): (False, True),
    # the 320-wide test layout: remainders 192, 64, 128, and the c_fc that tiles
    (33, 960, 320): (False, True), (33, 320, 320): (False, True), (33, 640, 320): (False, True),
    (33, 1280, 320): (True, True), (33, 320, 1280): (False, True), (1, 320, 256): (False, True),
    # a side below one full tile: the host keeps the earlier routing (the entry point itself serves these shapes)
    (1, 64, 64): (False, False), (1, 128, 64): (False, False), (1, 192, 64): (False, False), (1, 448, 64): (False, False),
    (33, 192, 192): (False, False), (33, 576, 192): (False, False), (33, 192, 768): (False, False),
    (33, 768, 192): (True, False), (33, 256, 64): (True, False),
    # neither: no rows, widths off the 64 grid, operands of 4 GiB
    (0, 1600, 1600): (False, False), (33, 1600, 1632): (False, False), (33, 1632, 1600): (False, False),
    (33, 331, 320): (False, False), (33, 256, 96): (False, False), (1 << 20, 1600, 2048): (False, False),
    ((1 << 20) - 1, 1600, 2048): (False, True), (1 << 20, 2048, 1600): (False, False),
}


def test_predicates_truth_table():
    from lavila_amd import ops
    got = {k: (ops._tn_ok(*k), ops._tn_ragged_ok(*k)) for k in TRUTH}
    assert got == TRUTH, {k: (got[k], v) for k, v in TRUTH.items() if got[k] != v}
    for k in TRUTH:
        assert ops._tn_rows_ok(*k) == any(TRUTH[k])


def test_routing_prefers_the_existing_entry(monkeypatch):
    """linear_tn_rows: lvl_linear_tn where _tn_ok holds, the ragged entry where only the new predicate does, None otherwise"""
    from lavila_amd import ops
    calls = []
    monkeypatch.setattr(ops, 'linear_tn_raw', lambda x, w, b, epi: calls.append(('tn', w.shape[0])) or 'tn')
    monkeypatch.setattr(ops, 'linear_tn_ragged_raw', lambda x, w, b: calls.append(('ragged', w.shape[0])) or 'ragged')
    x = torch.zeros(5, 320, dtype=torch.bfloat16)
    for n, want in ((1280, 'tn'), (768, 'tn'), (960, 'ragged'), (320, 'ragged'), (64, None), (192, None), (331, None)):
        assert ops.linear_tn_rows(x, torch.zeros(n, 320, dtype=torch.bfloat16), None) == want, n
    assert ops.linear_tn_rows(torch.zeros(5, 96, dtype=torch.bfloat16), torch.zeros(256, 96, dtype=torch.bfloat16)) is None
    assert calls == [('tn', 1280), ('tn', 768), ('ragged', 960), ('ragged', 320)]


def test_ragged_entry_is_loud_without_a_device():
    from lavila_amd import ops
    from lavila_amd._cabi import HipExtensionError
    x = torch.zeros(4, 320, dtype=torch.bfloat16)
    w = torch.zeros(960, 320, dtype=torch.bfloat16)
    with pytest.raises(HipExtensionError, match='no CPU'):
        ops.linear_tn_ragged_raw(x, w, torch.zeros(960))
    with pytest.raises(HipExtensionError, match='no CPU'):
        ops.linear_tn_rows(x, w)


def test_wgrad_plans_exist_for_the_160_family():
    """host-only workspace query: both sides of every Conv1D weight at widths 1600 and 320, and the padded-vocabulary lm_head of
    the test layouts; the real vocabulary against 1600 stays unsupported (more tiles than compute units)"""
    from lavila_amd import _cabi as C
    ws = C.lib().lvl_workspace_floats
    for d in (320, 1600):
        for n, k in ((d, 3 * d), (d, d), (d, 4 * d), (4 * d, d), (d, 2 * d), (512, d)):
            assert ws(b'linear_wgrad', n, k) >= n * k, (n, k)
    for n, k in ((160, 160), (320, 160), (160, 320)):
        assert ws(b'linear_wgrad', n, k) >= n * k, (n, k)
    assert ws(b'linear_wgrad', 50432, 1600) == -1
    assert ws(b'linear_wgrad', 1600, 1632) == -1


# lvl_workspace_floats('linear_wgrad', N, K) on the commit before the 160-family existed (host code: read off a build of that
# commit; 256 compute units). A changed answer means a changed plan for a shape the towers or the base decoder run.
PLAN_WIDTHS = (768, 1024, 1280, 2304, 3072, 4096)
PLANS_BEFORE = {
    (768, 768): 18898944, (768, 1024): 15744000, (768, 1280): 15740928, (768, 2304): 17702400, (768, 3072): 18880512,
    (768, 4096): 15732480, (1024, 768): 15749120, (1024, 1024): 16793600, (1024, 1280): 15740928, (1024, 2304): 14161920,
    (1024, 3072): 15733760, (1024, 4096): 16781312, (1280, 768): 15749120, (1280, 1024): 15744000, (1280, 1280): 13117440,
    (1280, 2304): -1, (1280, 3072): 15733760, (1280, 4096): 15732480, (2304, 768): 17717760, (2304, 1024): 14169600,
    (2304, 1280): -1, (2304, 2304): 15932160, (2304, 3072): 14160384, (2304, 4096): 9439488, (3072, 768): 18898944,
    (3072, 1024): 15744000, (3072, 1280): 15740928, (3072, 2304): 14161920, (3072, 3072): 18880512, (3072, 4096): 12585984,
    (4096, 768): 15749120, (4096, 1024): 16793600, (4096, 1280): 15740928, (4096, 2304): 9441280, (4096, 3072): 12587008,
    (4096, 4096): 16781312}


def test_wgrad_plans_of_earlier_shapes_unchanged():
    from lavila_amd import _cabi as C
    assert set(PLANS_BEFORE) == {(n, k) for n in PLAN_WIDTHS for k in PLAN_WIDTHS}
    got = {nk: C.lib().lvl_workspace_floats(b'linear_wgrad', *nk) for nk in PLANS_BEFORE}
    assert got == PLANS_BEFORE, {nk: (got[nk], v) for nk, v in PLANS_BEFORE.items() if got[nk] != v}
