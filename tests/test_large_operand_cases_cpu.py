"""CPU: the arithmetic of tests/large_operand_cases.py. Every case's named operand really straddles the boundary it is
there for (its last row starts beyond it, with at least one whole tile / step / row group and a partial one behind the
boundary), the entry point's documented limits hold at the shape, the test fits the 40 GiB memory cap, and the host gates of
lavila_amd/ops.py sit where the table says: one row below and at every limit."""
import pytest

import large_operand_cases as L

BOUNDARY = {'B31': L.B31, 'B32': L.B32, 'E31': L.E31}


@pytest.mark.parametrize('case', L.ALL_CASES, ids=lambda c: c.name)
def test_operand_straddles_its_boundaries(case):
    assert case.operands
    for op in case.operands:
        assert op.crosses
        for b in op.crosses:
            per_row = op.cols * (1 if b == 'E31' else op.esize)
            first = L.first_row_beyond(op, b)
            assert first * per_row >= BOUNDARY[b] > (first - 1) * per_row
            assert first >= 1, 'nothing in front of the boundary'
            # the last row starts beyond the boundary ...
            assert (op.rows - 1) * per_row >= BOUNDARY[b], (op.name, b)
            # ... a whole unit (tile / step / row group) lies beyond it, and the rows end in a partial unit
            unit = case.unit
            first_unit = L.ceil_div(first, unit) * unit
            assert first_unit + unit <= op.rows // unit * unit or (unit == 1 and op.rows - first >= 2), (op.name, b)
            if unit > 1:
                assert op.rows % unit != 0, (op.name, 'no partial tail')
        for b in set(BOUNDARY) - set(op.crosses):          # and crosses nothing the row does not name
            assert op.rows * op.cols * (1 if b == 'E31' else op.esize) <= BOUNDARY[b], (op.name, b)


@pytest.mark.parametrize('case', L.ALL_CASES, ids=lambda c: c.name)
def test_case_fits_the_memory_cap(case):
    assert 0 < L.peak_bytes(case) <= L.MEMORY_CAP, (case.name, L.peak_bytes(case) / L.GIB)


@pytest.mark.parametrize('case', L.TN_CASES, ids=lambda c: c.name)
def test_tn_cases_respect_the_documented_limits(case):
    """lvl_linear_tn / _ragged: N % 256 (64) == 0, K % 64 == 0, x and w below 4 GiB, fewer than 2^31 tiles; f32 class:
    K = 3 x a multiple of 64. The chunk calls (TN_CHUNK rows, a multiple of 256) keep every operand below B31."""
    s = case.shape
    M, N, K = s['M'], s['N'], s['K']
    assert N % (64 if 'ragged' in case.entry else 256) == 0 and K % 64 == 0
    assert M * K * 2 < L.B32 and N * K * 2 < L.B32
    assert L.ceil_div(M, 256) * (N // 256) < 1 << 31
    if s['f32']:
        assert K % 192 == 0 and set(s['epilogues']) <= set(L.F32_EPILOGUES)
    chunk = L.tn_chunk(case)
    out_e = 4 if s['f32'] else 2
    assert chunk % 256 == 0 and chunk * K * 2 < L.B31 and chunk * N * out_e < L.B31
    wins = L.tn_windows(case)
    assert wins[0] == (0, 256) and wins[-1][1] == M and wins[-1][0] % 256 == 0 and 0 < M - wins[-1][0] < 256
    assert all(0 <= a < b <= M and b - a <= 512 for a, b in wins)


def test_tn_tail_tile_offsets():
    """x_below_b32: the last tile's rows end exactly at 2^32 (no 32-bit sum wraps, X fills the range). x_tail_wraps: the
    largest M the entry takes at K = 4160; the tail tile's rows behind M have byte offsets past 2^32, so the kernel's
    per-lane `xrel + f_xrow` wraps for them (they are clamped to the last row's chunk or, wrapped, read rows near the
    start of X: never stored). The refused shape is exactly one row more than x_below_b32."""
    row = 2 * 4096
    assert L.M_X32 * row < L.B32 == (L.M_X32 + 1) * row == L.ceil_div(L.M_X32, 256) * 256 * row
    row = 2 * L.K_WRAP
    assert L.M_WRAP * row < L.B32 <= (L.M_WRAP + 1) * row
    tail_end = L.ceil_div(L.M_WRAP, 256) * 256
    assert L.M_WRAP % 256 != 0 and tail_end * row > L.B32 and (tail_end - 256) * row < L.B32
    wrapped = [(r * row) % L.B32 for r in range(L.M_WRAP, tail_end) if r * row >= L.B32]
    assert wrapped and max(wrapped) + 128 < (L.M_WRAP - 1) * row        # a wrapped offset lands inside X, below the clamp
    assert L.TN_REFUSED['M'] * L.TN_REFUSED['K'] * 2 == L.B32 and L.TN_REFUSED['M'] == L.M_X32 + 1


@pytest.mark.parametrize('case', L.WGRAD_CASES, ids=lambda c: c.name)
def test_wgrad_cases_have_a_plan_and_stay_exact(case):
    """the library tiles the shape (one shape per tile family), the row count leaves a < 32-row tail for the reduction
    kernel, and the marked rows sit on both sides of every boundary"""
    from lavila_amd import _cabi as C
    from wgrad_cases import plan
    s = case.shape
    p = plan(C.lib(), s['M'], s['N'], s['K'])
    assert p is not None and p['S'] >= 2, p
    family = {256: (5, 6, 7), 768: (0, 1, 2, 3, 4), 320: (8, 9, 10, 11, 12)}[s['N']]
    assert p['cfg'] in family, p
    assert 0 < s['M'] % 32 < 32 and s['M'] // 32 < 1 << 31
    # a full row offset is formed only where a stream starts: at least one split's first row lies beyond B32 (and one
    # beyond B31) in both operands
    starts = [(sp * p['base'] + min(sp, p['rem'])) * 32 for sp in range(p['S'])]
    for op in case.operands:
        for b in ('B31', 'B32'):
            assert any(r >= L.first_row_beyond(op, b) for r in starts), (op.name, b, starts[-1])
    marks = L.marked_rows(case)
    assert marks[0] == 0 and marks[-1] == s['M'] - 1 and len(marks) >= 6
    for op in case.operands:
        for b in op.crosses:
            r = L.first_row_beyond(op, b)
            assert r - 1 in marks and r in marks


@pytest.mark.parametrize('case', L.LN_CASES + L.ROWS_CASES, ids=lambda c: c.name)
def test_row_kernel_cases_respect_the_documented_limits(case):
    import rowops_reference as R
    s = case.shape
    assert s['cols'] % 8 == 0 and s['cols'] <= 4096 and s['rows'] < 1 << 32
    if case.family == 'layernorm':
        assert s['rows'] % s['rows_per_sample'] == 0 and 1 < s['rows_per_sample'] < 64
    else:
        assert s['rows'] * s['cols'] % 8 == 0
        # the case's unit is the longest sweep of any of the kernels (mirrors of the launch geometry: rowops_reference)
        sweeps = (R.GELU_UNROLL * R.gelu_fwd_gy(s['rows'], s['cols']), R.GELU_UNROLL * R.gelu_bwd_gy(s['rows']),
                  L.ceil_div(4096 * 256 * 8, s['cols']))
        assert case.unit == L.sweep_rows(s['cols']) >= max(sweeps), sweeps


def test_gather_cases_count_samples():
    for case in L.GATHER_CASES:
        op = case.operands[0]
        assert op.rows == case.shape['B'] and (op.rows - 1) * op.cols * op.esize >= L.B31 > (op.rows - 2) * op.cols * op.esize
    t = dict((c.name, c) for c in L.GATHER_CASES)['text_embed'].shape
    assert t['B'] * t['L'] < 1 << 31


@pytest.mark.parametrize('case', L.ATTN_CASES, ids=lambda c: c.name)
def test_replicated_attention_cases(case):
    """whole replicas, the last one beyond the boundary; a sample's byte size does not divide 2^32, so a wrapped offset
    never lands on a replica boundary; the replica scales have no short period; the kernel family takes the shape in the
    case's dtype (no generic kernel), and float32 runs at half the bf16 batch"""
    from lavila_amd import _cabi as C
    s = case.shape
    assert s['B'] % s['B0'] == 0 and s['B0'] <= 8
    assert (s['B'] - s['B0']) * s['sample_bytes'] >= L.B32
    assert L.B32 % s['sample_bytes'] != 0 and L.B31 % s['sample_bytes'] != 0
    scales = [L.replica_scales(r) for r in range(4096)]
    assert len(set(scales)) == 36
    for period in range(1, 1025):
        assert any(scales[r] != scales[r + period] for r in range(64)), period
    if s['mode'] != 'cls':              # the cls-only kernels take any shape in both dtypes
        fast = C.lib().lvl_attention_fast_path if s['esize'] == L.BF16 else C.lib().lvl_attention_fast_path_f32
        assert fast({'space': 0, 'time': 1, 'causal': 2}[s['mode']], s['F'], s['N'], s['H']) == 1
    if s['esize'] == L.F32:
        twin = next(c for c in L.ATTN_CASES if c.name == case.name[:-3] + 'bf16')
        assert abs(2 * s['B'] - twin.shape['B']) <= 4 * s['B0']


def test_attention_families_without_a_float32_instantiation():
    from lavila_amd import _cabi as C
    names = {c.name for c in L.ATTN_CASES}
    assert 'time_mfma_bf16' in names and 'time_mfma_f32' not in names
    for mode, F, N, H in L.ATTN_NO_F32:
        assert C.lib().lvl_attention_fast_path_f32({'space': 0, 'time': 1}[mode], F, N, H) == 0


def test_host_routing_rows():
    """the fused MLP's two runs: a 256-row tile below the gate every GEMM operand is below 4 GiB, at the gate the hidden
    tensor passes 2^31 elements; ops routes by _mlp_fused_ok's four _tn_ok questions; both fit the memory cap"""
    from lavila_amd import ops
    d, h = L.MLP_WIDTHS
    below, at = L.MLP_ROWS['below_gate'], L.MLP_ROWS['at_gate']
    assert at - below == 256 and below * h * 2 < L.B32 <= at * h * 2 and at * h > L.E31 > below * h
    for rows, want in ((below, True), (at, False)):
        assert (ops._tn_ok(rows, h, d) and ops._tn_ok(rows, d, h)) is want
        assert L.mlp_peak_bytes(rows) <= L.MEMORY_CAP


def test_element_boundary_is_reached_where_the_memory_cap_allows():
    """The kernels index ELEMENTS in C++: an `int` index goes wrong at E31, not at a byte boundary. Every family whose
    tensors fit the cap at 2^31 elements has a case there; the per-sample gathers and the float32 LayerNorm cases stop at
    the byte boundaries (noted in DESIGN.md)."""
    reached = {c.family for c in L.ALL_CASES for op in c.operands if 'E31' in op.crosses}
    assert reached == {'tn', 'wgrad', 'rows', 'layernorm', 'xent', 'attention'}


@pytest.mark.parametrize('name,args,want', L.GATES, ids=lambda v: str(v).replace(' ', ''))
def test_host_gates(name, args, want):
    from lavila_amd import ops
    assert ops.F32_MFMA, 'the table assumes the default (LAVILA_F32_MFMA unset)'
    assert getattr(ops, name)(*args) is want, (name, args)


def test_host_gates_cover_every_predicate_at_both_sides():
    seen = {}
    for name, _, want in L.GATES:
        seen.setdefault(name, set()).add(want)
    assert set(seen) == {'_tn_ok', '_tn_ragged_ok', '_tn_ok_f32', '_wgrad_f32_ok', '_skinny_ok', '_skinny_f32_ok'}
    assert all(v == {True, False} for v in seen.values()), seen


def test_text_embed_fwd_refuses_2_31_token_rows():
    """lvl_text_embed_fwd launches one workgroup per token row and indexes it with an int: B * L >= 2^31 is refused on the
    host, before any launch (the pointers are never dereferenced: 16-byte aligned dummies)."""
    from lavila_amd import _cabi as C
    lib = C.lib()
    p = lambda: __import__('ctypes').c_void_p(4096)
    rc = lib.lvl_text_embed_fwd(p(), 1 << 15, p(), p(), p(), 1 << 16, 1 << 15, 8, 100, C.LVL_BF16, None)
    assert rc == -22 and b'too many token rows' in lib.lvl_last_error()
