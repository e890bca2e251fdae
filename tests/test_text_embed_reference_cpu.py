"""CPU: the case list of tests/test_gpu_text_embed_exact.py reaches every branch of the token-embedding kernels
(csrc/text_embed.hip) by construction, and its float64 reference is nn.Embedding's.

scan_census (tests/text_embed_reference.py) restates the table kernel's partition -- 8 waves, per = ((span + 7) / 8 + 63) &
~63 rows each, 64-row windows, matches taken two at a time -- so a threshold moved in the kernel alone is not noticed here,
but one moved in both places shows up as a feature no case reaches any more."""
import torch

import text_embed_reference as R


def _census(case):
    B, L, ctx, V, W, name, stride = case
    return R.scan_census(R.pattern(name, B, L, V).reshape(-1).tolist())


def test_every_scan_feature_is_reached_by_a_case():
    reached = {f: [] for f in R.FEATURES}
    for i, case in enumerate(R.CASES):
        got = _census(case)
        assert got <= set(R.FEATURES), got
        for f in got:
            reached[f].append(i)
    print('\nfeature -> cases (index into CASES: B, L, ctx, V, W, pattern, stride)')
    for f in R.FEATURES:
        print(f'  {f:38s} {reached[f]}')
    for i, c in enumerate(R.CASES):
        print(f'  case {i:2d}: {c}  R = {c[0] * c[1]}')
    for f in R.FEATURES:
        assert reached[f], f'no case reaches {f}'


def test_census_of_hand_worked_token_lists():
    """The census itself, on lists small enough to work out by hand."""
    assert R.scan_census([4]) == {'once', 'first_at_R_minus_1'}
    assert R.scan_census([4, 4]) == {'first_at_R_minus_2_dup_at_R_minus_1', 'all_rows_one_token', 'window_1_match',
                                     'dups_only_wave0', 'range_cut_by_R', 'empty_range'}
    # 65 rows of one token: span 64, per 64, wave 0 owns rows 1 .. 64 exactly, waves 1 .. 7 start at R or behind it
    assert R.scan_census([1] * 65) == {'all_rows_one_token', 'window_64_matches', 'dups_only_wave0', 'empty_range'}
    # 513 rows: per = 64, eight ranges of exactly 64 rows
    assert R.scan_census([1] * 513) == {'all_rows_one_token', 'window_64_matches', 'dups_in_3plus_waves', 'dups_in_wave7'}
    # 512 rows: wave 7's range [449, 513) is cut to 63 rows
    assert R.scan_census([1] * 512) == {'all_rows_one_token', 'window_64_matches', 'window_odd_ge3', 'dups_in_3plus_waves',
                                        'dups_in_wave7', 'range_cut_by_R'}
    # first row 0, duplicates at 1 and 2 (two matches), then a third token once at the end
    assert R.scan_census([7, 7, 7, 3]) == {'window_2_matches', 'dups_only_wave0', 'range_cut_by_R', 'empty_range', 'once',
                                           'first_at_R_minus_1'}


def test_widths_rows_and_batches_cover_every_boundary():
    widths = {c[4] for c in R.CASES}
    assert widths >= set(R.WIDTHS), set(R.WIDTHS) - widths
    assert set(R.WIDTHS) >= {8, 504, 512, 520, 768, 1024, 1032, 1280, 1536, 1544, 1600, 2040, 2048}
    for bound in (512, 1024, 1536):                  # column-group / pass boundaries: below, at and above
        assert any(bound - 512 < w < bound for w in widths) and bound in widths and any(bound < w < bound + 512 for w in widths)
    assert all(w % 8 == 0 and w <= 2048 for w in widths)
    rows = {c[0] * c[1] for c in R.CASES}
    assert rows >= set(R.R_VALUES) and any(r % 64 for r in rows if r > 65)
    assert max(rows) <= R.MAX_ROWS
    assert {c[0] for c in R.CASES} >= set(R.B_VALUES)
    strides = {(c[6] == c[1], c[6] > c[1]) for c in R.CASES}
    assert strides == {(True, False), (False, True)}            # contiguous tokens and `[:, :L]` views
    assert any(c[2] == c[1] for c in R.CASES) and any(c[2] > c[1] for c in R.CASES)    # dpos with and without zero rows
    for B, L, ctx, V, W, name, stride in R.CASES + R.LARGE_CASES:
        assert ctx >= L and stride >= L
        t = R.pattern(name, B, L, V)
        full = R.strided_tokens(t, stride)
        assert torch.equal(full[:, :L], t) and 0 <= int(full.min()) and int(full.max()) < V
    print('\nwidths', sorted(widths), '\nrows', sorted(rows), '\nbatches', sorted({c[0] for c in R.CASES}))


def test_integer_operands_keep_every_sum_exact():
    """|dx| <= 8 and at most R <= 4096 terms: |sum| <= 2^15 < 2^24, so every partial sum in any order is a float32 (and the
    operands are bfloat16) exactly."""
    assert R.DX_MAX * R.MAX_ROWS <= 2 ** 15 < 2 ** 24
    for B, L, ctx, V, W, name, stride in R.CASES + R.LARGE_CASES:
        assert B * L <= R.MAX_ROWS
        dx = R.integer_dx(B, L, W)
        assert dx.shape == (B, L, W) and float(dx.abs().max()) <= R.DX_MAX and torch.equal(dx, dx.round())
        assert torch.equal(dx.to(torch.bfloat16).float(), dx)
        assert float(dx.min()) == -R.DX_MAX and float(dx.max()) == R.DX_MAX or dx.numel() < 64
        ids, rows, counts = R.occurring_rows(R.pattern(name, B, L, V), dx)
        assert int(counts.sum()) == B * L and int(counts.max()) <= R.MAX_ROWS
        for t in (rows, dx.double().sum(0)):
            assert float(t.abs().max()) <= 2 ** 15 and torch.equal(t.float().double(), t)


def test_reference_matches_nn_embedding_autograd_in_float64():
    B, L, ctx, V, W = 3, 5, 7, 11, 16
    g = torch.Generator().manual_seed(0)
    tokens = R.pattern('captions', B, L, 16) % V
    table = torch.randn(V, W, generator=g, dtype=torch.float64, requires_grad=True)
    pos = torch.randn(ctx, W, generator=g, dtype=torch.float64, requires_grad=True)
    dx = torch.randn(B, L, W, generator=g, dtype=torch.float64)
    x = torch.nn.functional.embedding(tokens, table) + pos[:L]
    x.backward(dx)
    rx, rt, rp = R.reference(tokens, table.detach(), pos.detach(), dx)
    assert torch.equal(rx, x.detach())
    torch.testing.assert_close(rt, table.grad, rtol=0, atol=1e-14)
    torch.testing.assert_close(rp, pos.grad, rtol=0, atol=1e-14)
    assert float(rp[L:].abs().max()) == 0.0


def test_a_scan_past_the_last_row_would_meet_a_nan_row():
    """Why the GPU file keeps NaN rows behind dx: in these cases a table kernel whose ranges were not cut at R would find a
    workspace word equal to its token behind the token list and add the dx row of that index. The furthest such row lies
    inside the guard (576 rows: no range reaches further than 8 x 64 + 63 rows past R)."""
    hit = {}
    for i, (B, L, ctx, V, W, name, stride) in enumerate(R.CASES):
        m = R.overrun_matches(R.pattern(name, B, L, V).reshape(-1).tolist(), V)
        assert all(B * L <= rr < B * L + 576 for _, rr in m)
        if m:
            hit[i] = m[:3]
    print('\ncase -> (token, row >= R) a scan past R would match:', hit)
    assert len(hit) >= 3 and R.overrun_matches([4, 4], 5) == []
    assert R.overrun_matches(R.pattern('tail_pair', 2, 3, 16).reshape(-1).tolist(), 16) == [(4, 10)]
