"""CPU-only helper of tests/test_gpu_text_embed_exact.py and tests/test_text_embed_reference_cpu.py: the float64 reference of
lvl_text_embed_fwd / _bwd (csrc/text_embed.hip), a restatement of the table kernel's scan partition that says which of its
branches a token list reaches, and the case list. Nothing here is sampled: token patterns and the integer operands are
closed formulas of the row and column index, so that what a case reaches it reaches by construction."""
import torch

# every width the three towers use (512 / 768 CLIP and DistilBERT; 768 / 1024 / 1280 / 1600 GPT-2) and one on each side of
# every boundary of the kernels' column walk: the table kernel's four column groups of 512 (c = (k * 64 + lane) * 8), the
# 512-column passes of the forward (c += 128 * 4) and of the positional kernel (cb += 512), the smallest and the largest width
WIDTHS = (8, 504, 512, 520, 768, 1024, 1032, 1280, 1536, 1544, 1600, 2040, 2048)
R_VALUES = (1, 63, 64, 65, 8 * 64, 8 * 64 + 1)       # plus one that is no multiple of 64 (asserted in the CPU file)
B_VALUES = (1, 2, 3, 4, 7)                           # the positional kernel's batch quarters [B q / 4, B (q + 1) / 4)
MAX_ROWS = 4096
DX_MAX = 8                                           # |integer dx| <= 8: exact in bfloat16 (8 significand bits)

FEATURES = ('once', 'dups_only_wave0', 'dups_in_3plus_waves', 'dups_in_wave7', 'window_1_match', 'window_2_matches',
            'window_odd_ge3', 'window_64_matches', 'range_cut_by_R', 'empty_range', 'first_at_R_minus_1',
            'first_at_R_minus_2_dup_at_R_minus_1', 'all_rows_one_token')

# (B, L, ctx, V, W, token pattern, token stride): tokens [B, L] are read in place with that row stride -- ctx: the `[:, :L]`
# view of a [B, ctx] tensor, L: a contiguous tensor; ctx is also the number of rows of the positional table
CASES = [
    (1, 1, 4, 3, 8, 'distinct', 1),                  # R = 1: one row, first at R - 1, nothing to scan
    (1, 1, 4, 3, 8, 'distinct', 4),
    (2, 3, 8, 16, 8, 'tail_pair', 8),                # R = 6: first at R - 2 with its only duplicate at R - 1
    (3, 21, 77, 300, 504, 'ladder', 77),             # R = 63
    (7, 9, 16, 64, 520, 'captions', 16),             # R = 63, seven captions: quarters of 1 / 2 / 2 / 2
    (4, 16, 16, 200, 512, 'one', 16),                # R = 64, ctx == L: no zero rows in dpos; 63 matches, range cut by R
    (2, 32, 77, 400, 768, 'ladder', 32),             # R = 64
    (1, 65, 77, 97, 1024, 'one', 77),                # R = 65: exactly one full window of 64 matches, 7 empty ranges
    (1, 65, 128, 300, 1032, 'tail_pair', 65),        # R = 65
    (4, 128, 128, 50, 1280, 'one', 128),             # R = 8 * 64: wave 7's range is cut by R (63 matches)
    (2, 256, 300, 1000, 1536, 'ladder', 300),        # R = 8 * 64
    (3, 171, 200, 1000, 1544, 'sparse', 200),        # R = 8 * 64 + 1: one match per window, in every wave
    (1, 513, 600, 40, 1600, 'one', 600),             # R = 8 * 64 + 1: eight ranges of exactly 64 rows, none cut
    (7, 77, 77, 997, 2040, 'captions', 77),          # R = 539
    (3, 77, 77, 700, 2048, 'ladder', 77),            # R = 231: no multiple of 64
    (32, 128, 128, 600, 512, 'captions', 128),       # R = 4096: the largest, a padding id with thousands of duplicates
]

# the two full-sized tables (bf16): (B, L, ctx, V, W, pattern, stride); only the occurring rows are compared
LARGE_CASES = [
    (2, 9, 1024, 50257, 1600, 'captions', 1024),     # GPT-2 XL: the narrator's tied table
    (2, 300, 512, 30522, 768, 'captions', 512),      # DistilBERT
]


def pattern(name, B, L, V):
    """The [B, L] int64 token matrix of a pattern; flat row r = b L + l."""
    R = B * L
    r = torch.arange(R, dtype=torch.int64)
    if name == 'distinct':                            # every token once
        assert V >= R
        t = r.clone()
    elif name == 'one':                               # one token everywhere
        t = torch.full((R,), min(1, V - 1), dtype=torch.int64)
    elif name == 'tail_pair':                         # distinct, but the last two rows share a token
        assert V >= R >= 2
        t = r.clone()
        t[R - 1] = t[R - 2]
    elif name == 'sparse':                            # token 2 at every 67th row (at most one per 64-row window), else distinct
        assert V >= R + 3
        t = r + 3
        t[r % 67 == 0] = 2
    elif name == 'ladder':
        # token 5 at rows {0, 3}: one match; 6 at {1, 4, 5}: two; 7 at {2, 6, 7, 8}: three; 8 at {9, 20, 21, 22, 23, 24}: five;
        # with room, token 9 at row 30 and rows 31 .. 94 (the first window behind its first row: 64 matches); else distinct
        assert V >= R + 100 and R >= 31
        t = r + 100
        for tok, rows in ((5, (0, 3)), (6, (1, 4, 5)), (7, (2, 6, 7, 8)), (8, (9, 20, 21, 22, 23, 24))):
            t[list(rows)] = tok
        if R >= 95:
            t[30:95] = 9
    elif name == 'captions':
        # ragged captions: the start token V - 1 once per caption, words from a set of 11, then the padding id 0 from
        # position 1 + (5 b) % L on (caption 0 is all padding behind its start token)
        assert V >= 16
        b, l = r // L, r % L
        t = 3 + (7 * b + 3 * l) % 11
        t[l == 0] = V - 1
        t[(l > 0) & (l >= 1 + (5 * b) % L)] = 0
    else:
        raise ValueError(name)
    assert int(t.min()) >= 0 and int(t.max()) < V     # never an out-of-range id
    return t.reshape(B, L)


def strided_tokens(tokens, stride):
    """The [B, L] tokens as a view with row stride `stride` (>= L) of a [B, stride] tensor whose other columns hold ids that
    differ from every neighbour's (a kernel that ignored the stride would gather other rows)."""
    B, L = tokens.shape
    assert stride >= L
    full = (tokens.max() - torch.arange(B * stride, dtype=torch.int64).reshape(B, stride) % (tokens.max() + 1))
    full[:, :L] = tokens
    return full


def integer_dx(B, L, W):
    """[B, L, W] float32 integers in [-8, 8]: a formula of row and column in which neighbouring rows and columns differ."""
    r = torch.arange(B * L, dtype=torch.int64)[:, None]
    c = torch.arange(W, dtype=torch.int64)[None, :]
    v = (r * 31 + c * 17 + (r * c) % 13 + (r // 64) * 5 + (c // 512) * 3) % (2 * DX_MAX + 1) - DX_MAX
    return v.to(torch.float32).reshape(B, L, W)


def reference(tokens, table, pos, dx):
    """float64: x = table[tokens] + pos[:L]; dtable = index_add_ of the dx rows; dpos[:L] = batch sum, rows >= L zero.
    tokens [B, L] int64, table [V, W], pos [ctx, W], dx [B, L, W] (any float dtype; all on the CPU)."""
    B, L = tokens.shape
    V, W = table.shape
    t64, p64, d64 = table.double(), pos.double(), dx.double()
    x = t64[tokens] + p64[:L]
    dtable = torch.zeros(V, W, dtype=torch.float64).index_add_(0, tokens.reshape(-1), d64.reshape(-1, W))
    dpos = torch.zeros(pos.shape[0], W, dtype=torch.float64)
    dpos[:L] = d64.sum(0)
    return x, dtable, dpos


def occurring_rows(tokens, dx):
    """(ids [U] sorted, float64 sums [U, W], counts [U]): the rows of dtable that are not zero by definition, without a
    [V, W] reference (the full-sized tables)."""
    ids, inv, counts = torch.unique(tokens.reshape(-1), return_inverse=True, return_counts=True)
    W = dx.shape[-1]
    rows = torch.zeros(ids.numel(), W, dtype=torch.float64).index_add_(0, inv, dx.double().reshape(-1, W))
    return ids, rows, counts


K_TAB_WAVES = 8
SCAN = 64


def scan_census(tokens_flat):
    """Which branches of text_embed_bwd_table_kernel a flat token list reaches. Restates, from csrc/text_embed.hip:
        kTabWaves = 8                                             (`constexpr int kTabWaves = 8;`)
        the kernel's `if (first[v] != r) return;` / `if (n > 1)`  (the first row of a token scans, and only with duplicates)
        span = R - (r + 1); per = ((span + kTabWaves - 1) / kTabWaves + 63) & ~63
        lo = r + 1 + wave * per, hi = min(R, lo + per)
        for (base = lo; base < hi; base += 64) with the ballot `rr < hi && tok32[rr] == v`
        the `while (m)` loop: matches taken two at a time, a last single one through the `else` branch
    Moving any of these in the kernel without moving it here makes tests/test_text_embed_reference_cpu.py lose a feature."""
    tok = [int(v) for v in tokens_flat]
    R = len(tok)
    rows = {}
    for r, v in enumerate(tok):
        rows.setdefault(v, []).append(r)
    feats = set()
    for v, rs in rows.items():
        r, n = rs[0], len(rs)
        if r == R - 1:
            feats.add('first_at_R_minus_1')
        if r == R - 2 and tok[R - 1] == v:
            feats.add('first_at_R_minus_2_dup_at_R_minus_1')
        if n == R and R > 1:
            feats.add('all_rows_one_token')
        if n == 1:
            feats.add('once')
            continue
        span = R - (r + 1)
        per = ((span + K_TAB_WAVES - 1) // K_TAB_WAVES + 63) & ~63
        waves = set()
        for wave in range(K_TAB_WAVES):
            lo = r + 1 + wave * per
            hi = min(R, lo + per)
            if lo >= R:
                feats.add('empty_range')
                continue
            if lo + per > R:
                feats.add('range_cut_by_R')
            for base in range(lo, hi, SCAN):
                m = sum(1 for rr in range(base, min(base + SCAN, hi)) if tok[rr] == v)
                if m:
                    waves.add(wave)
                if m == 1:
                    feats.add('window_1_match')
                if m == 2:
                    feats.add('window_2_matches')
                if m >= 3 and m % 2:
                    feats.add('window_odd_ge3')
                if m == SCAN:
                    feats.add('window_64_matches')
        if waves == {0}:
            feats.add('dups_only_wave0')
        if len(waves) >= 3:
            feats.add('dups_in_3plus_waves')
        if K_TAB_WAVES - 1 in waves:
            feats.add('dups_in_wave7')
    return feats


def overrun_matches(tokens_flat, V, guard=(0x5a5a5a5a,) * 64):
    """(token, row) pairs a scan WITHOUT the `min(R, ...)` of `hi` would match at rows >= R. There the ballot's
    `tok32[rr]` reads the words behind the token list, which lvl_text_embed_bwd lays out as tok32 [R] | first [V] | count [V]
    (`int* first = ws + R; int* count = first + V;`), followed in the GPU tests by 64 sentinel words; first[v'] == v means
    token v' first occurs at row v. Each such match would add a dx row >= R: the NaN rows the GPU tests keep behind dx."""
    tok = [int(v) for v in tokens_flat]
    R = len(tok)
    first, count = [0x7fffffff] * V, [0] * V
    for r, v in enumerate(tok):
        first[v] = min(first[v], r)
        count[v] += 1
    ws = tok + first + count + list(guard)
    out = []
    for v in sorted(set(tok)):
        r, n = first[v], count[v]
        if n == 1:
            continue
        per = ((R - (r + 1) + K_TAB_WAVES - 1) // K_TAB_WAVES + 63) & ~63
        for wave in range(K_TAB_WAVES):
            lo = r + 1 + wave * per
            out += [(v, rr) for rr in range(max(lo, R), min(lo + per, len(ws))) if ws[rr] == v]
    return out
