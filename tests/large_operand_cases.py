"""Shapes of the large-operand tests (test_gpu_large_operands.py) and what each of them is for: which operand of which entry
point crosses which size boundary. A plain module without torch: test_large_operand_cases_cpu.py checks the arithmetic of
every row here on the CPU (the operand really straddles the boundary, the entry's documented limits hold, the test fits
the memory cap, the host gates of lavila_amd/ops.py are where the table assumes them).

Three boundaries:
    B31 = 2^31 bytes     a signed 32-bit byte offset wraps
    B32 = 2^32 bytes     an unsigned 32-bit byte offset wraps
    E31 = 2^31 elements  a signed 32-bit element index wraps (bf16: the same row as B32, float32: twice B32)
Shapes are as small as the boundary allows: the boundary dimension follows from arithmetic, every other dimension sits at
the entry's minimum (one column tile, one K block, ...) unless the row says why not.
"""
import collections

B31, B32, E31 = 1 << 31, 1 << 32, 1 << 31
GIB = 1 << 30
MEMORY_CAP = 40 * GIB
BF16, F32 = 2, 4

# One operand of a case that crosses boundaries: `rows` rows of `cols` elements of `esize` bytes; `crosses` names them.
Operand = collections.namedtuple('Operand', 'name rows cols esize crosses')
# family: which test runs it; entry: the C entry point(s); shape: the call's arguments; unit: the rows of one tile / step /
# unrolled group of the kernel (at least one whole unit and a partial one must lie beyond every boundary crossed; 1 for the
# flat element-wise kernels and per-sample gathers, where two rows beyond the boundary are asked for);
# tensors: (rows, cols, esize, count) of everything the test holds on the device at its peak.
Case = collections.namedtuple('Case', 'name family entry shape operands unit tensors')


def ceil_div(a, b):
    return -(-a // b)


def first_row_beyond(op, boundary):
    """the first row of the operand that STARTS at or beyond the boundary (all of it lies beyond)"""
    per_row = op.cols * (1 if boundary == 'E31' else op.esize)
    return ceil_div({'B31': B31, 'B32': B32, 'E31': E31}[boundary], per_row)


def peak_bytes(case):
    return sum(r * c * e * n for r, c, e, n in case.tensors)


# ---- lvl_linear_tn / lvl_linear_tn_ragged ---------------------------------------------------------------------------------
TILE = 256
TN_CHUNK = 1 << 17            # rows of a chunk call (a multiple of 256): every chunk operand stays below B31 ...
TN_CHUNK_F32 = 1 << 16        # ... also the float32 outputs of the f32-class mode at N = 4096
M_X31 = (1 << 18) + 256 + 37          # K = 4096: row 2^18 starts at B31; one full tile and a 37-row tail beyond
M_X32 = (1 << 19) - 1                 # K = 4096: X ends one row below B32 (the largest M the entry takes), 255-row tail
K_WRAP = 4160                         # 65 K blocks: 2^32 is no multiple of 256 rows of 8320 bytes ...
M_WRAP = (B32 - 1) // (2 * K_WRAP)    # ... so the tail tile of the largest M the entry takes reaches past 2^32
M_Y = (1 << 19) + 256 + 37            # N = 4096: row 2^19 of y starts at E31 (bf16: = B32; float32: B32 is row 2^18)
N_RAGGED = 320                        # one full column tile + the 64-column edge kernel
M_RAGGED_Y = ceil_div(ceil_div(B32, 2 * N_RAGGED), TILE) * TILE + 256 + 37      # a full tile and a tail behind B32

BF16_EPILOGUES = (0, 1, 2, 3, 4, 5, 6, 7, 8)
F32_EPILOGUES = (0, 1, 2, 3, 6, 7)
AUX_IN, AUX_OUT, COLSUM = (2, 3, 5, 7), (1, 4, 6, 8), (2, 5, 7)


def _tn(name, entry, M, N, K, f32, epilogues, operands, extra=()):
    out_e = F32 if f32 else BF16
    chunk = min(M, TN_CHUNK_F32 if f32 else TN_CHUNK)
    tensors = [(M, K, BF16, 1), (N, K, BF16, 1), (M, N, out_e, 3),            # x, w; y, aux_out, one aux_in at a time
               (chunk, N, out_e, 2), (1 << 14, N, 8, 6)] + list(extra)         # chunk outputs; float64 windows / column sums
    return Case(name, 'tn', entry, dict(M=M, N=N, K=K, f32=f32, epilogues=epilogues), tuple(operands), TILE, tuple(tensors))


TN_CASES = (
    _tn('x_past_b31', 'lvl_linear_tn', M_X31, 256, 4096, False, (0,), [Operand('x', M_X31, 4096, BF16, ('B31',))]),
    _tn('x_below_b32', 'lvl_linear_tn', M_X32, 256, 4096, False, (0, 3), [Operand('x', M_X32, 4096, BF16, ('B31',))]),
    _tn('x_tail_wraps', 'lvl_linear_tn', M_WRAP, 256, K_WRAP, False, (0, 3), [Operand('x', M_WRAP, K_WRAP, BF16, ('B31',))]),
    _tn('y_past_b32', 'lvl_linear_tn', M_Y, 4096, 64, False, BF16_EPILOGUES,
        [Operand('y', M_Y, 4096, BF16, ('B31', 'B32', 'E31'))], extra=[(M_Y, 4096, BF16, 1)]),      # two aux_in tensors kept
    # float32 results: N = 4096 again, so that y also passes 2^31 ELEMENTS (the f32-class epilogue forms its own offsets);
    # at the issue's N = 2048 only the byte boundaries would be crossed
    _tn('y_f32_past_b32', 'lvl_linear_tn', M_Y, 4096, 3 * 192, True, F32_EPILOGUES,
        [Operand('y', M_Y, 4096, F32, ('B31', 'B32', 'E31'))], extra=[(M_Y, 192, F32, 1)]),
    _tn('ragged_y_past_b32', 'lvl_linear_tn_ragged', M_RAGGED_Y, N_RAGGED, 64, False, (0,),
        [Operand('y', M_RAGGED_Y, N_RAGGED, BF16, ('B31', 'B32', 'E31'))]),
    _tn('ragged_x_past_b31', 'lvl_linear_tn_ragged', M_X31, N_RAGGED, 4096, False, (0,),
        [Operand('x', M_X31, 4096, BF16, ('B31',))]),
)
# exactly at the limit: M * K * 2 == 2^32 -> LVL_ENOSYS from both entries, nothing launched
TN_REFUSED = dict(M=1 << 19, N=256, K=4096)


def tn_chunk(case):
    return TN_CHUNK_F32 if case.shape['f32'] else TN_CHUNK


def tn_windows(case):
    """row windows [r0, r1) held to float64: the first tile, 512 rows straddling every boundary crossed, the last tile"""
    M = case.shape['M']
    wins = {(0, min(256, M)), ((M - 1) // 256 * 256, M)}
    for op in case.operands:
        for b in op.crosses:
            r = first_row_beyond(op, b)
            wins.add((max(r - 256, 0), min(r + 256, M)))
    return sorted(wins)


# ---- lvl_linear_wgrad -----------------------------------------------------------------------------------------------------
WGRAD_STEP = 32               # rows of one step of the kernel; the < 32 tail rows are added by the reduction kernel


def _wgrad(N, K):
    # The kernel forms a full row offset only where a STREAM starts (a split's first row, a chunk after a steal) and then
    # advances 64-bit pointers: rows just behind a boundary are reached by pointer increments whatever the offset width.
    # So M runs 2 / 31 past the B32 row: with the up to 256 row splits of a launch at least one split starts beyond it.
    r32 = ceil_div(B32, 2 * max(N, K))
    M = (r32 * 33 // 31 // WGRAD_STEP + 3) * WGRAD_STEP + 5
    ops = [Operand('dy', M, N, BF16, ('B31', 'B32', 'E31')), Operand('x', M, K, BF16, ('B31', 'B32', 'E31'))]
    tensors = [(M, N, BF16, 1), (M, K, BF16, 1), (1 << 18, N + K, 8, 2), (N, K, 8, 4)]
    return Case(f'wgrad_{N}x{K}', 'wgrad', 'lvl_linear_wgrad', dict(M=M, N=N, K=K), tuple(ops), WGRAD_STEP, tuple(tensors))


# one shape per tile family: 128/256, 192/288/384, 160/320
WGRAD_CASES = (_wgrad(256, 256), _wgrad(768, 768), _wgrad(320, 320))


def marked_rows(case):
    """rows the exact-reduction tests mark: the first row, the row before and the row at every boundary, the last row"""
    rows = {0, case.shape['M' if 'M' in case.shape else 'rows'] - 1}
    for op in case.operands:
        for b in op.crosses:
            r = first_row_beyond(op, b)
            rows |= {r - 1, r}
    return sorted(rows)


# ---- element-wise row kernels ---------------------------------------------------------------------------------------------
ROW_UNROLL = 4                # kGeluUnroll / kRowsPerBlock: rows one thread or workgroup has in flight
ELEMENTWISE_ENTRIES = ('lvl_bias_quickgelu_fwd', 'lvl_bias_quickgelu_bwd', 'lvl_quickgelu_apply', 'lvl_act_fwd',
                       'lvl_act_bwd', 'lvl_act_inplace', 'lvl_dropout_apply')


def sweep_rows(cols):
    """rows one whole grid sweep of the widest-striding element-wise kernel covers (lvl_quickgelu_apply: 8192 workgroups x
    1024 vectors of 8); the other kernels' sweeps are shorter: bias + QuickGELU 4 x 1024 rows (backward) or 4 x 4096 / gx
    (forward), the flat activation / dropout kernels 4096 x 256 vectors"""
    return ceil_div(8192 * 1024 * 8, cols)


def _rows_case(name, cols, tail):
    # The kernels run whole sweeps in an unrolled loop and the rest in a tail loop: a few rows behind the boundary (the
    # issue's 2^19 + 3 and 699 051 + 5) would all fall to the tail loops. One whole sweep behind the first sweep boundary
    # at or beyond E31, plus `tail` rows, puts both loops of every kernel past the boundary.
    unit = sweep_rows(cols)
    rows = (ceil_div(ceil_div(E31, cols), unit) + 1) * unit + tail
    op = Operand('u', rows, cols, BF16, ('B31', 'B32', 'E31'))
    tensors = [(rows, cols, BF16, 5), (1 << 16, cols, 8, 6)]        # u, da, a, du, one more; float64 windows
    return Case(name, 'rows', ELEMENTWISE_ENTRIES, dict(rows=rows, cols=cols), (op,), unit, tuple(tensors))


ROWS_CASES = (_rows_case('rows_4096', 4096, 3), _rows_case('rows_3072', 3072, 5))


# ---- LayerNorm family -----------------------------------------------------------------------------------------------------
LN_ENTRIES = ('lvl_layernorm_fwd', 'lvl_layernorm_bwd', 'lvl_layernorm_apply', 'lvl_layernorm_fwd_mixed',
              'lvl_layernorm_bwd_mixed', 'lvl_droppath_add_layernorm_fwd', 'lvl_droppath_add_layernorm_bwd')


def _ln_case(name, rows, cols, rows_per_sample, dtypes, crosses):
    ops = tuple(Operand(f'x_{"f32" if e == F32 else "bf16"}', rows, cols, e, c) for e, c in zip(dtypes, crosses))
    tensors = [(rows, cols, max(dtypes), 8), (1 << 13, cols, 8, 12)]
    shape = dict(rows=rows, cols=cols, dtypes=dtypes, rows_per_sample=rows_per_sample)
    return Case(name, 'layernorm', LN_ENTRIES, shape, ops, ROW_UNROLL, tuple(tensors))


# rows_per_sample (lvl_droppath_add_layernorm_*) must divide the rows: 2^18 + 259 = 53 x 4951, 2^19 + 259 = 9 x 58 283,
# 699 309 = 39 x 17 931. The bf16 case runs to 2^19 rows: at 2^18 (past B31 only) no element index reaches 2^31, and the
# kernels index ELEMENTS; the float32 tensors of that row count would not fit the memory cap.
LN_CASES = (
    _ln_case('ln_4096_f32', (1 << 18) + 259, 4096, 53, (F32,), (('B31', 'B32'),)),
    _ln_case('ln_4096_bf16', (1 << 19) + 259, 4096, 9, (BF16,), (('B31', 'B32', 'E31'),)),
    _ln_case('ln_768_f32', ceil_div(B31, 768 * F32) + 258, 768, 39, (F32,), (('B31',),)),
)


# ---- vocabulary cross-entropy ---------------------------------------------------------------------------------------------
VOCAB = 50257


def _xent(rows, crosses):
    op = Operand('logits', rows, VOCAB, F32, crosses)
    tensors = [(rows, VOCAB, F32, 1), (rows, VOCAB + 7, F32, 2), (1 << 10, VOCAB, 8, 6)]
    return Case(f'xent_{rows}', 'xent', ('lvl_token_xent_fwd', 'lvl_token_xent_reduce', 'lvl_token_xent_bwd'),
                dict(rows=rows, vocab=VOCAB, T=100), (op,), 1, tuple(tensors))


# 42 800 rows (8.6 GB) are not in the issue's list: only there does `row * row_stride` pass 2^31 ELEMENTS
XENT_CASES = (_xent(10700, ('B31',)), _xent(21400, ('B31', 'B32')), _xent(42800, ('B31', 'B32', 'E31')))


# ---- gathers: patch matrix, token assembly, text embedding ----------------------------------------------------------------
def _gather(name, entry, shape, rows, cols, count=3):
    op = Operand('samples', rows, cols, F32, ('B31',))
    return Case(name, 'gather', entry, shape, (op,), 1, ((rows, cols, F32, count),))


PATCH_B = ceil_div(B31, 3 * 4 * 224 * 224 * F32) + 1          # clips of 4 x 3 x 224^2 float32
EMBED_B = ceil_div(B31, 785 * 768 * F32) + 1                  # clips of 1 + 4 x 196 tokens of 768 float32
TEXT_B = ceil_div(B31, 77 * 768 * F32) + 1                    # captions of 77 tokens of 768 float32
GATHER_CASES = (
    _gather('patchify', 'lvl_patchify', dict(B=PATCH_B, C=3, F=4, H=224, W=224), PATCH_B, 3 * 4 * 224 * 224),
    _gather('embed_tokens', ('lvl_embed_tokens_fwd', 'lvl_embed_tokens_bwd'), dict(B=EMBED_B, F=4, N=196, D=768),
            EMBED_B, 785 * 768),
    _gather('text_embed', ('lvl_text_embed_fwd', 'lvl_text_embed_bwd'), dict(B=TEXT_B, L=77, W=768, V=49408),
            TEXT_B, 77 * 768, count=4),
)

# ---- attention: one small exact problem (attention_problems), replicated ---------------------------------------------------
# (family, mode, shape of attention_problems' tables, element sizes): the smallest shapes whose groups fill the kernel family's
# tiles. divided: (B0, F, N, H); causal: (B0, -, L, H), the text tower's 77 tokens; cls: (B0, -, T, H). float32 at half
# the batch (the same bytes) where the family has a float32 instantiation: the MFMA time kernels have none
# (lvl_attention_fast_path_f32 answers 0 for 5 frames).
ATTN_SHAPES = (('space_resident', 'space', (2, 4, 32, 2), (BF16, F32)), ('space_streaming', 'space', (1, 1, 288, 1), (BF16, F32)),
               ('time_register', 'time', (1, 8, 9, 3), (BF16, F32)), ('time_mfma', 'time', (2, 5, 9, 4), (BF16,)),
               ('causal_text', 'causal', (3, 0, 77, 8), (BF16, F32)), ('cls_only', 'cls', (2, 0, 99, 2), (BF16, F32)))
ATTN_NO_F32 = (('time', 5, 9, 4),)


def _attn(name, mode, shape, esize):
    B0, F, N, H = shape
    T, D = (N if mode in ('causal', 'cls') else 1 + F * N), 64 * H
    width = (2 if mode == 'cls' else 3) * D                        # the large operand: qkv [B, T, 3D], cls: kv [B, T, 2D]
    B = (ceil_div(B32, T * width * esize) // B0 + 2) * B0          # whole replicas; the last one lies beyond B32 (bf16: E31)
    op = Operand('kv' if mode == 'cls' else 'qkv', B, T * width, esize, ('B31', 'B32', 'E31') if esize == BF16 else ('B31', 'B32'))
    # the operand, its gradient, a second gradient (the call without a bias) and a temporary; out / dout and friends; lse
    tensors = [(B, T * width, esize, 4), (B, T * D, esize, 4), (B * H, T, F32, 3)]
    entry = {'causal': ('lvl_causal_attn_fwd', 'lvl_causal_attn_bwd'), 'cls': ('lvl_cls_attn_fwd', 'lvl_cls_attn_bwd')}.get(
        mode, ('lvl_divided_attn_fwd', 'lvl_divided_attn_bwd', 'lvl_divided_attn_bwd_bias'))
    return Case(f'{name}_{"bf16" if esize == BF16 else "f32"}', 'attention', entry,
                dict(B=B, B0=B0, F=F, N=N, H=H, mode=mode, esize=esize, sample_bytes=T * width * esize), (op,), 1,
                tuple(tensors))


ATTN_CASES = tuple(_attn(n, m, sh, e) for n, m, sh, es in ATTN_SHAPES for e in es)


def replica_scales(r):
    """(c_v, c_dout) of replica r: signs and powers of two in {+-1/2, +-1, +-2} from a hash of r (no period a wrapped
    offset could land on): the expected results scale exactly -- out by c_v, dv by c_dout, dq and dk by both"""
    h = (r * 2654435761 + 0x9E3779B9) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 2246822519) & 0xFFFFFFFF
    h ^= h >> 13
    vals = (0.5, 1.0, 2.0, -0.5, -1.0, -2.0)
    return vals[h % 6], vals[(h >> 8) % 6]


ALL_CASES = TN_CASES + WGRAD_CASES + ROWS_CASES + LN_CASES + XENT_CASES + GATHER_CASES + ATTN_CASES


# ---- host routing: the fused MLP (768 -> 3072, bf16) on both sides of the _tn_ok gate --------------------------------------
MLP_WIDTHS = (768, 3072)
MLP_ROWS = {'below_gate': ceil_div(B32, 2 * 3072) - 256,      # one 256-row tile below: lvl_linear_tn / lvl_linear_wgrad throughout
            'at_gate': ceil_div(B32, 2 * 3072)}               # the library GEMM, the own element-wise kernels on > 2^31 elements


def mlp_peak_bytes(rows):
    """x, dx, dy, y [rows, 768] and u, a, da, du, one temporary [rows, 3072] in bf16, plus the float64 reference's chunk"""
    return rows * 768 * BF16 * 4 + rows * 3072 * BF16 * 5 + (1 << 15) * (3072 + 768) * 8 * 4


# ---- host gates of lavila_amd/ops.py --------------------------------------------------------------------------------------
# (predicate, (rows, n_out, n_in), value): every gate one row below its limit and at it, and at the case shapes.
# The fused MLP of the towers (768 -> 3072): the own GEMMs take rows * 3072 * 2 < 2^32.
MLP_GATE_ROWS = ceil_div(B32, 2 * 3072)           # 699 051: the first row count the library GEMM serves
GATES = (
    ('_tn_ok', (MLP_GATE_ROWS - 1, 3072, 768), True), ('_tn_ok', (MLP_GATE_ROWS, 3072, 768), False),
    ('_tn_ok', (MLP_GATE_ROWS - 1, 768, 3072), True), ('_tn_ok', (MLP_GATE_ROWS, 768, 3072), False),
    ('_tn_ok', (M_X32, 256, 4096), True), ('_tn_ok', (M_X32 + 1, 256, 4096), False),
    ('_tn_ok', (M_WRAP, 256, K_WRAP), True), ('_tn_ok', (M_WRAP + 1, 256, K_WRAP), False),
    # the gate also counts y (n_out): the entry point itself takes M_Y x 4096 (64-bit output offsets), the host does not
    ('_tn_ok', (M_Y, 4096, 64), False), ('_tn_ok', ((1 << 19) - 1, 4096, 64), True), ('_tn_ok_f32', (M_Y, 4096, 192), False),
    ('_tn_ragged_ok', (M_X31, N_RAGGED, 4096), True), ('_tn_ragged_ok', (M_X32, N_RAGGED, 4096), True),
    ('_tn_ragged_ok', (M_X32 + 1, N_RAGGED, 4096), False), ('_tn_ragged_ok', (M_RAGGED_Y, N_RAGGED, 64), False),
    ('_tn_ok_f32', (ceil_div(B32, 6 * 768) - 1, 768, 768), True), ('_tn_ok_f32', (ceil_div(B32, 6 * 768), 768, 768), False),
    ('_wgrad_f32_ok', (ceil_div(B32, 6 * 768) - 1, 768, 768), True), ('_wgrad_f32_ok', (ceil_div(B32, 6 * 768), 768, 768), False),
    ('_wgrad_f32_ok', (ceil_div(B32, 6 * 3072) - 1, 3072, 768), True), ('_wgrad_f32_ok', (ceil_div(B32, 6 * 3072), 768, 3072), False),
    # the skinny GEMMs stop at 2^31 bytes (their kernels index with 64 bits; nothing above is tested, so the gate stays)
    ('_skinny_ok', (ceil_div(B31, 2 * 768) - 1, 128, 768), True), ('_skinny_ok', (ceil_div(B31, 2 * 768), 128, 768), False),
    ('_skinny_f32_ok', (ceil_div(B31, 12 * 96) - 1, 48, 96), True), ('_skinny_f32_ok', (ceil_div(B31, 12 * 96), 48, 96), False),
)
