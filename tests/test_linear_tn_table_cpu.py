"""lvl_linear_tn / lvl_linear_tn_ragged on the host: what they refuse, and the epilogue table of _cabi.py.

  * the refusal matrix: every epilogue 0..8 and -1, 9 in both dtypes on both entries, each call valid but for ONE thing (the
    ragged entry in float32 with an epilogue it does not take breaks two rules: it pins the precedence, dtype first). Status
    and message substring of every case stand below as data, recorded from the library before its checks were folded into
    one table and one shared argument check (csrc/gemm_tn_kernel.h: kTnEpilogues, tn_check_args). No case is valid, so
    nothing launches: the pointers are made-up aligned addresses that are never dereferenced
    (as test_clip_loss_reference_cpu.py's), and the test needs no GPU;
  * the table of _cabi.py (TN_EPILOGUES) against the LVL_EPI_* enum of include/lavila_hip.h, and the sets ops.py derives from it
    against their members before they were derived.
"""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOSYS = -22, -38
F32, BF16 = 0, 1
ALL = tuple(range(9))
F32_EPIS = (0, 1, 2, 3, 6, 7)                   # the epilogues of the f32-class mode
M, N, K = 40, 256, 192                          # one partial tile; K serves both modes (64s, and 3 x 64)
M_4GIB = -(-(1 << 32) // (2 * K))               # the first M with M * K * 2 >= 2^32
PTRS = dict(x=0x10000, w=0x20000, bias=0x30000, y=0x40000, aux_out=0x50000, aux_in=0x60000, colsum=0x70000, ws=0x80000)

# (fault, {dtype: epilogues}, status, substring of lvl_last_error) for lvl_linear_tn
TN = [
    ('no_aux_out', {BF16: (1, 4, 6, 8), F32: (1, 6)}, EINVAL, 'aux_out'),
    ('no_aux_in', {BF16: (2, 3, 5, 7), F32: (2, 3, 7)}, EINVAL, 'aux_in'),
    ('no_colsum', {BF16: (2, 5, 7), F32: (2, 7)}, EINVAL, 'colsum and a workspace'),
    ('no_ws', {BF16: (2, 5, 7), F32: (2, 7)}, EINVAL, 'colsum and a workspace'),
    ('odd_ws', {BF16: (2, 5, 7), F32: (2, 7)}, EINVAL, 'colsum and a workspace'),
    ('odd_x', {BF16: ALL, F32: F32_EPIS}, EINVAL, 'aligned'),
    ('odd_w', {BF16: ALL, F32: F32_EPIS}, EINVAL, 'aligned'),
    ('odd_y', {BF16: ALL, F32: F32_EPIS}, EINVAL, 'aligned'),
    ('odd_bias', {BF16: ALL, F32: F32_EPIS}, EINVAL, 'aligned'),
    ('odd_aux_out', {BF16: ALL, F32: F32_EPIS}, EINVAL, 'aligned'),
    ('odd_aux_in', {BF16: ALL, F32: F32_EPIS}, EINVAL, 'aligned'),
    ('n_320', {BF16: ALL, F32: F32_EPIS}, ENOSYS, 'no tiling'),
    ('k_96', {BF16: ALL, F32: F32_EPIS}, ENOSYS, 'no tiling'),
    ('k_256', {F32: F32_EPIS}, EINVAL, 'not 3 x a multiple of 64'),
    ('m_4gib', {BF16: ALL, F32: F32_EPIS}, ENOSYS, '4 GiB'),
    ('none', {F32: (4, 5, 8)}, ENOSYS, 'bf16 epilogue'),
    ('none', {BF16: (-1, 9), F32: (-1, 9)}, EINVAL, 'unknown epilogue'),
    ('no_x', {BF16: (0,), F32: (0,)}, EINVAL, 'null pointer'),
    ('m_0', {BF16: (0,), F32: (0,)}, EINVAL, 'empty problem'),
    ('dtype_7', {BF16: (0,)}, EINVAL, 'unknown dtype'),
]
# the same for lvl_linear_tn_ragged (N = 320: one full tile and 64 edge columns)
RAGGED = [
    ('none', {BF16: tuple(range(1, 9))}, ENOSYS, 'LVL_EPI_BIAS only'),
    ('none', {BF16: (-1, 9)}, EINVAL, 'unknown epilogue'),
    ('none', {F32: (-1,) + ALL + (9,)}, ENOSYS, 'bf16 only'),
    ('odd_x', {BF16: (0,)}, EINVAL, 'aligned'),
    ('odd_w', {BF16: (0,)}, EINVAL, 'aligned'),
    ('odd_y', {BF16: (0,)}, EINVAL, 'aligned'),
    ('odd_bias', {BF16: (0,)}, EINVAL, 'aligned'),
    ('n_300', {BF16: (0,)}, ENOSYS, 'N % 64 == 0 and K % 64 == 0'),
    ('k_96', {BF16: (0,)}, ENOSYS, 'no tiling'),
    ('m_4gib', {BF16: (0,)}, ENOSYS, '4 GiB'),
    ('no_x', {BF16: (0,)}, EINVAL, 'null pointer'),
    ('m_0', {BF16: (0,)}, EINVAL, 'empty problem'),
    ('dtype_7', {BF16: (0,)}, EINVAL, 'unknown dtype'),
]


def _cases(table, entry):
    for fault, by_dtype, status, text in table:
        for dtype, epilogues in by_dtype.items():
            for e in epilogues:
                yield pytest.param(entry, fault, dtype, e, status, text, id=f'{entry}-{fault}-{"f32" if dtype == F32 else "bf16"}-epi{e}')


def _call(lib, entry, fault, dtype, epilogue):
    p = dict(PTRS)
    m, n, k = M, (320 if entry == 'ragged' else N), K
    kind, _, what = fault.partition('_')
    if kind == 'no':
        p[what] = None
    elif kind == 'odd':
        p[what] += 8
    elif kind == 'n':
        n = int(what)
    elif kind == 'k':
        k = int(what)
    elif fault == 'm_4gib':
        m = M_4GIB
    elif fault == 'm_0':
        m = 0
    elif fault == 'dtype_7':
        dtype = 7
    else:
        assert fault == 'none', fault
    v = {name: (None if a is None else ctypes.c_void_p(a)) for name, a in p.items()}
    if entry == 'ragged':
        return lib.lvl_linear_tn_ragged(v['x'], v['w'], v['bias'], v['y'], None, m, n, k, epilogue, dtype, None)
    return lib.lvl_linear_tn(v['x'], v['w'], v['bias'], v['y'], v['aux_out'], v['aux_in'], v['colsum'], v['ws'], None, m, n, k,
                             epilogue, dtype, None)


@pytest.mark.parametrize('entry,fault,dtype,epilogue,status,text', [*_cases(TN, 'tn'), *_cases(RAGGED, 'ragged')])
def test_refusal_matrix(entry, fault, dtype, epilogue, status, text):
    from lavila_amd import _cabi as C
    lib = C.lib()
    rc = _call(lib, entry, fault, dtype, epilogue)
    msg = lib.lvl_last_error().decode()
    assert rc == status and text in msg, (rc, msg)
    assert msg.startswith('linear_tn_ragged' if entry == 'ragged' else 'linear_tn')


def test_matrix_covers_every_epilogue_in_both_dtypes_on_both_entries():
    for table in (TN, RAGGED):
        seen = {(d, e) for _, by_dtype, _, _ in table for d, es in by_dtype.items() for e in es}
        assert seen == {(d, e) for d in (F32, BF16) for e in range(-1, 10)}


def test_cabi_epilogue_table_is_the_header_enum_and_the_derived_sets_keep_their_members():
    from lavila_amd import _cabi as C
    from lavila_amd import ops
    header = open(os.path.join(ROOT, 'include', 'lavila_hip.h')).read()
    enum = {name: int(v) for name, v in re.findall(r'LVL_(EPI_\w+) = (\d+)', header)}
    assert len(enum) == 9 and sorted(enum.values()) == list(range(9))
    assert {name: row[0] for name, row in C.TN_EPILOGUES.items()} == enum
    assert all(getattr(C, name) == code for name, code in enum.items())
    assert tuple(ops._TN_TWO_OUT) == (1, 4, 6, 8) and tuple(ops._TN_COLSUM) == (2, 5, 7)
    assert ops._MLP_EPILOGUES == {'quickgelu': (1, 4, 2), 'gelu': (6, 8, 7)}
    # f32: the epilogues of the f32-class mode, as the matrix above has them from the library
    assert tuple(code for code, _, _, f32 in C.TN_EPILOGUES.values() if f32) == F32_EPIS
