"""GPU (-m gpu): the MFMA-shape policy of the persistent TN GEMM (lvl_linear_tn, bf16 results, epilogues 0-5): the K loop on
v_mfma_f32_16x16x32_bf16 (gemm_tn_mfma16 in csrc/gemm_tn_kernel.h) beside the one on v_mfma_f32_32x32x16_bf16, selected through
lvl_set_gemm_mfma_shape. The shape changes the fragment reads, the MFMAs of a phase and the accumulator map of the epilogue
(16-row groups, four 8-byte pieces of a row widened by permlane16_swap, column sums over 16 lanes); everything here runs under
BOTH shapes, through the setter, and restores the default.

  * an output matrix at the smallest shapes at which that code can go wrong: one and three column tiles, nb = 1, 2, 3 and 5
    K blocks per tile (5: the only nb below 6 that the dynamic schedule admits), one and six full tile rows plus a remainder
    on either side of every 16-row boundary of the first 48 rows (15, 16, 17, 31, 33, 48), the one-row and all-but-one-row
    tails and the remainder-0 control -- the checkers, bounds and guards of gemm_tn_cases.py, unchanged;
  * the GM_AUDIT build with shape 16 selected: bit-equal outputs, store counts, fill order, exact waits;
  * the setter's refusals, and the f32-class launches staying where they were.
"""
import pytest
import torch

import gemm_tn_cases as G
from gemm_tn_cases import DEV, LATE_MOD
from helpers import launch_config as _launch_config

pytestmark = pytest.mark.gpu

NS_ = (256, 768)
KS = (64, 128, 192, 320)
TILE_ROWS = (1, 6)
REMAINDERS = (0, 1, 15, 16, 17, 31, 33, 48, 255)
BF16_KERNELS = G.kb_kernels('bf16')
NO_CHECK = 0x7fffffff


@pytest.fixture()
def shape_setter():
    """set(shape) on the product library and on every library handed in later; the default is restored in any case"""
    from lavila_amd import _cabi as C
    libs = [C.lib()]

    def set_shape(shape, *more):
        for lib in more:
            if lib not in libs:
                libs.append(lib)
        for lib in libs:
            assert lib.lvl_set_gemm_mfma_shape(shape) == 0
    try:
        yield set_shape
    finally:
        for lib in libs:
            assert lib.lvl_set_gemm_mfma_shape(0) == 0


@pytest.fixture(scope='module')
def audit_lib(tmp_path_factory):
    return G.build_audit_library(tmp_path_factory.mktemp('gm_audit'))


def _operands(N, K, t, rem):
    M = 256 * t + rem
    d = G.case_data(N, M, 1000 * N + 8 * K + 3 * t + rem, K, None)
    di = G.kblock_int_data(N, M, 7 * N + rem + K + t, 'bf16', K, DEV)
    di['u'] = d['u']              # epilogue 2's pre-activation rows: any values (its products are not integers)
    return M, d, di


@pytest.mark.parametrize('N,K,t,rem', [(n, k, t, r) for n in NS_ for k in KS for t in TILE_ROWS for r in REMAINDERS])
def test_both_mfma_shapes_vs_float64_and_exactly(shape_setter, N, K, t, rem):
    """every bf16 kernel of lvl_linear_tn at one (N, K, M = 256 t + rem), under shape 16 and shape 32: the float64 bounds of
    check_random_vs_float64 on random operands; equality on integer operands in which every K block counts; the two shapes
    bit-equal to each other on the integer operands AND on the random ones, column sums and their partial slabs included
    (the MFMAs of the two shapes return the same accumulators for the same K block -- measured, not documented -- and the
    16x16 map forms its column sums in the order of the 32x32 one: that the step computes what it computed on 32x32x16
    rests on exactly this); and within shape 16 bit-equality under 8 / 16 / all CUs x the schedules the nb admits,
    with NaN/Inf rows behind inputs and aux tensors, sentinel rows behind the outputs, NaN-poisoned column-sum outputs and
    workspace, and the counter block zero afterwards (asserted inside gemm_tn_cases.tn)"""
    from lavila_amd import _cabi as C
    lib = C.lib()
    M, d, di = _operands(N, K, t, rem)
    assert G.check_every_block_counts(di, 'bf16') == 1.0
    base, ints = {}, {}
    for shape in (16, 32):
        shape_setter(shape)
        for kern in BF16_KERNELS:
            out = G.tn(lib, kern, d, 'static', guard=False)
            G.check_random_vs_float64(kern, out, d)
            got = G.tn(lib, kern, di, 'static', guard=True)
            G.check_integers(kern, got, di)
            base[shape, kern[0]], ints[shape, kern[0]] = out, got
    for kern in BF16_KERNELS:
        assert G.same(ints[16, kern[0]], ints[32, kern[0]]), (kern[0], 'the shapes differ on exact operands')
        assert G.same(base[16, kern[0]], base[32, kern[0]]), (kern[0], 'the shapes differ on random operands')
    shape_setter(16)
    for cus, sched in G.kb_configs('bf16', K):
        with _launch_config([lib], cus, LATE_MOD if sched == 'late' else 0):
            for kern in BF16_KERNELS:
                got = G.tn(lib, kern, d, sched, guard=True)
                assert G.same(got, base[16, kern[0]]), (kern[0], K, M, cus, sched)
            if cus == 8:
                for kern in BF16_KERNELS:
                    G.check_integers(kern, G.tn(lib, kern, di, sched, guard=True), di)


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('rem', (0, 17))
def test_audit_build_on_shape_16(shape_setter, audit_lib, K, rem):
    """GM_AUDIT build with shape 16 selected explicitly in both libraries (N = 768, six tile rows and a remainder: at 8 CUs a
    workgroup walks two or three tiles): outputs bit-equal to the product library's; full tiles issue exactly the expected
    number of stores (gemm_tn_cases.ns: the same 16 / 32 (+ 1) per wave as shape 32) and use the full allowance, no record
    with allowance > stores issued; no fill-order violation, no negative margin; and the tightest margin is EXACTLY 0 in
    some wave other than wave 0 of a workgroup with at least two tiles, for every kernel (the waits are exact: see
    test_gpu_gemm_kblocks.py)"""
    from lavila_amd import _cabi as C
    lib = C.lib()
    shape_setter(16, audit_lib)
    N, M = 768, 256 * 6 + rem
    d = G.case_data(N, M, 31 * K + rem, K, None)
    tiles_m = (M + 255) // 256
    want = {kern[0]: G.tn(lib, kern, d, 'static', guard=False) for kern in BF16_KERNELS}
    exact = {kern[0]: 0 for kern in BF16_KERNELS}
    for cus, sched in G.kb_configs('bf16', K):
        for kern in BF16_KERNELS:
            out, r, h = G.audit_run(audit_lib, kern, d, cus, sched)
            where = (kern[0], K, M, cus, sched)
            assert G.same(out, {k: v for k, v in want[kern[0]].items() if k != 'colsum'}), where
            ns, full = G.ns(kern)
            tail = (r[:, 0] + 1) * 256 > M
            assert bool((r[:, 0] < tiles_m).all()) and bool((r[:, 1] < N // 256).all()), where
            assert bool((r[~tail, 2] == full).all()), where + ('full-tile store count',)
            assert bool((r[~tail, 3] == ns).all()), where
            assert int((r[:, 3] > r[:, 2]).sum()) == 0, where + ('allowance > stores issued',)
            bad = torch.nonzero(h[:, 1]).flatten().tolist()
            assert not bad, where + tuple(f'workgroup {row // 8} wave {row % 8}: ' + G.decode_violation(int(h[row, 2]))
                                          for row in bad[:4])
            checked = h[:, 3] != NO_CHECK
            assert int((h[checked, 3] < 0).sum()) == 0, where
            wave = torch.arange(len(h)) % 8
            exact[kern[0]] += int(((wave != 0) & (h[:, 0] >= 1) & (h[:, 3] == 0)).sum())
    for kern in BF16_KERNELS:
        assert exact[kern[0]] > 0, (kern[0], K, M, 'no wave with an exact wait')


def test_setter_refuses_other_values_and_leaves_f32_class_alone(shape_setter):
    """lvl_set_gemm_mfma_shape takes 0, 16 and 32 and nothing else (a refused value changes nothing); the f32-class launches
    run the same kernel whatever is set: bit-equal results on random operands under 16, 32 and the default"""
    from lavila_amd import _cabi as C
    lib = C.lib()
    N, M, K = 256, 256 * 2 + 17, 128
    d = G.case_data(N, M, 5, 64, K)
    bias = BF16_KERNELS[0]
    shape_setter(32)
    want32 = G.tn(lib, bias, d, 'static', guard=True)
    for bad in (-1, 1, 8, 15, 17, 31, 48, 64, 1 << 20):
        assert lib.lvl_set_gemm_mfma_shape(bad) == -22                             # LVL_EINVAL
        assert b'set_gemm_mfma_shape' in lib.lvl_last_error()
        assert G.same(G.tn(lib, bias, d, 'static', guard=True), want32), bad       # still on shape 32
    f32 = G.kb_kernels('f32')
    outs = {}
    for shape in (16, 32, 0):
        shape_setter(shape)
        for kern in f32:
            outs[shape, kern[0]] = G.tn(lib, kern, d, 'static', guard=True)
            G.check_random_vs_float64(kern, outs[shape, kern[0]], d)
    for kern in f32:
        assert G.same(outs[16, kern[0]], outs[32, kern[0]]) and G.same(outs[0, kern[0]], outs[32, kern[0]]), kern[0]
