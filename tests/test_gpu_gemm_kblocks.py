"""GPU (-m gpu): the persistent TN GEMM (lvl_linear_tn) over the K axis: nb = K / 64 = 1 .. 8 K blocks per tile for the bf16
kernels, nb = 3 and 9 for the f32-class ones (test_gpu_gemm_tails.py holds the M axis at nb = 5 / 6).

The kernel never drains at a tile boundary, fetches two K blocks ahead of the one it multiplies and counts every vmcnt wait
by hand, so what a barrier waits for depends on nb: the blocks behind an epilogue (`k_block(IS, IS); if (nb > 1) ...`), the
fetch cursor that wraps every block at nb = 1 and then runs two tiles ahead, the past-the-end re-read of block nb - 1, the
ring of four bias images that is only full at nb = 1, the ring half a tile starts on (odd / even nb), the epilogues' re-read
of the next tile's first fragments, and DYN_MIN_NB = 5 as the only nb the dynamic schedule was run at.

  * an output matrix (test_linear_tn_k_blocks_...): every kernel, five row remainders, 8 / 16 / all compute units (6 / 3 / 1
    tiles per workgroup) on every schedule the nb admits -- float64 bounds on random operands, equality on integers built so
    that EVERY K block counts (gemm_tn_cases.kblock_int_data), bit-equality across CU counts and schedules, guards;
  * the fill-order audit of the GM_AUDIT build (test_fill_order_audit_...): an output comparison cannot see a wait that is
    too loose (the fill has usually landed anyway). The audit build numbers the vector-memory operations every wave issues
    and checks at every barrier that the fill it waits for is older than the operations the wait leaves in flight
    (csrc/gemm_tn_mfma.hip, GM_AUDIT). No timing is involved, and no wrong kernel is run: the check is non-vacuous because
    the kernel's waits are EXACT -- the tightest margin a wave sees must be 0, not merely >= 0.
"""
import pytest
import torch

import gemm_tn_cases as G
from gemm_tn_cases import DEV, LATE_MOD
from helpers import launch_config as _launch_config

NO_CHECK = 0x7fffffff         # margin of a wave that made no check (a late workgroup)


def _case(mode, K, N, rem):
    M = G.kb_rows(N, rem)
    d = G.case_data(N, M, 1000 * N + 8 * K + rem, K if mode == 'bf16' else None, K if mode == 'f32' else None)
    return M, d


@pytest.fixture(scope='module')
def audit_lib(tmp_path_factory):
    return G.build_audit_library(tmp_path_factory.mktemp('gm_audit'))


@pytest.mark.gpu
@pytest.mark.parametrize('mode,K,N,rem', G.KB_CASES)
def test_linear_tn_k_blocks_vs_float64_on_every_schedule(mode, K, N, rem):
    """every kernel of the mode at one (K, N, row remainder): what test_linear_tn_tail_tiles_vs_float64_on_every_schedule
    asserts -- the float64 bounds of check_random_vs_float64 on random operands, equality on small integers, bit-equality
    under 8 / 16 / all CUs x the schedules of the nb (static alone below DYN_MIN_NB, where a counter block handed in must
    change nothing and stay zero), NaN/Inf rows behind the inputs, sentinel rows behind the outputs, NaN-poisoned column-sum
    outputs and workspace, counter block zero afterwards -- with integer operands in which every K block counts"""
    from lavila_amd import _cabi as C
    from lavila_amd import ops
    lib = C.lib()
    M, d = _case(mode, K, N, rem)
    di = G.kblock_int_data(N, M, 7 * N + rem + K, mode, K, DEV)
    assert G.check_every_block_counts(di, mode) == 1.0
    if mode == 'f32':         # the term images the reference was computed from are the ones the library's split makes
        assert torch.equal(ops.split3(di['xf'], 0), di['x3']) and torch.equal(ops.split3(di['wf'], 1), di['w3'])
    base = {}
    for kern in G.kb_kernels(mode):
        base[kern[0]] = G.tn(lib, kern, d, 'static', guard=False)
        G.check_random_vs_float64(kern, base[kern[0]], d)
        if kern[1] != 2 and kern[1] != 4:
            G.check_integers(kern, G.tn(lib, kern, di, 'static', guard=True), di)
    for cus, sched in G.kb_configs(mode, K):
        with _launch_config([lib], cus, LATE_MOD if sched == 'late' else 0):
            for kern in G.kb_kernels(mode):
                got = G.tn(lib, kern, d, sched, guard=True)         # (asserts the guards and the counter block)
                assert G.same(got, base[kern[0]]), (kern[0], K, M, cus, sched)
            if cus == 8:
                # the exact check where one workgroup walks six tiles back to back
                for kern in G.kb_kernels(mode):
                    if kern[1] != 2 and kern[1] != 4:
                        G.check_integers(kern, G.tn(lib, kern, di, sched, guard=True), di)


@pytest.mark.gpu
@pytest.mark.parametrize('mode,K,N,rem', G.KB_CASES)
def test_fill_order_audit_over_the_k_axis(audit_lib, mode, K, N, rem):
    """GM_AUDIT build, every kernel and configuration of one (K, N, row remainder):
      * its outputs are bit-equal to the product library's;
      * the store-count invariant of test_counted_waits_never_exceed_the_stores_issued: allowance <= stores issued, full
        tiles issue exactly the expected count and use the full allowance;
      * no wave reports a fill-order violation: at every barrier the fills of the slot the next phase reads, at init_acc the
        bias image, at publish the counter reply, at the epilogue's re-read both slots, are older than everything the last
        vmcnt wait left in flight;
      * margins: the tightest `completed - awaited` a wave saw is >= 0 everywhere, and EXACTLY 0 in some wave other than
        wave 0 of a workgroup with at least two tiles, for every kernel. The kernel's comment gives the waits as exact
        (N = the operations issued behind the slot's fills: 10 / 8 / 10 / 10, plus NS stores behind a full tile), and a wave
        other than wave 0 issues nothing but its fills and stores, all of which the audit counts -- so a margin that is
        positive everywhere would mean the audit miscounts (or a wait stricter than documented), and a check that cannot
        fail would show as one. f32-class kernels: the blocks behind an epilogue wait for its stores too (no allowance,
        positive margin there), their other blocks are exact like the bf16 ones."""
    from lavila_amd import _cabi as C
    lib = C.lib()
    M, d = _case(mode, K, N, rem)
    nb = G.kb_blocks(mode, K)
    tiles_m = (M + 255) // 256
    want = {kern[0]: G.tn(lib, kern, d, 'static', guard=False) for kern in G.kb_kernels(mode)}
    exact = {kern[0]: 0 for kern in G.kb_kernels(mode)}        # waves (not wave 0, >= 2 tiles) with margin exactly 0
    low = {kern[0]: NO_CHECK for kern in G.kb_kernels(mode)}
    bad_store, bad_fill, negative = [], [], 0
    for cus, sched in G.kb_configs(mode, K):
        for kern in G.kb_kernels(mode):
            out, r, h = G.audit_run(audit_lib, kern, d, cus, sched)
            where = (kern[0], f'nb={nb}', f'M={M}', f'cus={cus}', sched)
            assert G.same(out, {k: v for k, v in want[kern[0]].items() if k != 'colsum'}), where
            ns, full = G.ns(kern)
            tail = (r[:, 0] + 1) * 256 > M
            assert bool((r[:, 0] < tiles_m).all()) and bool((r[:, 1] < N // 256).all()), where
            assert bool((r[~tail, 2] == full).all()), where + ('full-tile store count',)
            assert bool((r[~tail, 3] == ns).all()), where
            if int((r[:, 3] > r[:, 2]).sum()):
                bad_store.append(where + (int((r[:, 3] > r[:, 2]).sum()), len(r)))
            for row in torch.nonzero(h[:, 1]).flatten().tolist():
                bad_fill.append(where + (f'workgroup {row // 8} wave {row % 8}: {int(h[row, 1])} violations, first: '
                                         + G.decode_violation(int(h[row, 2])),))
            checked = h[:, 3] != NO_CHECK
            negative += int((h[checked, 3] < 0).sum())
            multi = checked & (h[:, 0] >= 1)                     # waves of workgroups that ran at least two tiles
            if bool(multi.any()):
                low[kern[0]] = min(low[kern[0]], int(h[multi, 3].min()))
            wave = torch.arange(len(h)) % 8
            exact[kern[0]] += int(((wave != 0) & (h[:, 0] >= 1) & (h[:, 3] == 0)).sum())
    assert not bad_store, f'records with slack > issued: {bad_store}'
    assert not bad_fill, 'fill-order violations:\n' + '\n'.join(str(b) for b in bad_fill)
    assert negative == 0                                         # (a negative margin is a violation: reported above)
    print(f'\n[gemm_tn fill-order audit] {mode} nb={nb} N={N} M={M}: tightest margin (workgroups with >= 2 tiles) {low}, '
          f'waves at margin 0 {exact}')
    for kern in G.kb_kernels(mode):
        assert exact[kern[0]] > 0, (kern[0], nb, M, 'no wave with an exact wait: tightest margin', low[kern[0]])
