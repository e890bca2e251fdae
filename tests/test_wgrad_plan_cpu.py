"""CPU: the plans of lvl_linear_wgrad (make_plan / row_plan, through lvl_linear_wgrad_plan), the kernel's block decode
(lvl_linear_wgrad_pair_of_block) and the case table of test_gpu_wgrad_configs.py.

  * invariants of every plan over a sweep of widths, CU limits and row counts: the launch fits the workspace, the compute
    units and the counter block that were sized without knowing M; the row plan deals every full row block exactly once,
    in chunks of an even length none of which is empty or starts behind the unit;
  * the block decode is a bijection for every number of pairs it is launched with;
  * every row of the case table reaches the configuration it names (13 of 13, one-chunk and multi-chunk / multi-split),
    and the late-workgroup settings the GPU test uses leave every tile with a workgroup that computes it.
"""
import ctypes

import wgrad_cases as W

WIDTHS = sorted({d for b in (96, 128, 160) for d in range(b, 6401, b)})
CU_LIMITS = (8, 16, 24, 32, 104, 0)
ROWS = (0, 1, 31, 32, 33, 1535, 1536, 3100, 9631, 19201, 40001, 200960)


def _lib():
    from lavila_amd import _cabi as C
    return C.lib()


def test_plan_invariants_over_widths_cu_limits_and_rows():
    lib = _lib()
    out = (ctypes.c_int * len(W.FIELDS))()
    query = lib.lvl_linear_wgrad_plan
    plans = launches = 0
    for cus in CU_LIMITS:
        with W.compute_units(lib, cus):
            n_cus = cus or 256          # no device: the library plans for 256 compute units
            if not cus:
                # the device's own count, read off a plan no limit can shrink: 160 x 160 is one tile, S(0) = the CUs
                p = W.plan(lib, 0, 160, 160)
                n_cus = p['S']
                assert n_cus >= 104 and p['ntiles'] == 1
            for N in WIDTHS:
                for K in WIDTHS:
                    rc = query(0, N, K, out)
                    ws = lib.lvl_workspace_floats(b'linear_wgrad', N, K)
                    if rc == W.ENOSYS:
                        assert ws == -1, (cus, N, K)
                        continue
                    assert rc == 0, (cus, N, K, rc)
                    cfg0, tk0, nt0, S0 = out[0], out[1], out[2], out[3]
                    assert list(out[4:9]) == [0] * 5, (cus, N, K)
                    assert ws == S0 * N * K + S0 * N, (cus, N, K)         # partial slabs of dW and of dbias
                    plans += 1
                    for M in ROWS[1:]:
                        assert query(M, N, K, out) == 0, (cus, N, K, M)   # a plan for M > 0 wherever one exists for M = 0
                        cfg, tiles_k, ntiles, S, base, rem, L, nch0, nch1 = out
                        wn, wk, ta, tb = W.CFGS[cfg]
                        tn, tk = 16 * ta * wn, 16 * tb * wk
                        key = (cus, N, K, M, list(out))
                        assert N % tn == 0 and K % tk == 0 and tiles_k == K // tk and ntiles == (N // tn) * tiles_k, key
                        assert 1 <= S <= S0, key                          # the partial slabs stay inside the workspace
                        assert ntiles * S <= n_cus, key                   # one resident workgroup per compute unit
                        assert cfg >= W.FIRST_160 or ntiles * S % 8 == 0, key     # whole XCD rounds (older decode)
                        assert ntiles * S + ntiles + 1 <= W.COUNTER_WORDS, key    # unit counters | tile counts | sign-offs
                        assert S * base + rem == M // 32 and 0 <= rem < S, key
                        assert L >= 2 and L % 2 == 0, key
                        for ulen, nch in ((base, nch0), (base + 1, nch1)):
                            assert (nch - 1) * L < ulen <= nch * L, key   # no empty chunk, none starts behind the unit
                        launches += 1
    assert plans > 4000 and launches == plans * (len(ROWS) - 1)


def test_plan_entry_rejects_what_it_cannot_answer():
    lib = _lib()
    out = (ctypes.c_int * 9)()
    assert lib.lvl_linear_wgrad_plan(0, 768, 768, None) == -22
    assert lib.lvl_linear_wgrad_plan(-1, 768, 768, out) == -22
    assert lib.lvl_linear_wgrad_plan(0, 0, 768, out) == -22
    for N, K in ((200, 768), (1600, 1632), (50432, 1600)):
        assert lib.lvl_linear_wgrad_plan(4096, N, K, out) == W.ENOSYS and lib.lvl_linear_wgrad_plan(0, N, K, out) == W.ENOSYS
    for cfg, pairs, bid in ((-1, 8, 0), (13, 8, 0), (0, 0, 0), (0, 8, 8), (0, 8, -1)):
        assert lib.lvl_linear_wgrad_pair_of_block(cfg, pairs, bid) < 0, (cfg, pairs, bid)


def test_block_decode_is_a_bijection():
    """pair_of_block maps the block ids [0, P) onto the pairs [0, P): every (split, tile) unit has exactly one workgroup.
    The older family is launched with multiples of 8 only (make_plan), the 160 family with any P. Every configuration
    of a family decodes alike."""
    lib = _lib()
    f = lib.lvl_linear_wgrad_pair_of_block
    for cfg in range(len(W.CFGS)):
        step = 8 if cfg < W.FIRST_160 else 1
        sizes = range(step, 305, step) if cfg in (0, W.FIRST_160) else (8, 48, 152, 256, 304)
        for P in sizes:
            assert sorted(f(cfg, P, bid) for bid in range(P)) == list(range(P)), (cfg, P)
    for P in (1, 2, 5, 6, 7, 9, 150, 303):
        ref = [f(W.FIRST_160, P, bid) for bid in range(P)]
        assert all([f(cfg, P, bid) for bid in range(P)] == ref for cfg in range(W.FIRST_160, len(W.CFGS))), P
    # XCD x = bid % 8 owns a contiguous range of pairs, in XCD order
    for cfg, P in ((0, 48), (5, 256), (8, 150), (11, 6), (12, 13)):
        owned = [sorted(f(cfg, P, bid) for bid in range(x, P, 8)) for x in range(8)]
        assert [v for o in owned for v in o] == list(range(P)), (cfg, P)


def test_case_table_reaches_every_configuration():
    """every row lands on the configuration it names -- at M, M + 1 and M + 31 --, 'one' rows with a single chunk per unit
    at the device's CU count, 'multi' rows with S >= 2 and >= 3 chunks per unit; 13 of 13 configurations in both kinds"""
    lib = _lib()
    seen = {'one': set(), 'multi': set()}
    for c in W.CASES:
        assert c.M % 32 == 0 and c.kind in seen
        with W.compute_units(lib, c.cus):
            got = [W.plan(lib, c.M + r, c.N, c.K) for r in W.REMAINDERS]
            ws = W.plan(lib, 0, c.N, c.K)
        assert all(p is not None and p == got[0] for p in got), (c, got)
        p = got[0]
        assert p['cfg'] == c.cfg, (c, p)
        assert p['S'] <= ws['S'], (c, p, ws)
        if c.kind == 'one':
            assert c.cus == 0 and p['nch0'] == 1 and W.chunks(p) == 1, (c, p)
        else:
            assert p['S'] >= 2 and p['nch0'] >= 3 and W.chunks(p) >= 3, (c, p)
        seen[c.kind].add(p['cfg'])
    assert seen['one'] == set(range(13)) and seen['multi'] == set(range(13)), seen


def test_late_settings_leave_every_tile_a_workgroup():
    """The late hook's precondition, from the kernel's own decode: with S splits a tile whose S workgroups are all late
    (bid % late_mod == 1) is computed by nobody. late_mod = 1024 (only block 1) holds whenever S >= 2; late_mod = 3 holds
    on some plans only -- not on 3 tiles x 2 splits of the 160 family, where blocks 1 and 4 both serve tile 1 -- and must
    survive on at least one multi-chunk row of each family."""
    lib = _lib()
    with_3 = {False: 0, True: 0}
    for c in W.CASES:
        with W.compute_units(lib, c.cus):
            p = W.plan(lib, c.M, c.N, c.K)
        mods = W.late_mods(lib, p)
        assert all(W.late_ok(lib, p, m) for m in mods)
        assert (1024 in mods) == (p['S'] >= 2), (c, p)
        if p['S'] == 1 and p['ntiles'] >= 2:          # block 1 is tile 1's only workgroup
            assert not W.late_ok(lib, p, 1024) and not W.late_ok(lib, p, 3), (c, p)
        if c.kind == 'multi':
            with_3[c.cfg >= W.FIRST_160] += 3 in mods
    assert with_3[False] >= 1 and with_3[True] >= 1, with_3
    with W.compute_units(lib, 8):
        p = W.plan(lib, 9631, 320, 480)
    assert (p['cfg'], p['ntiles'], p['S']) == (8, 3, 2) and not W.late_ok(lib, p, 3) and W.late_ok(lib, p, 1024)
