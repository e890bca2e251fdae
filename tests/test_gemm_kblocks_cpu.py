"""Host-only conditions of the K-axis matrix of lvl_linear_tn (test_gpu_gemm_kblocks.py): the shape table really runs the
paths it is there for, and the integer operands really make every K block count."""
import pytest
import torch

import gemm_tn_cases as G

ALL_CUS = 256          # compute units of an MI355X (any count >= 48 gives the same walk: one tile per workgroup)


def test_shape_table_walks_the_paths_it_is_there_for():
    """the static tile walk restated (gemm_tn_cases.static_walk) on the shapes of the matrix: at 8 CUs some workgroup walks
    at least 5 tiles (the ring of four bias images wraps) and, where there is more than one column tile, consecutive tiles of
    a workgroup differ in tn (they use different bias images); at 8 and 16 CUs a tail tile is followed by another tile of the
    same workgroup (the drain after a tail epilogue is followed by first blocks); at all CUs every workgroup has exactly one
    tile (the single-tile prologue and the past-the-end re-read)"""
    for N, (tile_rows, rems) in G.KB_SHAPES.items():
        tiles_n = N // 256
        ntiles = tile_rows * tiles_n
        for cus in (8, 16, ALL_CUS):
            walks = G.static_walk(ntiles, cus)
            assert sorted(t for w in walks for t in w) == list(range(ntiles)), (N, cus)       # every tile exactly once
            if cus == ALL_CUS:
                assert all(len(w) == 1 for w in walks), (N, cus)
                continue
            assert max(len(w) for w in walks) >= (5 if cus == 8 else 2), (N, cus)
            assert all(len(w) <= 6 for w in walks)                        # far below the audit's record capacity
            if tiles_n > 1:
                assert all(a % tiles_n != b % tiles_n for w in walks for a, b in zip(w, w[1:])), (N, cus)
                # with a row remainder the last tile row is the tail: one of its tiles is not its workgroup's last
                tail = set(range(ntiles - tiles_n, ntiles))
                assert any(a in tail for w in walks for a in w[:-1]), (N, cus)
        for rem in rems:
            M = G.kb_rows(N, rem)
            assert (M + 255) // 256 == tile_rows and M % 256 == rem
    # the configurations: static only below DYN_MIN_NB (plus the counter-block call), the full matrix from there on
    assert [G.kb_blocks(m, k) for m, k in G.KB_MODES] == [1, 2, 3, 4, 5, 6, 7, 8, 3, 9]
    for mode, K in G.KB_MODES:
        cfg = G.kb_configs(mode, K)
        if G.kb_blocks(mode, K) < G.DYN_MIN_NB:
            assert cfg == ((8, 'static'), (16, 'static'), (0, 'static'), (0, 'dynamic'))
        else:
            assert cfg == G.CONFIGS and len(cfg) == 8
    assert len(G.KB_CASES) == 10 * 6


@pytest.mark.parametrize('mode,K', G.KB_MODES)
def test_every_k_block_counts_in_the_integer_operands(mode, K):
    """gemm_tn_cases.kblock_int_data on the host, both shapes: results exactly representable (|acc| + |b| + |r| < 256 for
    the bf16 kernels, < 2^24 for the f32-class ones), and for every nb > 1 and every K block b the reference with block b
    removed, and with block b counted twice, differs from the true one in at least 90 % of the output elements (by
    construction in all of them: every block's own product is odd, or dominated by its marker column)"""
    for N, rem in ((768, 255), (256, 33)):
        d = G.kblock_int_data(N, G.kb_rows(N, rem), 7 * N + rem + K, mode, K, 'cpu')
        worst = G.check_every_block_counts(d, mode)
        assert worst == 1.0, (mode, K, N, worst)
        if mode == 'bf16':
            # marker columns: +-1 in x and w; every other x even
            cols = torch.arange(0, K, 64)
            assert bool((d['x'][:, cols].abs() == 1).all()) and bool((d['w'][:, cols].abs() == 1).all())
            assert bool((d['x'].float() % 2 == 0).sum() == d['x'].numel() - d['x'].shape[0] * len(cols))
        else:
            # both low term images are alive in every block that holds them
            Kc = K
            assert bool((d['x3'][:, 2 * Kc:][:, ::64] != 0).all()) and bool((d['w3'][:, Kc:2 * Kc][:, ::64] != 0).all())
