"""CPU: the float64 slab reference of the contrastive head (tests/clip_loss_reference.py) against the float32 oracle
restatements and float64 autograd, and every input condition tests/test_gpu_clip_loss_exact.py and
tests/test_gpu_clip_loss_bwd_exact.py rely on -- exactness of the logits in any summation order (also of the lo-bearing
cases, fragment by fragment), the planted ties and their relation to the kernels' work split, the branch each shape
reaches, the grouped lse_all against the plain one -- computed from the shapes, plus the measurements the GPU tolerances
of lse / expect and of both backwards are derived from."""
import os

import numpy as np
import pytest
import torch

import clip_loss_reference as R
from helpers import (oracle_slab_backward, oracle_slab_forward, oracle_ssl_slab_backward, oracle_ssl_slab_forward)
from oracle import oracle as O

ALL_EXACT = R.CLIP_SPECS + R.SSL_SPECS


def _old_inputs(kind, B, G, E, row0):
    c = R.random_case(kind, B, G, E, row0)
    return c, torch.from_numpy(c['img']), torch.from_numpy(c['txt'])


@pytest.mark.parametrize('B,G,E,row0', R.OLD_SHAPES)
def test_clip_reference_agrees_with_float32_oracle_and_float64_autograd(B, G, E, row0):
    c, img, txt = _old_inputs('clip', B, G, E, row0)
    scale = torch.from_numpy(c['scale'])
    z, st, am = R.slab_forward(img, txt, scale, B, row0)
    st_o, am_o = oracle_slab_forward(img, txt, scale[0], B, row0)
    li = O.clip_logits(img, txt, scale[0])
    # float32 rounding of values of size <= scale: a few ulp(16) = 2e-6 each, E-term sums
    np.testing.assert_allclose(z, torch.stack([li[row0:row0 + B], li.t()[row0:row0 + B]]).numpy(), atol=2e-5, rtol=0)
    np.testing.assert_allclose(R.stats4(st), st_o.numpy(), atol=2e-5, rtol=0)
    assert np.array_equal(am, am_o.numpy())
    lse = R.lse_all(img, txt, scale)
    np.testing.assert_allclose(lse[:, row0:row0 + B], st['lse'], atol=1e-13, rtol=0)
    up = torch.tensor([0.7])
    for rows_only, coef in ((False, 3.0 / (2 * G)), (True, 1.0 / (2 * B))):
        gi, gt, mi, mt = R.slab_backward(img, txt, lse, scale, up, coef, B, row0, rows_only)
        gi_o, gt_o = oracle_slab_backward(img, txt, torch.from_numpy(lse).float(), scale, up, coef, B, row0, rows_only)
        np.testing.assert_allclose(gi, gi_o.numpy(), atol=2e-6, rtol=1e-4)
        np.testing.assert_allclose(gt, gt_o.numpy(), atol=2e-6, rtol=1e-4)
        assert (np.abs(gi) <= mi * (1 + 1e-12)).all() and (np.abs(gt) <= mt * (1 + 1e-12)).all()
    # float64 autograd of the oracle's full loss: coef * upstream * 2G * d loss / d local rows
    ia, ta = img.double().requires_grad_(True), txt.double().requires_grad_(True)
    loss = O.clip_loss(ia, ta, scale.double().reshape(()))['loss']
    g_i, g_t = torch.autograd.grad(loss, [ia, ta])
    gi, gt, _, _ = R.slab_backward(img, txt, lse, scale, up, 3.0 / (2 * G), B, row0)
    k = 3.0 / (2 * G) * float(up.double()) * 2 * G
    np.testing.assert_allclose(gi, k * g_i[row0:row0 + B].numpy(), atol=1e-13, rtol=1e-10)
    np.testing.assert_allclose(gt, k * g_t[row0:row0 + B].numpy(), atol=1e-13, rtol=1e-10)
    if B == G:                                                # one rank: the slab statistics are the whole loss
        assert abs(loss.item() - (st['lse'] - st['diag']).sum() / (2 * G)) < 1e-12


@pytest.mark.parametrize('B,G,E,row0', R.OLD_SHAPES)
def test_ssl_reference_agrees_with_float32_oracle_and_float64_autograd(B, G, E, row0):
    c, img, txt = _old_inputs('ssl', B, G, E, row0)
    ind, s3 = torch.from_numpy(c['ind']).long(), torch.from_numpy(c['scales3'])
    z, st, am, d = R.ssl_slab_forward(img, txt, ind, s3, B, row0)
    st_o, am_o = oracle_ssl_slab_forward(img, txt, ind, s3, B, row0)
    np.testing.assert_allclose(st[..., :7], st_o[..., :7].numpy(), atol=2e-5, rtol=0)
    assert np.array_equal(am, am_o.numpy()) and (st[..., 7] == 0).all()
    lse = R.lse_all(img, txt, None, ind, s3, chunk=5)
    np.testing.assert_allclose(lse[:, row0:row0 + B], st[..., 0], atol=1e-13, rtol=0)
    up = torch.tensor([0.7])
    gi, gt, mi, mt = R.ssl_slab_backward(img, txt, ind, lse, s3, up, 3.0 / (2 * G), B, row0)
    gi_o, gt_o = oracle_ssl_slab_backward(img, txt, ind, torch.from_numpy(lse).float(), s3, up, 3.0 / (2 * G), B, row0)
    np.testing.assert_allclose(gi, gi_o.numpy(), atol=2e-6, rtol=1e-4)
    np.testing.assert_allclose(gt, gt_o.numpy(), atol=2e-6, rtol=1e-4)
    ia, ta = img.double().requires_grad_(True), txt.double().requires_grad_(True)
    # the float64 loss on the SAME three scales (the geometric mean as stored, not recomputed)
    s3d = s3.double()
    li = s3d[ind[:, None] + ind[None, :]] * (ia @ ta.t())
    lab = torch.arange(G)
    loss = (torch.nn.functional.cross_entropy(li, lab) + torch.nn.functional.cross_entropy(li.t(), lab)) / 2
    g_i, g_t = torch.autograd.grad(loss, [ia, ta])
    k = 3.0 / (2 * G) * float(up.double()) * 2 * G
    np.testing.assert_allclose(gi, k * g_i[row0:row0 + B].numpy(), atol=1e-13, rtol=1e-10)
    np.testing.assert_allclose(gt, k * g_t[row0:row0 + B].numpy(), atol=1e-13, rtol=1e-10)
    ref = O.ssl_clip_loss(img.double(), txt.double(), ind, s3d[2], s3d[0])['loss']      # geo recomputed: float32 rounding of it
    assert abs(ref.item() - loss.item()) < 1e-5


def test_chunked_lse_equals_the_direct_computation():
    for kind in ('clip', 'ssl'):
        c = R.exact_case(kind, 5, 300, 8, 295, 1)             # sparse rows: few distinct logits
        r = R.random_case(kind, 5, 300, 8, 295)
        for d in (c, r):
            ssl = kind == 'ssl'
            args = (d['img'], d['txt'], None if ssl else d['scale'], d['ind'] if ssl else None, d['scales3'] if ssl else None)
            a, b = d['img'].astype(np.float64), d['txt'].astype(np.float64)
            s = d['scales3'].astype(np.float64)[d['ind'][:, None] + d['ind'][None, :]] if ssl else float(d['scale'][0])
            z = s * (a @ b.T)                                 # G = 300: the one place a full matrix is formed, as the check
            want = np.stack([torch.logsumexp(torch.from_numpy(z), 1).numpy(), torch.logsumexp(torch.from_numpy(z), 0).numpy()])
            for chunk in (512, 64, 7, 1):
                np.testing.assert_allclose(R.lse_all(*args, chunk=chunk), want, atol=1e-12, rtol=0)


def _f32_logits_in_order(own, other, scale, order, pair=None):
    """float32 evaluation of the scaled dot products, accumulating the E products in the given order"""
    a = (np.float32(scale) * own) if pair is None else own
    acc = np.zeros((own.shape[0], other.shape[0]), dtype=np.float32)
    for e in order:
        acc = acc + a[:, e, None] * other[None, :, e]
        assert acc.dtype == np.float32
    return acc if pair is None else acc * pair


@pytest.mark.parametrize('spec', ALL_EXACT, ids=lambda s: '-'.join(map(str, s)))
def test_exact_cases_hold_their_conditions(spec):
    """Building a case asserts bf16-exact operands, the 2^24 bound and the tie sets (clip_loss_reference.exact_inputs).
    Here: the float32 logits are bit-identical in several summation orders and equal float64, every planted tie is the
    row maximum at exactly {label, other} in the relation its tag names, and for SSL the tie is absent before scaling."""
    kind, B, G, E, row0, n = spec
    c = R.exact_case(*spec)
    f = R.case_forward(c)
    rng = np.random.default_rng(n)
    orders = [np.arange(E), np.arange(E)[::-1], rng.permutation(E), np.concatenate([np.arange(1, E, 2), np.arange(0, E, 2)])]
    rows = slice(row0, row0 + B)
    for d in range(2):
        own, other = (c['img'], c['txt'])[d][rows], (c['txt'], c['img'])[d]
        pair = c['scales3'][c['ind'][rows, None] + c['ind'][None, :]] if kind == 'ssl' else None
        for o in orders:
            got = _f32_logits_in_order(own, other, None if kind == 'ssl' else c['scale'][0], o, pair)
            assert np.array_equal(got.astype(np.float64), f['logits'][d])
    rel_of = R.mfma_relation if c['layout'] == 'mfma' else R.valu_relation
    for lab, oth, rel, pos in c['ties']:
        assert row0 <= lab < row0 + B and 0 <= oth < G
        assert rel_of(lab, oth, G) == rel and ((lab < oth) == (pos == 'lower'))
        for d in range(2):
            z = f['logits'][d][lab - row0]
            assert sorted(np.flatnonzero(z == z.max())) == sorted((lab, oth))
            assert f['argmax'][d][lab - row0] == min(lab, oth)               # the label wins only when it is the lower one
            if kind == 'ssl':
                dots = f['dots'][d][lab - row0]
                assert c['ind'][lab] != c['ind'][oth] and dots[lab] != dots[oth]
    # the row's contribution to the accuracy count moves with the rule: under "last maximum" every planted row flips
    last = G - 1 - np.argmax(f['logits'][0][:, ::-1], axis=-1)
    for lab, oth, _, pos in c['ties']:
        assert (f['argmax'][0][lab - row0] == lab) == (pos == 'lower') and (last[lab - row0] == lab) == (pos == 'higher')


def test_tie_placements_cover_every_relation_both_ways():
    clip = [R.exact_case(*s) for s in R.CLIP_SPECS]
    want_m = {(r, p) for r in R.MFMA_RELATIONS for p in ('lower', 'higher')}
    want_v = {(r, p) for r in R.VALU_RELATIONS for p in ('lower', 'higher')}
    assert R.tie_coverage([c for c in clip if c['layout'] == 'mfma']) == want_m
    assert R.tie_coverage([c for c in clip if c['layout'] == 'valu']) == want_v
    assert R.tie_coverage([R.exact_case(*s) for s in R.SSL_SPECS]) == want_v
    # the planted pairs of the matrix-core list never share a LANE (columns 64 n apart: same wave, same j % 16), where
    # the per-lane `z > best` decides; the sparse rows tie there on their own -- rows whose first maximum has a later
    # tied column in its own lane, which `>=` would report instead
    same_lane = 0
    for c in (c for c in clip if c['layout'] == 'mfma'):
        assert all((lab - oth) % 64 for lab, oth, _, _ in c['ties'])
        z = R.case_forward(c)['logits'].reshape(-1, c['G'])
        for row in z:
            w = np.flatnonzero(row == row.max())
            same_lane += bool(((w[1:] - w[0]) % 64 == 0).any())
    assert same_lane >= 10, same_lane
    for E in R.MFMA_WIDTHS:                                   # every width sees ties inside a tile and across waves
        cov = R.tie_coverage([c for c in clip if c['E'] == E])
        assert {r for r, _ in cov} >= {'same_tile', 'cross_wave'}, (E, cov)
    assert all(c['layout'] == 'valu' for c in (R.exact_case(*s) for s in R.SSL_SPECS))


def test_shapes_reach_the_branches_they_are_listed_for():
    m = {s: R.mfma_branches(s[0], s[1], s[3]) for s in R.MFMA_SHAPES}
    assert {s[2] for s in R.MFMA_SHAPES} == set(R.MFMA_WIDTHS)
    for E in R.MFMA_WIDTHS:
        assert 2 <= sum(s[2] == E for s in R.MFMA_SHAPES) <= 4
    assert {(1, 1, 0), (16, 16, 0), (17, 83, 66), (33, 50, 17), (5, 300, 295), (40, 129, 3)} <= {(s[0], s[1], s[3]) for s in R.MFMA_SHAPES}
    for s, b in m.items():
        B, G, E, row0 = s
        if (B, G, row0) == (33, 50, 17):       # 4 tiles would need G > 48: here tiles 0..3, the last partial; G < 64
            assert b['partial_tile'] and b['second_workgroup_partial'] and b['row0_unaligned'] and 16 < G < 64
        if (B, G, row0) == (17, 83, 66):       # second workgroup with ONE live row, partial tile 5, row0 % 16 = 2
            assert b['second_workgroup_partial'] and b['partial_tile'] and b['row0_unaligned'] and b['several_tiles_per_wave']
        if (B, G, row0) == (40, 129, 3):       # three workgroups, the last with 8 rows; tile 8 holds one column
            assert b['second_workgroup_partial'] and G % 16 == 1 and b['several_tiles_per_wave'] and b['row0_unaligned']
        if (B, G, row0) == (5, 300, 295):      # the local rows END at G inside the partial tile 18
            assert b['partial_row_group'] and b['partial_tile'] and row0 + B == G
        if (B, G, row0) in ((1, 1, 0), (16, 16, 0)):   # one tile: three waves carry m = -inf into the merge
            assert b['idle_waves']
        if (B, G, row0) == (19, 37, 13):       # 3 tiles at 16 < G < 64: wave 3 owns none; second workgroup with 3 rows
            assert b['idle_waves'] and b['partial_tile'] and b['row0_unaligned'] and b['second_workgroup_partial']
    assert any(b['idle_waves'] and 16 < s[1] < 64 for s, b in m.items())
    v = {s: R.valu_branches(s[0], s[1], s[3]) for s in R.VALU_SHAPES}
    assert {s[2] for s in R.VALU_SHAPES} == {8, 24, 264, 768} and {s[1] for s in R.VALU_SHAPES} == {1, 63, 257, 300, 1025}
    assert all(s[0] % 2 == 1 and not R.uses_mfma(s[2]) for s in R.VALU_SHAPES)
    assert sum(b['ends_at_G'] for b in v.values()) >= 3
    for E in (8, 24, 264, 768):
        bs = [b for s, b in v.items() if s[2] == E]
        assert any(b['stride'] for b in bs) or E == 24 and any(b['ragged_last_pass'] for b in bs)
        assert any(b['idle_threads'] for b in bs) or any(b['ragged_last_pass'] for b in bs)
    assert any(b['stride'] and b['ragged_last_pass'] for b in v.values()) and any(b['idle_waves'] for b in v.values())


def test_float32_restatement_error_is_within_the_recorded_one():
    """The number the GPU tolerance of lse / expect is 8 x of: measured here, from the float32 restatement alone. Only
    `measured <= recorded` depends on this host's float32 exp / log; `recorded` itself is held under fixed ceilings."""
    fs = max(R.forward_f32_error(R.exact_case(*s)) for s in R.CLIP_SPECS + R.SSL_SPECS)
    print(f'forward float32 restatement: {fs:.3e}')
    assert max(s[2] for s in R.CLIP_SPECS + R.SSL_SPECS) == R.MEASURED_G_MAX
    assert fs <= R.FWD_F32_ERR <= R.FWD_F32_ERR_CEILING
    assert R.MARGIN == 8 and R.fwd_tol(R.MEASURED_G_MAX) <= 1e-4      # never looser than the older slab test at scale ~ 14


def _body(src, name):
    """the definition of one extern "C" entry point, comments removed"""
    start = src.index(f'extern "C" int {name}(')
    end = src.find('\nextern "C"', start + 1)
    body = src[start:end if end > 0 else len(src)]
    body = body[:body.index('\n}\n') + 3]
    return '\n'.join(line.split('//')[0] for line in body.split('\n'))


@pytest.mark.parametrize('name', ['lvl_clip_loss_bwd', 'lvl_ssl_clip_loss_bwd'])
def test_backward_refuses_a_row_beyond_the_LDS_limit_on_the_host(name):
    """G = 38393 with E = 8: (E + G) * 4 is four bytes over the 150 KiB the coefficient row may take. The entry point's
    source is read FIRST: the null, shape and LDS checks are its first statements, in front of lvl_allow_lds, the launch
    and every other use of an argument. Only then is it called -- which therefore needs no device: the buffers are host
    arrays that are never dereferenced, the gradient buffers keep their sentinel, and lvl_last_error names G."""
    import ctypes
    from lavila_amd import _cabi as C
    src = open(os.path.join(os.path.dirname(C.LIB_PATH), '..', 'csrc', 'clip_loss.hip')).read()
    body = _body(src, name)
    stmts = [t.strip() for t in body[body.index('{') + 1:].split(';')]
    assert [t.split('(')[0] for t in stmts[:3]] == ['LVL_REQUIRE'] * 3, stmts[:3]
    assert 'null pointer' in stmts[0] and 'bad shape' in stmts[1]
    assert '(size_t)(E + G) * sizeof(float) <= 150 * 1024' in stmts[2] and 'too large for the LDS-resident row' in stmts[2]
    assert not any(w in t for t in stmts[:3] for w in ('hip', 'lvl_allow_lds', '<<<', '*scale', '*upstream'))
    assert body.count('hipLaunchKernelGGL') == 1 and body.index('lvl_allow_lds') < body.index('hipLaunchKernelGGL')
    lib = C.lib()
    G, E, B = 38393, 8, 3
    assert (E + G) * 4 == R.LDS_LIMIT_BYTES + 4
    emb = np.zeros((2, G, E), np.float32)
    lse, ind, scales, up = np.zeros((2, G), np.float32), np.zeros(G, np.int32), np.float32([16, 32, 64]), np.float32([0.7])
    grads = np.full((2, B, E), 0x7FA5A5A5, dtype=np.uint32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)           # noqa: E731
    for dtype in (C.LVL_F32, C.LVL_BF16):
        if name == 'lvl_clip_loss_bwd':
            rc = lib.lvl_clip_loss_bwd(p(emb[0]), p(emb[1]), p(lse), p(scales), p(up), 1.0, B, G, E, G - B, 0, p(grads[0]),
                                       p(grads[1]), dtype, None)
        else:
            rc = lib.lvl_ssl_clip_loss_bwd(p(emb[0]), p(emb[1]), p(ind), p(lse), p(scales), p(up), 1.0, B, G, E, G - B,
                                           p(grads[0]), p(grads[1]), dtype, None)
        msg = lib.lvl_last_error().decode()
        assert rc != 0 and 'too large for the LDS-resident row' in msg and f'G={G}' in msg, (rc, msg)
        assert (grads == 0x7FA5A5A5).all()


# ----------------------------------------------------------------------------------------------------------------------
# what tests/test_gpu_clip_loss_bwd_exact.py and the lo-bearing forward cases rely on
# ----------------------------------------------------------------------------------------------------------------------
def _lse_args(c):
    ssl = c['kind'] == 'ssl'
    return (c['img'], c['txt'], None if ssl else c['scale'], c['ind'] if ssl else None, c['scales3'] if ssl else None)


def test_grouped_lse_equals_the_chunked_one():
    """lse_all computes each distinct (row, indicator) once, weighted by its count: equal to every row against every
    column at G <= 1025 (weights instead of repeated terms reorder a float64 sum: 1e-12 on values of size <= 100), on the
    sparse exact cases, where the grouping bites, and on random rows, where every row is its own group"""
    cases = [R.exact_case(*s) for s in R.BWD_SPECS]
    cases += [R.random_bwd_case(kind, *sh, cls, False) for kind in ('clip', 'ssl') for sh in R.RANDOM_BWD_SHAPES
              for cls in R.RANDOM_SCALES]
    grouped = 0
    for c in cases:
        assert c['G'] <= 1025
        want = R.lse_all_chunked(*_lse_args(c))
        for chunk in (512, 7):
            np.testing.assert_allclose(R.lse_all(*_lse_args(c), chunk=chunk), want, atol=1e-12, rtol=0)
        key = np.concatenate([c['txt'], c['ind'][:, None]], 1) if c['kind'] == 'ssl' else c['txt']
        grouped += len(np.unique(key, axis=0)) < c['G'] // 2
    assert grouped >= 3, grouped                              # the E = 8 shapes: at most 112 (SSL: 224) distinct rows
    for s in R.LARGE_SPECS:                                   # E = 8, two non-zeros: at most 4 * C(8,2) rows, planted ones aside
        c = R.exact_case(*s)
        assert len(np.unique(c['txt'], axis=0)) <= 112 + 2 * len(c['ties']) and len(c['ties']) >= 2


def test_backward_shapes_reach_the_branches_they_are_listed_for():
    clip = [s[1:5] for s in R.BWD_SPECS if s[0] == 'clip']
    ssl = [s[1:5] for s in R.BWD_SPECS if s[0] == 'ssl']
    assert sorted(clip) == sorted(R.MFMA_SHAPES + R.VALU_SHAPES) and sorted(ssl) == sorted(R.VALU_SHAPES)
    for shapes in (clip, ssl):
        br = {s: R.bwd_branches(*s) for s in shapes}
        for tag in ('e_second_pass', 'idle_column_threads', 'stride', 'ends_at_G'):
            assert any(b[tag] for b in br.values()), tag
        assert any(b['e_second_pass'] and b['stride'] for b in br.values())
        assert {s[2] for s in shapes} >= {264, 768} and max(s[1] for s in shapes) == 1025
        assert not any(b['lds_opt_in'] for b in br.values())
    assert 512 in {s[2] for s in clip} and 256 in {s[2] for s in clip}      # E == 256: exactly one pass, no idle thread
    lg = [R.bwd_branches(*s) for s in R.LARGE_SHAPES]
    assert [(s[2] + s[1]) * 4 for s in R.LARGE_SHAPES] == [65536, 65540, R.LDS_LIMIT_BYTES]
    assert [b['lds_opt_in'] for b in lg] == [False, True, True] and [b['lds_limit'] for b in lg] == [False, False, True]
    assert any(b['ends_at_G'] for b in lg) and any(s[3] == 0 for s in R.LARGE_SHAPES)
    assert all(s[0] in (2, 3) and s[2] == 8 for s in R.LARGE_SHAPES)
    assert {s[0] for s in R.LARGE_SPECS} == {'clip', 'ssl'}
    assert R.RANDOM_BWD_SHAPES == ((32, 256, 256, 64), (5, 300, 768, 7), (7, 1025, 24, 500))
    assert R.RANDOM_SCALES == {'random14': 14.285714, 'random100': 100.0, 'paired100': 100.0}


def _bwd_classes():
    """class -> [(case, rows_only)]: every case whose device tolerance is MARGIN x the class's recorded number"""
    ex = [R.exact_case(*s) for s in R.BWD_SPECS + R.SINGLE_RANK_SPECS]
    ex += [R.one_value_pair(*s, v)[1] for s in R.VALU_SHAPES for v in (0, 1)]               # held to the clip class
    out = {'clip': [(c, False) for c in ex if c['kind'] == 'clip'], 'rows_only': [(c, True) for c in ex if c['kind'] == 'clip'],
           'ssl': [(c, False) for c in ex if c['kind'] == 'ssl'], 'large': [(R.exact_case(*s), False) for s in R.LARGE_SPECS]}
    for cls in R.RANDOM_SCALES:
        out[cls] = []
        for sh in R.RANDOM_BWD_SHAPES:
            for bf16 in (False, True):
                out[cls] += [(R.random_bwd_case('clip', *sh, cls, bf16), False), (R.random_bwd_case('clip', *sh, cls, bf16), True),
                             (R.random_bwd_case('ssl', *sh, cls, bf16), False)]
    return out


def test_backward_float32_restatement_error_is_within_the_recorded_one():
    """The numbers the device tolerances of both backwards are 8 x of, per class, measured here from backward_f32 alone
    over the un-cancelled magnitude. Only `measured <= recorded` depends on this host's float32 exp; `recorded` is held
    under a ceiling fixed from the class's G (clip_loss_reference.bwd_ceiling states the reason)."""
    classes = _bwd_classes()
    assert set(classes) == set(R.BWD_F32_ERR) == set(R.BWD_CLASS_G)
    for cls, cases in classes.items():
        measured = max(R.backward_f32_error(c, ro) for c, ro in cases)
        print(f'backward float32 restatement, {cls}: {measured:.3e} (recorded {R.BWD_F32_ERR[cls]:.1e}, '
              f'ceiling {R.bwd_ceiling(cls):.1e})')
        assert max(c['G'] for c, _ in cases) == R.BWD_CLASS_G[cls]
        assert measured <= R.BWD_F32_ERR[cls] <= R.bwd_ceiling(cls), cls
        assert R.bwd_tol(cls, R.BWD_CLASS_G[cls]) == 8 * R.BWD_F32_ERR[cls]
    eps = float(np.finfo(np.float32).eps)
    assert R.bwd_ceiling('clip') == eps * 1025 and R.bwd_ceiling('large') == eps * 38392
    assert R.bwd_ceiling('random100') == eps * (1025 + 0.5 * 768 * 100.0)


def test_uncancelled_magnitude_is_the_sum_of_the_terms_before_the_diagonal_subtraction():
    for c, rows_only in ((R.exact_case('clip', 5, 300, 8, 295, 1), False), (R.exact_case('clip', 5, 300, 8, 295, 1), True),
                         (R.exact_case('ssl', 3, 63, 24, 11, 3), False), (R.random_bwd_case('ssl', 5, 300, 768, 7, 'random100', False), False)):
        B, G, row0, ssl = c['B'], c['G'], c['row0'], c['kind'] == 'ssl'
        lse = R.case_lse32(c).astype(np.float64)
        coef = R.bwd_coef(c, rows_only)
        g, u = R.case_backward(c, lse, coef, R.UPSTREAM, rows_only)
        k = coef * float(np.float64(R.UPSTREAM[0]))
        a, b = c['img'].astype(np.float64), c['txt'].astype(np.float64)
        ind = c['ind'].astype(np.int64)
        for d, (own, other) in enumerate(((a, b), (b, a))):
            for i in range(B):
                gi = row0 + i
                s = c['scales3'].astype(np.float64)[ind[gi] + ind] if ssl else np.full(G, float(c['scale'][0]))
                z = s * (other @ own[gi])
                t = np.exp(z - lse[d, gi]) + (0 if rows_only else np.exp(z - lse[1 - d]))
                t[gi] += 1.0 if rows_only else 2.0
                np.testing.assert_allclose(u[d, i], k * ((s * t) @ np.abs(other)), rtol=1e-12, atol=0)
        if ssl:
            o = R.ssl_slab_backward(c['img'], c['txt'], c['ind'], lse, c['scales3'], R.UPSTREAM, coef, B, row0, True)
        else:
            o = R.slab_backward(c['img'], c['txt'], lse, c['scale'], R.UPSTREAM, coef, B, row0, rows_only, True)
        for grad, mag, umag in ((o[0], o[2], o[4]), (o[1], o[3], o[5])):
            assert (np.abs(grad) <= mag * (1 + 1e-12)).all() and (mag <= umag * (1 + 1e-12)).all()
    # sparse rows: some gradient column takes its WHOLE un-cancelled magnitude from the diagonal term, while |c_ii| is
    # far below 2 there -- a tolerance over sum |c| |b| would hold the kernel to ulps of a cancelled value
    c = R.exact_case('clip', 5, 300, 8, 295, 1)
    lse = R.case_lse32(c)
    o = R.slab_backward(c['img'], c['txt'], lse, c['scale'], R.UPSTREAM, R.bwd_coef(c), c['B'], c['row0'], False, True)
    assert (o[4] > 1.5 * o[2]).any()


def test_peaked_random_cases_have_the_diagonal_cancellation():
    """scale 100, 'paired100': in every case some local row holds softmax mass > 0.99 on its diagonal, so
    c_ii = (p + p') - 2 cancels. The loose pairs of random_case ('random100') peak off the diagonal: stated, not hidden."""
    loose = 0.0
    for kind in ('clip', 'ssl'):
        for sh in R.RANDOM_BWD_SHAPES:
            for bf16 in (False, True):
                assert R.diag_mass(R.random_bwd_case(kind, *sh, 'paired100', bf16)).max() > 0.99
                c = R.random_bwd_case(kind, *sh, 'random100', bf16)
                f = R.case_forward(c)
                loose = max(loose, R.diag_mass(c).max())
                if sh[2] != 768:
                    assert np.exp(f['max'] - f['lse']).max() > 0.99       # peaked all the same, on another column
    print(f'largest diagonal mass of the loose pairs at scale 100: {loose:.4f}')
    assert loose < 0.99


@pytest.mark.parametrize('which', ['img', 'txt'])
@pytest.mark.parametrize('shape', R.MFMA_SHAPES, ids=lambda s: '-'.join(map(str, s)))
def test_lo_bearing_cases_hold_their_conditions(shape, which):
    """lo_case asserts the fragments, the other matrix and the 2^24 bound from the inputs. Here: the float32 logits are
    bit-identical in several summation orders -- also when every operand is split into its bfloat16 hi and lo fragments
    and the three products the kernel forms are accumulated separately -- and equal float64; the logits are the base
    case's times 513 / 512, the argmax and the tie sets are the base case's; dropping either mixed product moves every
    non-zero logit of one direction."""
    n = R.MFMA_SHAPES.index(shape)
    c, base = R.lo_case(which, *shape, n), R.exact_case('clip', *shape, n)
    f, fb = R.case_forward(c), R.case_forward(base)
    B, G, E, row0 = shape
    assert np.array_equal(f['logits'], fb['logits'] * (1 + 2.0 ** -9)) and np.array_equal(f['argmax'], fb['argmax'])
    assert c['ties'] == base['ties'] and len(c['ties']) >= (0 if G == 1 else 1)
    for lab, oth, _, _ in c['ties']:
        for d in range(2):
            z = f['logits'][d][lab - row0]
            assert sorted(np.flatnonzero(z == z.max())) == sorted((lab, oth))
    rows = slice(row0, row0 + B)
    rng = np.random.default_rng(n)
    orders = [np.arange(E), np.arange(E)[::-1], rng.permutation(E)]
    scale = c['scale'][0]
    for d in range(2):
        own, other = (c['img'], c['txt'])[d][rows], (c['txt'], c['img'])[d]
        for o in orders:
            assert np.array_equal(_f32_logits_in_order(own, other, scale, o).astype(np.float64), f['logits'][d])
        a = np.float32(scale) * own
        ah, al, bh, bl = R.round_bf16(a), R.bf16_lo(a), R.round_bf16(other), R.bf16_lo(other)
        assert np.array_equal(ah + al, a) and np.array_equal(bh + bl, other) and not (al != 0).any() * (bl != 0).any()
        three = (_f32_logits_in_order(al, bh, 1.0, orders[2]) + _f32_logits_in_order(ah, bl, 1.0, orders[1])
                 + _f32_logits_in_order(ah, bh, 1.0, orders[0]))
        assert three.dtype == np.float32 and np.array_equal(three.astype(np.float64), f['logits'][d])
        a_lo_side = (which == 'img') == (d == 0)                  # this direction's lo fragments sit in A (the own rows)
        assert (al != 0).any() == a_lo_side and (bl != 0).any() == (not a_lo_side)
        dropped = _f32_logits_in_order(ah, bh, 1.0, orders[0]).astype(np.float64)      # without the mixed product
        nz = f['logits'][d] != 0
        assert (nz.any() or G == 1) and (dropped[nz] != f['logits'][d][nz]).all()     # (one sparse pair may not overlap)
        assert np.array_equal(dropped, fb['logits'][d])           # off by 2^-9 relative, everywhere
