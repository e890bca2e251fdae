"""GPU (-m gpu): lvl_clip_loss_bwd and lvl_ssl_clip_loss_bwd through the C ABI against the float64 slab reference
(tests/clip_loss_reference.py), float32 and bfloat16, on the exact-logit cases of every forward shape (E up to 768: the
gradient loop's second pass over the columns; G up to 1025), on coefficient rows around the 64 KiB LDS opt-in and at the
150 KiB limit (G = 16376, 16377, 38392), and on random rows at scale 14.285714 and 100.

The kernel and the reference read the SAME float32 lse_all array (the float64 LSEs rounded once); upstream = 0.7,
coef = 3 / (2 G) (rows_only: 1 / (2 B)). Tolerance, not chosen by running a kernel: elementwise
    |kernel - float64| <= 8 x recorded x un-cancelled magnitude,
the magnitude being |k| sum_j s_ij (p_ij + p'_ij + 2 delta_ij) |b_je| -- the terms as they stand BEFORE the diagonal
subtraction, because the kernel forms c_ii = (p + p') - 2 in float32 -- and `recorded` the distance of a float32
restatement of the kernels' arithmetic from float64 over the class of the case, measured on the CPU by
tests/test_clip_loss_reference_cpu.py (clip_loss_reference.BWD_F32_ERR). An element of magnitude 0 must be exactly 0. No
element and no case is skipped; every test prints its worst error / allowance.

Beyond the tolerance: float32 and bfloat16 launches of an exact case are bit-identical (the inputs are bfloat16 values and
all arithmetic is float32), so is a second launch; upstream == NULL is a device 1.0; B == 0 writes nothing; rows_only
never reads a partner LSE (they are NaN); the SSL kernel on one indicator value IS the clip kernel at that scale; any
non-zero indicator counts as 1; and the backward fed with the forward kernels' own LSEs gives the float64 autograd
gradient of the whole loss. Every gradient buffer lies inside 32 sentinel rows on each side, asserted untouched after every
launch (tests/clip_loss_launch.py, which also reads every small input back before it launches).
"""
import functools

import numpy as np
import pytest
import torch

import clip_loss_launch as K
import clip_loss_reference as R

pytestmark = pytest.mark.gpu

DTYPES = K.DTYPES
_id = lambda s: '-'.join(map(str, s))            # noqa: E731
_dt = lambda dt: 'bf16' if dt == torch.bfloat16 else 'f32'       # noqa: E731


@functools.lru_cache(maxsize=None)
def _ref(spec, rows_only=False):
    """(case, lse32, float64 gradient [2,B,E], un-cancelled magnitude [2,B,E]) of an exact case: computed once, shared,
    never written to"""
    c = R.exact_case(*spec)
    lse32 = R.case_lse32(c)
    g, u = R.case_backward(c, lse32, R.bwd_coef(c, rows_only), R.UPSTREAM, rows_only)
    for a in (lse32, g, u):
        a.setflags(write=False)
    return c, lse32, g, u


def _launch(c, dt, lse32, coef, upstream=R.UPSTREAM, rows_only=False, **kw):
    if c['kind'] == 'ssl':
        assert not rows_only
        return K.ssl_backward(c, dt, lse32, coef, upstream, **kw)
    return K.clip_backward(c, dt, lse32, coef, upstream, rows_only, **kw)


def _within(got, ref, umag, tol, tag, extra=0.0):
    """|got - ref| <= (tol + extra) * umag elementwise; magnitude 0 -> exactly 0. -> worst err / allowance"""
    assert got.shape == ref.shape == umag.shape and got.dtype == np.float32
    assert np.isfinite(got).all(), tag
    err = np.abs(got.astype(np.float64) - ref)
    allowed = (tol + extra) * umag
    zero = umag == 0
    assert (got[zero] == 0).all() and (ref[zero] == 0).all(), tag
    worst = float((err[~zero] / allowed[~zero]).max()) if (~zero).any() else 0.0
    print(f'{tag}: worst err/allowed {worst:.3f} (err/magnitude {worst * (tol + extra):.2e})')
    assert (err <= allowed).all(), (tag, worst)
    return worst


def _branches_reached(c):
    b = R.bwd_branches(c['B'], c['G'], c['E'], c['row0'])
    assert b['e_second_pass'] == (c['E'] > 256) and b['stride'] == (c['G'] > 256)
    return b


@pytest.mark.parametrize('dt', DTYPES, ids=('f32', 'bf16'))
@pytest.mark.parametrize('spec', R.BWD_SPECS, ids=_id)
def test_backward_exact_cases(spec, dt):
    """every gradient element within 8 x the recorded float32 error of the un-cancelled magnitude; a second launch
    bit-identical; upstream NULL == device 1.0; clip rows_only with NaN partner LSEs; B == 0 writes nothing"""
    c, lse32, ref, umag = _ref(spec)
    kind, G, B, row0 = c['kind'], c['G'], c['B'], c['row0']
    _branches_reached(c)
    coef = R.bwd_coef(c)
    tag = (spec, _dt(dt))
    got = _launch(c, dt, lse32, coef)
    _within(got, ref, umag, R.bwd_tol(kind, G), tag)
    assert np.array_equal(_launch(c, dt, lse32, coef), got), tag                       # deterministic
    # upstream == NULL means 1.0
    one = _launch(c, dt, lse32, coef, upstream=np.float32([1.0]))
    null = _launch(c, dt, lse32, coef, upstream=None)
    assert np.array_equal(null, one), tag
    assert not np.array_equal(one, got) or not got.any(), tag                          # 0.7 is not 1.0
    ref1, umag1 = R.case_backward(c, lse32, coef, None)
    _within(null, ref1, umag1, R.bwd_tol(kind, G), tag + ('NULL',))
    # B == 0: OK, nothing written (the launcher asserts every word of both buffers still the sentinel)
    assert _launch(c, dt, lse32, coef, B=0).shape == (2, 0, c['E'])
    if kind == 'clip':
        # rows_only: only the local entries of lse_all may be read
        _, _, ref_r, umag_r = _ref(spec, True)
        local = np.full_like(lse32, np.nan)
        local[:, row0:row0 + B] = lse32[:, row0:row0 + B]
        assert np.isnan(local).sum() == 2 * (G - B)
        got_r = _launch(c, dt, local, R.bwd_coef(c, True), rows_only=True)
        _within(got_r, ref_r, umag_r, R.bwd_tol('rows_only', G), tag + ('rows_only',))


@pytest.mark.parametrize('spec', R.BWD_SPECS, ids=_id)
def test_backward_float32_and_bfloat16_launches_are_bit_identical(spec):
    """the inputs of an exact case are bfloat16 values and all arithmetic is float32: any difference is a load bug"""
    c, lse32, _, _ = _ref(spec)
    coef = R.bwd_coef(c)
    assert R._is_bf16(c['img']) and R._is_bf16(c['txt'])
    a, b = _launch(c, torch.float32, lse32, coef), _launch(c, torch.bfloat16, lse32, coef)
    assert np.array_equal(a, b), spec
    if c['kind'] == 'clip':
        a, b = (_launch(c, dt, lse32, R.bwd_coef(c, True), rows_only=True) for dt in DTYPES)
        assert np.array_equal(a, b), spec


@pytest.mark.parametrize('kind', ['clip', 'ssl'])
def test_backward_at_the_lds_opt_in_and_at_the_lds_limit(kind):
    """E = 8: G = 16376 ((E + G) * 4 = 65536, no opt-in), 16377 (the first row that needs lvl_allow_lds), 38392 (153600
    bytes, the last row the host accepts); 2 or 3 local rows, one case starting at row 0, two ending at G. Exact inputs
    with ties, true LSEs from the grouped lse_all, the tolerance of the large-G class."""
    specs = [s for s in R.LARGE_SPECS if s[0] == kind]
    assert [(s[3] + s[2]) * 4 for s in specs] == [64 * 1024, 64 * 1024 + 4, R.LDS_LIMIT_BYTES]
    for spec in specs:
        c, lse32, ref, umag = _ref(spec)
        b = _branches_reached(c)
        assert b['lds_opt_in'] == (c['G'] > 16376) and b['lds_limit'] == (c['G'] == 38392) and len(c['ties']) >= 2
        outs = []
        for dt in DTYPES:
            got = _launch(c, dt, lse32, R.bwd_coef(c))
            _within(got, ref, umag, R.bwd_tol('large', c['G']), (spec, _dt(dt)))
            outs.append(got)
        assert np.array_equal(outs[0], outs[1]), spec


def _one_value_condition(clip, lse):
    """min over the local rows of (z - L_own) and (z - L_other[j]) in float64: above -80, no exp of the kernel is
    subnormal (exp(-80) = 1.8e-35), so a power-of-two scale commutes with every rounding"""
    z = R.case_forward(clip)['logits']
    idx = np.arange(clip['row0'], clip['row0'] + clip['B'])
    return min(float((z[d] - lse[d, idx][:, None]).min()) for d in range(2)), \
        min(float((z[d] - lse[1 - d][None, :]).min()) for d in range(2))


@pytest.mark.parametrize('spec', R.VALU_SHAPES, ids=_id)
def test_ssl_backward_with_one_indicator_value_is_the_clip_backward(spec):
    """scales3 = (16, 32, 64): all-zero indicators give lvl_clip_loss_bwd at scale 16 bit for bit, all-one at scale 64
    (c carries the factor s in one kernel and k in the other: a power of two, exact while nothing is subnormal -- asserted
    from the float64 reference: min (z - L) > -80)"""
    for value, scale in ((0, 16.0), (1, 64.0)):
        c, clip = R.one_value_pair(*spec, value)
        coef = R.bwd_coef(c)
        ind = c['ind']
        assert float(clip['scale'][0]) == scale and (ind == value).all()
        lse = R.lse_all(c['img'], c['txt'], clip['scale'])
        lo = _one_value_condition(clip, lse)
        assert min(lo) > -80, lo
        lse32 = lse.astype(np.float32)
        ref, umag = R.case_backward(clip, lse32, coef)
        for dt in DTYPES:
            a = K.ssl_backward(c, dt, lse32, coef, R.UPSTREAM, ind=ind)
            b = K.clip_backward(clip, dt, lse32, coef, R.UPSTREAM)
            assert np.array_equal(a, b), (spec, value, _dt(dt))
            _within(a, ref, umag, R.bwd_tol('clip', c['G']), (spec, value, _dt(dt)))


@pytest.mark.parametrize('spec', R.SSL_SPECS[1:6:2] + R.LARGE_SPECS[4:5], ids=_id)
def test_ssl_backward_reads_any_nonzero_indicator_as_one(spec):
    """indicators drawn from {0, 1, 2, -1, 7}: gradients bit-identical to the launch on their 0 / 1 images"""
    c, lse32, _, _ = _ref(spec)
    wild = K.wild_indicators(c['ind'], seed=spec[-1])
    for dt in DTYPES:
        a = K.ssl_backward(c, dt, lse32, R.bwd_coef(c), R.UPSTREAM, ind=wild)
        assert np.array_equal(a, K.ssl_backward(c, dt, lse32, R.bwd_coef(c), R.UPSTREAM)), (spec, _dt(dt))


@pytest.mark.parametrize('shape', R.RANDOM_BWD_SHAPES, ids=_id)
@pytest.mark.parametrize('cls', list(R.RANDOM_SCALES))
def test_backward_random_rows(cls, shape):
    """random unit rows at scale 14.285714 and at 100 (the clamp's upper end), rounded to the dtype first: clip, clip
    rows_only and SSL within 8 x the class's own recorded number. 'paired100': some local row holds more than 0.99 of its
    softmax mass on the diagonal, so c_ii = (p + p') - 2 cancels."""
    B, G, E, row0 = shape
    for dt in DTYPES:
        for kind in ('clip', 'ssl'):
            c = R.random_bwd_case(kind, *shape, cls, dt == torch.bfloat16)
            if cls == 'paired100':
                assert R.diag_mass(c).max() > 0.99
            lse32 = R.case_lse32(c)
            for rows_only in ((False, True) if kind == 'clip' else (False,)):
                coef = R.bwd_coef(c, rows_only)
                ref, umag = R.case_backward(c, lse32, coef, R.UPSTREAM, rows_only)
                lse_in = lse32
                if rows_only:
                    lse_in = np.full_like(lse32, np.nan)
                    lse_in[:, row0:row0 + B] = lse32[:, row0:row0 + B]
                got = _launch(c, dt, lse_in, coef, rows_only=rows_only)
                _within(got, ref, umag, R.bwd_tol(cls, G), (cls, kind, shape, _dt(dt), 'rows_only' if rows_only else 'full'))


def _autograd(c):
    """float64 autograd of the whole single-rank loss (mean of the two cross-entropies) -> d loss / d img, d loss / d txt"""
    a = torch.from_numpy(c['img']).double().requires_grad_(True)
    b = torch.from_numpy(c['txt']).double().requires_grad_(True)
    G = c['G']
    if c['kind'] == 'ssl':
        ind = torch.from_numpy(c['ind']).long()
        s = torch.from_numpy(c['scales3']).double()[ind[:, None] + ind[None, :]]
    else:
        s = float(c['scale'][0])
    z = s * (a @ b.t())
    lab = torch.arange(G)
    loss = (torch.nn.functional.cross_entropy(z, lab) + torch.nn.functional.cross_entropy(z.t(), lab)) / 2
    ga, gb = torch.autograd.grad(loss, [a, b])
    return np.stack([ga.numpy(), gb.numpy()])


@pytest.mark.parametrize('dt', DTYPES, ids=('f32', 'bf16'))
@pytest.mark.parametrize('spec', R.SINGLE_RANK_SPECS, ids=_id)
def test_backward_from_the_forward_kernels_own_lse(spec, dt):
    """single rank (B = G, row0 = 0), one shape per forward kernel (matrix-core, VALU, SSL): the backward is handed the
    lse the forward kernel produced and compared with float64 autograd of the whole loss. Allowance per element =
    the backward's own (8 x recorded x magnitude) + (exp(delta) - 1) x magnitude with delta = fwd_tol(G) x the largest row
    scale: an LSE off by delta multiplies every p of its row (or column) by exp(+-delta)."""
    c = R.exact_case(*spec)
    kind, G = c['kind'], c['G']
    assert c['B'] == G and c['row0'] == 0 and (c['layout'] == 'mfma') == (spec[3] == 64)
    f = R.case_forward(c)
    stats = (K.ssl_forward if kind == 'ssl' else K.clip_forward)(c, dt, want_logits=False)[0]
    lse_fwd = np.ascontiguousarray(stats[..., 0], dtype=np.float32)                    # [2,G], float32 as emitted
    assert np.array_equal(lse_fwd.astype(np.float64), stats[..., 0])
    delta = R.fwd_tol(G) * float(R.row_scale(f['logits']).max())
    assert (np.abs(lse_fwd - f['lse']) <= delta).all()
    coef = R.bwd_coef(c)
    k = coef * float(np.float64(R.UPSTREAM[0])) * 2 * G
    want = k * _autograd(c)
    ref, umag = R.case_backward(c, f['lse'], coef)                                      # from the true LSEs
    np.testing.assert_allclose(ref, want, atol=1e-13, rtol=1e-10)
    got = _launch(c, dt, lse_fwd, coef)
    _within(got, want, umag, R.bwd_tol(kind, G), (spec, _dt(dt)), extra=float(np.expm1(delta)))
