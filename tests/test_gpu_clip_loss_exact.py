"""GPU (-m gpu): the two contrastive forwards through the C ABI against the float64 slab reference
(tests/clip_loss_reference.py): lvl_clip_loss_fwd -- the matrix-core kernel for E in 64/128/256/512 and the VALU kernel for
every other width -- and lvl_ssl_clip_loss_fwd (per-pair temperature, three bucket expectations, its own 9-word merge),
on inputs whose logits are EXACT in float32 (so the logits slab, the diagonal, the maximum and the argmax under "first
maximum kept" must be equal to the reference bit for bit), with the row maximum tied at planted column pairs in every
relation to the kernels' work split (same 16-column tile / tiles jt and jt+4 of one wave / different waves / the last
partial tile; columns j and j+256 of one thread / two lanes / two waves), the label once the lower and once the higher tied
index; the SSL ties exist only after the per-pair scale has been applied. The matrix-core kernel additionally runs
lo-bearing inputs: one matrix times 1 + 2^-9, so that every non-zero entry has a bfloat16 lo fragment and a dropped
a.lo x b.hi or a.hi x b.lo product moves every logit of one direction by 2^-9 relative. Degenerate indicators hold the SSL
kernel to lvl_clip_loss_fwd bit for bit; indicators other than 0 / 1 count as 1.

Every output is a view into a larger buffer filled with a NaN bit pattern (the same pattern as an int32 sentinel for
argmax), 32 guard rows before and after; the inputs lie between NaN rows. Every launch asserts the guards untouched.

Tolerance of lse and expect (not chosen by running a kernel). tests/test_clip_loss_reference_cpu.py measures, on the CPU,
how far a float32 restatement of the kernels' streaming m / l / ex recurrence and its merges lies from float64 over these
cases (clip and SSL), each row's error taken over max(1, max |logit|) of the row (the SSL bucket expectations: over
max(1, max |dot|)): 3.33e-7, recorded as 3.6e-7. A kernel is allowed 8 x the recorded number (__expf / __logf are the
fast variants; their argument reduction adds an error that grows with |x|): 2.9e-6 per unit of row scale, where the older
slab test allows 1e-4 at scale ~ 14.

The launchers (tests/clip_loss_launch.py) name every device tensor until the launch has completed -- a temporary would hand
its block back to the allocator, and the next allocation could overwrite it before the kernel runs -- and read the
indicators and scales back from the device, bit for bit, before they launch. Both backwards:
tests/test_gpu_clip_loss_bwd_exact.py.
"""
import numpy as np
import pytest
import torch

import clip_loss_launch as K
import clip_loss_reference as R

pytestmark = pytest.mark.gpu

DTYPES = K.DTYPES
_id = lambda s: '-'.join(map(str, s))            # noqa: E731

# what each (B, G, row0) of the matrix-core sweep is there for (asserted from the shape in _assert_reaches)
MFMA_REACHES = {
    (1, 1, 0): ('idle_waves', 'partial_tile', 'partial_row_group'),        # one column, one row: 3 waves carry m = -inf
    (16, 16, 0): ('idle_waves',),                                          # exactly one full tile and one full row group
    (17, 83, 66): ('second_workgroup_partial', 'partial_tile', 'row0_unaligned', 'several_tiles_per_wave'),
    (33, 50, 17): ('second_workgroup_partial', 'partial_tile', 'row0_unaligned'),   # third workgroup: one live row
    (19, 37, 13): ('idle_waves', 'partial_tile', 'second_workgroup_partial', 'row0_unaligned'),   # wave 3 owns no tile
    (5, 300, 295): ('partial_row_group', 'partial_tile', 'row0_unaligned', 'several_tiles_per_wave'),   # rows end at G
    (40, 129, 3): ('second_workgroup_partial', 'partial_tile', 'row0_unaligned', 'several_tiles_per_wave'),
}
# and of the VALU sweep (thread t visits columns t, t + 256, ...)
VALU_REACHES = {
    (1, 1, 0): ('idle_threads', 'idle_waves', 'ends_at_G'),
    (5, 300, 295): ('stride', 'ragged_last_pass', 'ends_at_G'),
    (7, 1025, 500): ('stride', 'ragged_last_pass'),                       # five passes, the last with one live thread
    (3, 63, 11): ('idle_threads', 'idle_waves'),                          # not even one full wave
    (7, 257, 250): ('stride', 'ragged_last_pass', 'ends_at_G'),           # thread 0 alone makes a second pass
    (5, 257, 100): ('stride', 'ragged_last_pass'),
    (3, 1025, 1022): ('stride', 'ragged_last_pass', 'ends_at_G'),
    (3, 63, 60): ('idle_threads', 'idle_waves', 'ends_at_G'),
    (5, 300, 7): ('stride', 'ragged_last_pass'),
}


def _assert_reaches(c):
    key = (c['B'], c['G'], c['row0'])
    table, got = ((MFMA_REACHES, R.mfma_branches(*key)) if c['layout'] == 'mfma' else (VALU_REACHES, R.valu_branches(*key)))
    assert R.uses_mfma(c['E']) == (c['layout'] == 'mfma')
    for tag in table[key]:
        assert got[tag], (key, tag)


_forward = K.clip_forward


def _check_forward_exact(c, dt):
    _assert_reaches(c)
    f = R.case_forward(c)
    B, G = c['B'], c['G']
    stats, argmax, logits = _forward(c, dt)
    tag = (c['kind'], B, G, c['E'], c['row0'], str(dt), c['ties'])
    assert np.array_equal(logits, f['logits']), tag                     # every logit, bit for bit
    assert np.array_equal(argmax, f['argmax']), (tag, argmax, f['argmax'])      # first maximum, on every planted tie
    for lab, oth, _, pos in c['ties']:                                  # (restated: what a wrong rule would flip)
        assert (argmax[:, lab - c['row0']] == min(lab, oth)).all(), tag
    tol = R.fwd_tol(G) * R.row_scale(f['logits'])                       # [2,B]
    assert np.array_equal(stats[..., 1], f['diag']) and np.array_equal(stats[..., 3], f['max']), tag
    err = np.abs(stats[..., 2] - f['expect'])
    print(f'{tag[:6]}: expect err/tol {(err / tol).max():.3f}')
    assert (err <= tol).all(), tag
    err = np.abs(stats[..., 0] - f['lse'])
    print(f'{tag[:6]}: lse err/tol {(err / tol).max():.3f}')
    assert (err <= tol).all(), tag
    # the statistics do not depend on whether the logits slab is asked for
    s2, a2, _ = _forward(c, dt, want_logits=False)
    assert np.array_equal(s2, stats) and np.array_equal(a2, argmax), tag


@pytest.mark.parametrize('dt', DTYPES, ids=('f32', 'bf16'))
@pytest.mark.parametrize('spec', R.CLIP_SPECS, ids=_id)
def test_forward_exact_logits_and_first_index_argmax(spec, dt):
    """logits, diag, max and argmax equal to float64; lse and expect within 8 x the float32 restatement's error; guards
    untouched; the same statistics with and without the logits output"""
    _check_forward_exact(R.exact_case(*spec), dt)


@pytest.mark.parametrize('which', ['img', 'txt'])
@pytest.mark.parametrize('shape', R.MFMA_SHAPES, ids=_id)
def test_forward_exact_with_lo_fragments(shape, which):
    """float32 inputs whose one matrix carries non-zero bfloat16 lo fragments (conditions: clip_loss_reference.lo_case
    and the CPU file): the same bit-exact assertions. Direction 0 needs a.lo x b.hi for 'img' and a.hi x b.lo for 'txt',
    direction 1 the other one; without it every non-zero logit of that direction is off by 2^-9 relative."""
    c = R.lo_case(which, *shape, R.MFMA_SHAPES.index(shape))
    assert c['layout'] == 'mfma' and c['lo'] == which
    _check_forward_exact(c, torch.float32)


# ----------------------------------------------------------------------------------------------------------------------
# lvl_ssl_clip_loss_fwd
# ----------------------------------------------------------------------------------------------------------------------
def _check_ssl_stats(c, f, stats, argmax, logits, tag):
    B, G = c['B'], c['G']
    assert np.array_equal(logits, f['logits']), tag                     # every scaled logit, bit for bit
    assert np.array_equal(argmax, f['argmax']), (tag, argmax, f['argmax'])
    assert np.array_equal(stats[..., 1], f['diag']) and np.array_equal(stats[..., 5], f['diag_dot']), tag
    assert np.array_equal(stats[..., 6], f['max']) and (stats[..., 7] == 0).all(), tag
    tol = R.fwd_tol(G) * R.row_scale(f['logits'])                       # [2,B]
    err = np.abs(stats[..., 0] - f['lse'])
    print(f'{tag[:6]}: lse err/tol {(err / tol).max():.3f}')
    assert (err <= tol).all(), tag
    tol_e = R.fwd_tol(G) * np.maximum(1.0, np.abs(f['dots']).max(-1))   # [2,B]: the expectations are of the unscaled dot
    err = np.abs(stats[..., 2:5] - f['expect'])
    print(f'{tag[:6]}: bucket expectations err/tol {(err / tol_e[..., None]).max():.3f}')
    assert (err <= tol_e[..., None]).all(), tag


@pytest.mark.parametrize('dt', DTYPES, ids=('f32', 'bf16'))
@pytest.mark.parametrize('spec', R.SSL_SPECS, ids=_id)
def test_ssl_forward_exact_logits_and_first_index_argmax(spec, dt):
    """logits, diagonal logit, diagonal dot, max and argmax equal to float64, stats[7] == 0; every planted tie -- it exists
    only after the per-pair scale -- resolves to the lower index; lse and the three bucket expectations within 8 x the
    float32 restatement's error; guards untouched; the same statistics with and without the logits output"""
    c = R.exact_case(*spec)
    _assert_reaches(c)
    f = R.case_forward(c)
    stats, argmax, logits = K.ssl_forward(c, dt)
    tag = (c['kind'], c['B'], c['G'], c['E'], c['row0'], str(dt), c['ties'])
    _check_ssl_stats(c, f, stats, argmax, logits, tag)
    assert len(c['ties']) >= (0 if c['G'] == 1 else 1)
    for lab, oth, _, pos in c['ties']:
        assert c['ind'][lab] != c['ind'][oth]
        assert (f['dots'][:, lab - c['row0'], lab] != f['dots'][:, lab - c['row0'], oth]).all()      # no tie before the scale
        assert (argmax[:, lab - c['row0']] == min(lab, oth)).all(), tag
    s2, a2, _ = K.ssl_forward(c, dt, want_logits=False)
    assert np.array_equal(s2, stats) and np.array_equal(a2, argmax), tag


@pytest.mark.parametrize('dt', DTYPES, ids=('f32', 'bf16'))
@pytest.mark.parametrize('spec', R.SSL_SPECS, ids=_id)
def test_ssl_forward_with_one_indicator_value_is_the_clip_forward(spec, dt):
    """scales3 = (16, 32, 64): all-zero indicators against lvl_clip_loss_fwd at scale 16, all-one at scale 64, at widths
    where both run the same VALU recurrence (a power-of-two scale commutes with every rounding of the dot product):
    logits, lse, diagonal, maximum and argmax bit-identical; E_k * scale against expect within fwd_tol only (the two
    products are rounded at different points); the other two buckets are exactly 0."""
    c = R.exact_case(*spec)
    assert not R.uses_mfma(c['E']) and [float(v) for v in c['scales3']] == [16.0, 32.0, 64.0]
    for value, bucket, scale in ((0, 0, 16.0), (1, 2, 64.0)):
        ind = np.full(c['G'], value, dtype=np.int32)
        st, am, lg = K.ssl_forward(c, dt, ind=ind)
        clip = R.one_value_case(c, value)
        assert float(clip['scale'][0]) == scale
        st_c, am_c, lg_c = K.clip_forward(clip, dt)
        tag = (spec, str(dt), value)
        assert np.array_equal(lg, lg_c) and np.array_equal(am, am_c), tag
        assert np.array_equal(st[..., 0], st_c[..., 0]) and np.array_equal(st[..., 1], st_c[..., 1]), tag
        assert np.array_equal(st[..., 6], st_c[..., 3]) and np.array_equal(st[..., 5] * scale, st_c[..., 1]), tag
        others = [k for k in range(3) if k != bucket]
        assert (st[..., 2:5][..., others] == 0).all() and (st[..., 7] == 0).all(), tag
        f = R.case_forward(clip)
        assert np.array_equal(lg, f['logits']), tag
        tol = R.fwd_tol(c['G']) * R.row_scale(f['logits'])
        assert (np.abs(st[..., 2 + bucket] * scale - f['expect']) <= tol).all(), tag
        assert (np.abs(st_c[..., 2] - f['expect']) <= tol).all(), tag


@pytest.mark.parametrize('dt', DTYPES, ids=('f32', 'bf16'))
@pytest.mark.parametrize('spec', R.SSL_SPECS[1:6:2], ids=_id)
def test_ssl_forward_reads_any_nonzero_indicator_as_one(spec, dt):
    """indicators drawn from {0, 1, 2, -1, 7}: every output bit-identical to the launch on their 0 / 1 images"""
    c = R.exact_case(*spec)
    wild = K.wild_indicators(c['ind'], seed=spec[-1])
    got = K.ssl_forward(c, dt, ind=wild)
    want = K.ssl_forward(c, dt)
    for a, b in zip(got, want):
        assert np.array_equal(a, b), (spec, str(dt))
