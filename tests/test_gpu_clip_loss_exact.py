"""GPU (-m gpu): lvl_clip_loss_fwd -- the matrix-core kernel for E in 64/128/256/512 and the VALU kernel for every other
width -- through the C ABI against the float64 slab reference (tests/clip_loss_reference.py), on inputs whose logits are
EXACT in float32 (so the logits slab, the diagonal, the maximum and the argmax under "first maximum kept" must be equal
to the reference bit for bit), with the row maximum tied at planted column pairs in every relation to the kernels' work
split (same 16-column tile / tiles jt and jt+4 of one wave / different waves / the last partial tile; columns j and j+256
of one thread / two lanes / two waves), the label once the lower and once the higher tied index. Every output is a view
into a larger buffer filled with a NaN bit pattern (the same pattern as an int32 sentinel for argmax), 32 guard rows
before and after; the inputs lie between NaN rows. Every test asserts the guards untouched.

Tolerance of lse and expect (not chosen by running a kernel). tests/test_clip_loss_reference_cpu.py measures, on the CPU,
how far a float32 restatement of the kernels' streaming m / l / ex recurrence and its merges lies from float64 over these
cases, each row's error taken over max(1, max |logit|) of the row: 3.33e-7, recorded as 3.6e-7. A kernel is allowed 8 x the
recorded number (__expf / __logf are the fast variants; their argument reduction adds an error that grows with |x|):
2.9e-6 per unit of row scale, where the older slab test allows 1e-4 at scale ~ 14.

This file covers lvl_clip_loss_fwd only. The launcher names every device tensor until its launch has completed: a
temporary would hand its block back to the allocator, and the next allocation could overwrite it before the kernel runs.
"""
import numpy as np
import pytest
import torch

import clip_loss_reference as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
GUARD = 32                      # rows; more than the 15 a 16-row workgroup could overrun by
SENT32 = 0x7FA5A5A5             # a NaN payload nobody computes; the int32 sentinel of the argmax guards
DTYPES = (torch.float32, torch.bfloat16)
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


def _lib():
    from lavila_amd import _cabi as C
    return C, C.lib()


def _guarded(rows, width, dtype=torch.float32):
    """(buffer, view of its rows GUARD .. GUARD + rows): every word of the buffer starts as the sentinel"""
    buf = torch.empty(rows + 2 * GUARD, width, dtype=dtype, device=DEV)
    buf.view(torch.int32).fill_(SENT32)
    return buf, buf[GUARD:GUARD + rows]


def _untouched(buf, rows):
    w = buf.view(torch.int32)
    return bool((w[:GUARD] == SENT32).all()) and bool((w[GUARD + rows:] == SENT32).all())


def _guarded_in(x, dt):
    """x [G,E] (numpy float32) in dtype dt between NaN rows"""
    t = torch.from_numpy(np.ascontiguousarray(x))
    buf = torch.full((t.shape[0] + 2 * GUARD, t.shape[1]), float('nan'), dtype=dt, device=DEV)
    buf[GUARD:GUARD + t.shape[0]] = t.to(DEV, dt)
    assert torch.equal(buf[GUARD:GUARD + t.shape[0]].float().cpu(), t)            # the dtype holds the values exactly
    return buf[GUARD:GUARD + t.shape[0]]


def _dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


def _forward(c, dt, want_logits=True):
    """one lvl_clip_loss_fwd launch into guarded outputs -> stats [2,B,4], argmax [2,B], logits [2,B,G] (CPU, float64 /
    int)"""
    C, lib = _lib()
    B, G, E, row0 = c['B'], c['G'], c['E'], c['row0']
    assert c['kind'] == 'clip'
    W = 4
    img, txt = _guarded_in(c['img'], dt), _guarded_in(c['txt'], dt)
    sbuf, stats = _guarded(2 * B, W)
    abuf, argmax = _guarded(2 * B, 1, torch.int32)
    lbuf, logits = _guarded(2 * B, G) if want_logits else (None, None)
    # every device tensor keeps a name until the launch has completed: a temporary would hand its block back to the
    # allocator, and the next temporary could overwrite it before the kernel reads it
    scale = _dev(c['scale'])
    rc = lib.lvl_clip_loss_fwd(C.ptr(img), C.ptr(txt), C.ptr(scale), B, G, E, row0, C.ptr(stats), C.ptr(argmax),
                               C.ptr(logits), C.dtype_code(img), C.stream_ptr())
    C.check(rc, 'forward')
    torch.cuda.synchronize()
    assert _untouched(sbuf, 2 * B), 'stats written outside [2,B,W]'
    assert _untouched(abuf, 2 * B), 'argmax written outside [2,B]'
    assert lbuf is None or _untouched(lbuf, 2 * B), 'logits written outside [2,B,G]'
    return (stats.double().cpu().numpy().reshape(2, B, W), argmax.cpu().numpy().reshape(2, B),
            logits.double().cpu().numpy().reshape(2, B, G) if want_logits else None)


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
