"""Launchers of the four contrastive-head entry points for the GPU tests (tests/test_gpu_clip_loss_exact.py,
tests/test_gpu_clip_loss_bwd_exact.py), through the C ABI. Imported only by tests marked gpu.

Every launcher
  * keeps every device tensor in a local name until torch.cuda.synchronize() has returned: a temporary would hand its
    block back to the caching allocator as soon as its pointer has been taken, and the next upload could overwrite it
    before the kernel reads it (the indicators of a small case and the three scales share the allocator's smallest block);
  * reads the small inputs -- indicators, scale(s), upstream, lse_all -- BACK from the device right before the launch and
    asserts them bit-equal to the host arrays: a launch on overwritten indicators cannot happen;
  * places the embeddings between NaN rows and every output inside a buffer filled with a NaN bit pattern (the same
    pattern as an int32 sentinel for argmax), 32 guard rows before and after, and asserts the guards untouched.
"""
import numpy as np
import torch

DEV = 'cuda'
GUARD = 32                      # rows; more than the 15 a 16-row workgroup could overrun by
SENT32 = 0x7FA5A5A5             # a NaN payload nobody computes; the int32 sentinel of the argmax guards
DTYPES = (torch.float32, torch.bfloat16)


def lib():
    from lavila_amd import _cabi as C
    return C, C.lib()


def guarded(rows, width, dtype=torch.float32):
    """(buffer, view of its rows GUARD .. GUARD + rows): every word of the buffer starts as the sentinel"""
    buf = torch.empty(rows + 2 * GUARD, width, dtype=dtype, device=DEV)
    buf.view(torch.int32).fill_(SENT32)
    return buf, buf[GUARD:GUARD + rows]


def untouched(buf, rows):
    w = buf.view(torch.int32)
    return bool((w[:GUARD] == SENT32).all()) and bool((w[GUARD + rows:] == SENT32).all())


def all_sentinel(buf):
    return bool((buf.view(torch.int32) == SENT32).all())


def guarded_in(x, dt):
    """x [G,E] (numpy float32) in dtype dt between NaN rows"""
    t = torch.from_numpy(np.ascontiguousarray(x))
    buf = torch.full((t.shape[0] + 2 * GUARD, t.shape[1]), float('nan'), dtype=dt, device=DEV)
    buf[GUARD:GUARD + t.shape[0]] = t.to(DEV, dt)
    assert torch.equal(buf[GUARD:GUARD + t.shape[0]].float().cpu(), t)            # the dtype holds the values exactly
    return buf[GUARD:GUARD + t.shape[0]]


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4
    return a.view(np.uint32).reshape(-1)


def small(host, np_dtype):
    """host array -> (device tensor, the host array in the kernel's 32-bit type)"""
    h = np.ascontiguousarray(np.asarray(host), dtype=np_dtype)
    return torch.from_numpy(h.copy()).to(DEV), h


def assert_device_holds(*pairs):
    """the precondition of every launch: each (device tensor, host array) pair is bit-equal NOW, all uploads done"""
    torch.cuda.synchronize()
    for t, h in pairs:
        if t is None:
            continue
        got = t.cpu().numpy()
        assert got.dtype == h.dtype and np.array_equal(_bits(got), _bits(h)), 'a device input no longer holds its host values'


def clip_forward(c, dt, want_logits=True):
    """one lvl_clip_loss_fwd launch into guarded outputs -> stats [2,B,4], argmax [2,B], logits [2,B,G] (CPU, float64 /
    int)"""
    C, L = lib()
    B, G, E, row0 = c['B'], c['G'], c['E'], c['row0']
    W = 4
    img, txt = guarded_in(c['img'], dt), guarded_in(c['txt'], dt)
    sbuf, stats = guarded(2 * B, W)
    abuf, argmax = guarded(2 * B, 1, torch.int32)
    lbuf, logits = guarded(2 * B, G) if want_logits else (None, None)
    scale, scale_h = small(c['scale'], np.float32)
    assert_device_holds((scale, scale_h))
    rc = L.lvl_clip_loss_fwd(C.ptr(img), C.ptr(txt), C.ptr(scale), B, G, E, row0, C.ptr(stats), C.ptr(argmax),
                             C.ptr(logits), C.dtype_code(img), C.stream_ptr())
    C.check(rc, 'forward')
    torch.cuda.synchronize()
    assert untouched(sbuf, 2 * B), 'stats written outside [2,B,W]'
    assert untouched(abuf, 2 * B), 'argmax written outside [2,B]'
    assert lbuf is None or untouched(lbuf, 2 * B), 'logits written outside [2,B,G]'
    return (stats.double().cpu().numpy().reshape(2, B, W), argmax.cpu().numpy().reshape(2, B),
            logits.double().cpu().numpy().reshape(2, B, G) if want_logits else None)


def ssl_forward(c, dt, want_logits=True, ind=None):
    """one lvl_ssl_clip_loss_fwd launch -> stats [2,B,8], argmax [2,B], logits [2,B,G]; `ind` replaces the case's
    indicators"""
    C, L = lib()
    B, G, E, row0 = c['B'], c['G'], c['E'], c['row0']
    W = 8
    img, txt = guarded_in(c['img'], dt), guarded_in(c['txt'], dt)
    sbuf, stats = guarded(2 * B, W)
    abuf, argmax = guarded(2 * B, 1, torch.int32)
    lbuf, logits = guarded(2 * B, G) if want_logits else (None, None)
    ind_d, ind_h = small(c['ind'] if ind is None else ind, np.int32)
    s3_d, s3_h = small(c['scales3'], np.float32)
    assert ind_h.shape == (G,) and s3_h.shape == (3,)
    assert_device_holds((ind_d, ind_h), (s3_d, s3_h))
    rc = L.lvl_ssl_clip_loss_fwd(C.ptr(img), C.ptr(txt), C.ptr(ind_d), C.ptr(s3_d), B, G, E, row0, C.ptr(stats),
                                 C.ptr(argmax), C.ptr(logits), C.dtype_code(img), C.stream_ptr())
    C.check(rc, 'ssl forward')
    torch.cuda.synchronize()
    assert untouched(sbuf, 2 * B), 'stats written outside [2,B,W]'
    assert untouched(abuf, 2 * B), 'argmax written outside [2,B]'
    assert lbuf is None or untouched(lbuf, 2 * B), 'logits written outside [2,B,G]'
    return (stats.double().cpu().numpy().reshape(2, B, W), argmax.cpu().numpy().reshape(2, B),
            logits.double().cpu().numpy().reshape(2, B, G) if want_logits else None)


def _grads_out(B, E):
    ibuf, dimg = guarded(B, E)
    tbuf, dtxt = guarded(B, E)
    return ibuf, dimg, tbuf, dtxt


def _row_ptr(C, buf):
    """address of row GUARD of a guarded buffer (an empty view, B = 0, has no address of its own)"""
    return C.ptr(buf[GUARD:])


def _grads_back(B, E, ibuf, dimg, tbuf, dtxt):
    assert untouched(ibuf, B), 'dimg written outside [B,E]'
    assert untouched(tbuf, B), 'dtxt written outside [B,E]'
    if B == 0:
        assert all_sentinel(ibuf) and all_sentinel(tbuf)
    return np.stack([dimg.cpu().numpy().reshape(B, E), dtxt.cpu().numpy().reshape(B, E)])


def clip_backward(c, dt, lse32, coef, upstream, rows_only=False, B=None, scale=None):
    """one lvl_clip_loss_bwd launch into guarded gradients -> [2,B,E] float32 (dimg, dtxt). upstream None = NULL;
    `B` / `scale` replace the case's."""
    C, L = lib()
    B = c['B'] if B is None else B
    G, E, row0 = c['G'], c['E'], c['row0']
    img, txt = guarded_in(c['img'], dt), guarded_in(c['txt'], dt)
    outs = _grads_out(B, E)
    lse_d, lse_h = small(lse32, np.float32)
    sc_d, sc_h = small(c['scale'] if scale is None else [scale], np.float32)
    up_d, up_h = (None, None) if upstream is None else small(upstream, np.float32)
    assert lse_h.shape == (2, G) and sc_h.shape == (1,)
    assert_device_holds((lse_d, lse_h), (sc_d, sc_h), (up_d, up_h))
    rc = L.lvl_clip_loss_bwd(C.ptr(img), C.ptr(txt), C.ptr(lse_d), C.ptr(sc_d), C.ptr(up_d), float(coef), B, G, E, row0,
                             int(rows_only), _row_ptr(C, outs[0]), _row_ptr(C, outs[2]), C.dtype_code(img), C.stream_ptr())
    C.check(rc, 'backward')
    torch.cuda.synchronize()
    return _grads_back(B, E, *outs)


def ssl_backward(c, dt, lse32, coef, upstream, B=None, ind=None):
    """one lvl_ssl_clip_loss_bwd launch into guarded gradients -> [2,B,E] float32"""
    C, L = lib()
    B = c['B'] if B is None else B
    G, E, row0 = c['G'], c['E'], c['row0']
    img, txt = guarded_in(c['img'], dt), guarded_in(c['txt'], dt)
    outs = _grads_out(B, E)
    lse_d, lse_h = small(lse32, np.float32)
    ind_d, ind_h = small(c['ind'] if ind is None else ind, np.int32)
    s3_d, s3_h = small(c['scales3'], np.float32)
    up_d, up_h = (None, None) if upstream is None else small(upstream, np.float32)
    assert lse_h.shape == (2, G) and ind_h.shape == (G,) and s3_h.shape == (3,)
    assert_device_holds((lse_d, lse_h), (ind_d, ind_h), (s3_d, s3_h), (up_d, up_h))
    rc = L.lvl_ssl_clip_loss_bwd(C.ptr(img), C.ptr(txt), C.ptr(ind_d), C.ptr(lse_d), C.ptr(s3_d), C.ptr(up_d), float(coef),
                                 B, G, E, row0, _row_ptr(C, outs[0]), _row_ptr(C, outs[2]), C.dtype_code(img), C.stream_ptr())
    C.check(rc, 'ssl backward')
    torch.cuda.synchronize()
    return _grads_back(B, E, *outs)


def wild_indicators(ind, seed):
    """indicators whose non-zero entries are drawn from {1, 2, -1, 7} (all four present when there are enough), zeros kept"""
    ind = np.asarray(ind)
    rng = np.random.default_rng(seed)
    out = np.where(ind != 0, rng.choice(np.int32([1, 2, -1, 7]), size=ind.shape), 0).astype(np.int32)
    assert np.array_equal(out != 0, ind != 0) and set(np.unique(out)) <= {0, 1, 2, -1, 7}
    assert ind.sum() < 8 or {2, -1, 7} <= set(np.unique(out))
    return out
