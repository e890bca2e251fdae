"""Float64 restatement of the contrastive-head kernels (lavila_amd/csrc/clip_loss.hip, clip_loss_mfma.hip), slab-wise:
nothing here ever forms the G x G logit matrix. CPU only, numpy float64.

  slab_forward / ssl_slab_forward      logits [2,B,G], the statistics the kernels emit, argmax under "first maximum"
  slab_backward / ssl_slab_backward    the gradient of the local rows from the SAME lse_all array the kernel is handed
                                       (it is an input of the kernel), the per-element magnitude sum
                                       |k| sum_j |c_ij| |b_je|, and the un-cancelled one |k| sum_j s (p + p' + 2 delta) |b|
                                       that the device tests use as the error scale
  lse_all                              all 2 G row / column log-sum-exps in float64, equal rows grouped, by column chunks
  backward_f32                         float32 restatement of the backward kernels' arithmetic: its distance from
                                       float64 per class of cases is where the tolerances of
                                       tests/test_gpu_clip_loss_bwd_exact.py come from
  lo_case                              exact matrix-core cases whose one matrix carries non-zero bfloat16 lo fragments
  exact_inputs                         embeddings whose logits are exact in float32 in ANY summation order, with planted
                                       ties of the row maximum in a chosen relation to the kernels' work split
  stream_f32                           float32 restatement of the forward kernels' arithmetic (streaming m/l/ex recurrence
                                       with its merges): its distance from float64 is where the lse / expect tolerance
                                       of tests/test_gpu_clip_loss_exact.py comes from
  CASES ...                            the case lists the CPU and the GPU test files share

Layout facts restated from the kernels (the predicates below are what the tests assert a case reaches):
  matrix-core forward (E in 64/128/256/512): one workgroup per 16 local rows; wave w of 4 sweeps the 16-column tiles
      w, w+4, w+8, ...; lane column c = j % 16. Merges: per lane over its tiles, over the 16 column lanes, over the 4 waves.
  VALU forward (any other E, and every SSL launch): one workgroup of 256 threads per row; thread t sweeps the columns
      t, t+256, ...; merges: per thread, over the 64 lanes of a wave, over the 4 waves.
"""
import functools

import numpy as np

MFMA_WIDTHS = (64, 128, 256, 512)
LDS_LIMIT_BYTES = 150 * 1024            # a coefficient row (E + G) * 4 beyond this is refused by the backward's host side


def uses_mfma(E):
    return E in MFMA_WIDTHS


# ----------------------------------------------------------------------------------------------------------------------
# where two columns sit in the kernels' work split
# ----------------------------------------------------------------------------------------------------------------------
MFMA_RELATIONS = ('same_tile', 'same_wave', 'cross_wave', 'partial_tile')
VALU_RELATIONS = ('same_thread', 'same_wave', 'cross_wave')


def mfma_relation(a, b, G):
    """relation of columns a, b (arrays broadcast) in the matrix-core sweep: 'partial_tile' = both in the last, partial
    16-column tile (then the lower of two tied indices lies in it); 'same_tile' = one full tile; 'same_wave' = tiles jt and
    jt + 4n of one wave; 'cross_wave' = tiles of different waves."""
    a, b = np.broadcast_arrays(np.asarray(a), np.asarray(b))
    ta, tb = a // 16, b // 16
    last = (G - 1) // 16
    out = np.where(ta == tb, 'same_tile', np.where(ta % 4 == tb % 4, 'same_wave', 'cross_wave')).astype(object)
    out[(ta == tb) & (ta == last) & (G % 16 != 0)] = 'partial_tile'
    return out


def valu_relation(a, b, G=None):
    """relation of columns a, b in the VALU sweep: 'same_thread' = j and j + 256 n; 'same_wave' = two lanes of one wave;
    'cross_wave' = two different waves."""
    a, b = np.broadcast_arrays(np.asarray(a), np.asarray(b))
    ta, tb = a % 256, b % 256
    return np.where(ta == tb, 'same_thread', np.where(ta // 64 == tb // 64, 'same_wave', 'cross_wave')).astype(object)


def mfma_branches(B, G, row0):
    """what a shape makes clip_fwd_mfma_kernel do, from the shape alone"""
    ntiles = (G + 15) // 16
    return {'idle_waves': ntiles < 4,                       # some of the 4 waves own no tile: m = -inf into the merge
            'partial_tile': G % 16 != 0,                    # clamped column loads, j < G guard
            'several_tiles_per_wave': ntiles > 4,
            'partial_row_group': B % 16 != 0,               # clamped row loads, i < B guard
            'second_workgroup_partial': B > 16 and B % 16 != 0,
            'row0_unaligned': row0 % 16 != 0}               # diagonal j == row0 + i against the C-layout row mapping


def valu_branches(B, G, row0):
    return {'idle_threads': G < 256, 'idle_waves': G <= 192, 'stride': G > 256,     # a thread visits j and j + 256
            'ragged_last_pass': G > 256 and G % 256 != 0, 'ends_at_G': row0 + B == G}


# ----------------------------------------------------------------------------------------------------------------------
# float64 slabs
# ----------------------------------------------------------------------------------------------------------------------
def _f64(x):
    try:
        import torch
        if isinstance(x, torch.Tensor):
            x = x.detach().cpu()
            x = (x.double() if x.is_floating_point() else x).numpy()
    except ImportError:
        pass
    return np.asarray(x, dtype=np.float64) if np.asarray(x).dtype.kind == 'f' else np.asarray(x)


def _sides(img_all, txt_all, B, row0):
    """(own rows [B,E], partner matrix [G,E]) for direction 0 (image rows) and 1 (text rows)"""
    img, txt = _f64(img_all), _f64(txt_all)
    return ((img[row0:row0 + B], txt), (txt[row0:row0 + B], img))


def _row_stats(z):
    """z [B,G] float64 -> lse, softmax p, max, first argmax"""
    m = z.max(-1)
    e = np.exp(z - m[:, None])
    s = e.sum(-1)
    return m + np.log(s), e / s[:, None], m, z.argmax(-1).astype(np.int32)      # numpy's argmax keeps the first maximum


def slab_forward(img_all, txt_all, scale, B, row0):
    """-> logits [2,B,G], stats dict of [2,B] arrays {lse, diag, expect, max}, argmax [2,B] int32 (first index)."""
    scale = float(np.asarray(_f64(scale)).reshape(-1)[0])
    idx = np.arange(row0, row0 + B)
    L, S, A = [], {k: [] for k in ('lse', 'diag', 'expect', 'max')}, []
    for own, other in _sides(img_all, txt_all, B, row0):
        z = (scale * own) @ other.T
        lse, p, m, am = _row_stats(z)
        L.append(z)
        S['lse'].append(lse)
        S['diag'].append(z[np.arange(B), idx])
        S['expect'].append((p * z).sum(-1))
        S['max'].append(m)
        A.append(am)
    return np.stack(L), {k: np.stack(v) for k, v in S.items()}, np.stack(A)


def stats4(stats):
    """the dict of slab_forward in the kernel's [2,B,4] layout"""
    return np.stack([stats['lse'], stats['diag'], stats['expect'], stats['max']], -1)


def ssl_slab_forward(img_all, txt_all, ind_all, scales3, B, row0):
    """-> logits [2,B,G], stats [2,B,8] = {lse, diag logit, E0, E1, E2, diag dot, max, 0} as ssl_fwd_kernel lays them out
    (E_k = sum over the columns of bucket k = ind_i + ind_j of softmax_ij * unscaled dot_ij), argmax [2,B], dots [2,B,G]."""
    ind = np.asarray(_f64(ind_all)).astype(np.int64)
    s3 = _f64(scales3).reshape(3)
    idx, rows = np.arange(row0, row0 + B), np.arange(B)
    bucket = ind[row0:row0 + B, None] + ind[None, :]
    L, D, S, A = [], [], [], []
    for own, other in _sides(img_all, txt_all, B, row0):
        d = own @ other.T
        z = d * s3[bucket]
        lse, p, m, am = _row_stats(z)
        ek = [(p * d * (bucket == k)).sum(-1) for k in range(3)]
        S.append(np.stack([lse, z[rows, idx], ek[0], ek[1], ek[2], d[rows, idx], m, np.zeros(B)], -1))
        L.append(z)
        D.append(d)
        A.append(am)
    return np.stack(L), np.stack(S), np.stack(A), np.stack(D)


def _backward(img_all, txt_all, lse_all, B, row0, k, rows_only, pair_scale):
    """shared body: c_ij from the logits and the given LSEs, grad = k sum_j c_ij b_j, mag = |k| sum_j |c_ij| |b_j|, and
    the UN-CANCELLED magnitude umag = |k| sum_j s_ij (p_ij + p'_ij + 2 delta_ij) |b_je| (rows_only: p_ij + delta_ij) --
    the sum of the terms as they stand before the diagonal subtraction. pair_scale(i_global [B,1], j [1,G]) -> the
    per-pair temperature [B,G]. -> (grad_img, grad_txt, mag_img, mag_txt, umag_img, umag_txt)."""
    lse = _f64(lse_all).reshape(2, -1)
    G = lse.shape[1]
    idx, rows = np.arange(row0, row0 + B), np.arange(B)
    s = pair_scale(idx[:, None], np.arange(G)[None, :])
    grads, mags, umags = [], [], []
    for d, (own, other) in enumerate(_sides(img_all, txt_all, B, row0)):
        z = s * (own @ other.T)
        own_l = lse[d, idx][:, None]
        if rows_only:                                   # the partner LSEs are not read (they may be NaN)
            c = np.exp(z - own_l)
            diag = 1.0
        else:
            c = np.exp(z - own_l) + np.exp(z - lse[1 - d][None, :])
            diag = 2.0
        u = c.copy()
        u[rows, idx] += diag
        c[rows, idx] -= diag
        c = c * s
        grads.append(k * (c @ other))
        mags.append(abs(k) * (np.abs(c) @ np.abs(other)))
        umags.append(abs(k) * ((u * s) @ np.abs(other)))
    return grads[0], grads[1], mags[0], mags[1], umags[0], umags[1]


def slab_backward(img_all, txt_all, lse_all, scale, upstream, coef, B, row0, rows_only=False, uncancelled=False):
    """lvl_clip_loss_bwd in float64 -> dimg [B,E], dtxt [B,E], mag_img, mag_txt (and, with `uncancelled`, the two
    un-cancelled magnitudes). With k = coef * upstream, d/d(own row) = k * scale * sum_j c_ij b_j; the per-pair
    temperature is the one scale."""
    scale = float(np.asarray(_f64(scale)).reshape(-1)[0])
    up = 1.0 if upstream is None else float(np.asarray(_f64(upstream)).reshape(-1)[0])
    out = _backward(img_all, txt_all, lse_all, B, row0, coef * up, rows_only,
                    lambda i, j: np.full(np.broadcast(i, j).shape, scale))
    return out if uncancelled else out[:4]


def ssl_slab_backward(img_all, txt_all, ind_all, lse_all, scales3, upstream, coef, B, row0, uncancelled=False):
    ind = np.asarray(_f64(ind_all)).astype(np.int64)
    s3 = _f64(scales3).reshape(3)
    up = 1.0 if upstream is None else float(np.asarray(_f64(upstream)).reshape(-1)[0])
    out = _backward(img_all, txt_all, lse_all, B, row0, coef * up, False, lambda i, j: s3[ind[i] + ind[j]])
    return out if uncancelled else out[:4]


def _lse_args(img_all, txt_all, scale, ind_all, scales3):
    img, txt = _f64(img_all), _f64(txt_all)
    G = img.shape[0]
    ind = np.zeros(G, dtype=np.int64) if ind_all is None else np.asarray(_f64(ind_all)).astype(np.int64)
    if scales3 is None:
        s = float(np.asarray(_f64(scale)).reshape(-1)[0])
        s3 = np.array([s, s, s])
    else:
        s3 = _f64(scales3).reshape(3)
    return img, txt, ind, s3, G


def lse_all_chunked(img_all, txt_all, scale=None, ind_all=None, scales3=None, chunk=512):
    """All 2 G true LSEs in float64, [2,G], every row against every column, `chunk` columns at a time (at most G x chunk
    logits exist at once). What lse_all is checked against at G <= 1025."""
    img, txt, ind, s3, G = _lse_args(img_all, txt_all, scale, ind_all, scales3)
    row_m, row_s = np.full(G, -np.inf), np.zeros(G)
    col = np.empty(G)
    for c0 in range(0, G, chunk):
        c1 = min(G, c0 + chunk)
        z = (img @ txt[c0:c1].T) * s3[ind[:, None] + ind[None, c0:c1]]
        mn = np.maximum(row_m, z.max(1))
        row_s = row_s * np.exp(row_m - mn) + np.exp(z - mn[:, None]).sum(1)
        row_m = mn
        cm = z.max(0)
        col[c0:c1] = cm + np.log(np.exp(z - cm[None, :]).sum(0))
    return np.stack([row_m + np.log(row_s), col])


def _distinct(x, ind):
    """distinct (row, indicator) pairs -> rows [U,E], indicators [U], index of each original row [G], counts [U]"""
    key = np.concatenate([x, ind[:, None].astype(np.float64)], axis=1)
    u, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    return u[:, :-1], u[:, -1].astype(np.int64), inv.reshape(-1), cnt.astype(np.float64)


def lse_all(img_all, txt_all, scale=None, ind_all=None, scales3=None, chunk=512):
    """All 2 G true LSEs in float64, [2,G]: row 0 = rows of logits_per_image, row 1 = rows of logits_per_text. Equal
    rows are grouped: every distinct (row, indicator) of either matrix is computed once and enters the other side's sums
    weighted by its count (sparse ternary rows at E = 8 have about a hundred distinct ones, whatever G), visiting the
    distinct columns `chunk` at a time."""
    img, txt, ind, s3, G = _lse_args(img_all, txt_all, scale, ind_all, scales3)
    a, ia, inv_a, na = _distinct(img, ind)
    b, ib, inv_b, nb = _distinct(txt, ind)
    row_m, row_s = np.full(len(a), -np.inf), np.zeros(len(a))
    col = np.empty(len(b))
    for c0 in range(0, len(b), chunk):
        c1 = min(len(b), c0 + chunk)
        z = (a @ b[c0:c1].T) * s3[ia[:, None] + ib[None, c0:c1]]
        mn = np.maximum(row_m, z.max(1))
        row_s = row_s * np.exp(row_m - mn) + (np.exp(z - mn[:, None]) * nb[None, c0:c1]).sum(1)
        row_m = mn
        cm = z.max(0)
        col[c0:c1] = cm + np.log((np.exp(z - cm[None, :]) * na[:, None]).sum(0))
    return np.stack([(row_m + np.log(row_s))[inv_a], col[inv_b]])


# ----------------------------------------------------------------------------------------------------------------------
# exact-logit inputs with planted ties
# ----------------------------------------------------------------------------------------------------------------------
def _is_bf16(x):
    """every float32 value survives the round trip through bfloat16 (its low 16 bits are zero)"""
    return bool((np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & 0xFFFF == 0).all())


def plan_ties(B, G, row0, relation_of, relations, first=0, limit=None, rows_available=None):
    """Picks disjoint column pairs (label, other, relation, position): `label` = global index of a local row, `other` any
    column, in the asked relation, with the label the 'lower' or the 'higher' of the two. Combinations are tried in a
    fixed order rotated by `first`; those the shape cannot host are skipped. -> list of tuples."""
    combos = [(r, p) for r in relations for p in ('lower', 'higher')]
    combos = combos[first % len(combos):] + combos[:first % len(combos)]
    used = np.zeros(G, dtype=bool)
    cols = np.arange(G)
    out = []
    for rel, pos in combos:
        if limit is not None and len(out) >= limit:
            break
        found = None
        for lab in range(row0, row0 + B):
            if used[lab]:
                continue
            ok = (relation_of(lab, cols, G) == rel) & ~used & (cols != lab) & ((cols > lab) if pos == 'lower' else (cols < lab))
            hit = np.flatnonzero(ok)
            if hit.size:
                found = (lab, int(hit[hit.size // 2]))
                break
        if found:
            used[list(found)] = True
            out.append((found[0], found[1], rel, pos))
    return out


def exact_inputs(B, G, E, row0, scale, k, nnz, seed, ties=(), ssl=False, scales3=(16.0, 32.0, 64.0)):
    """Embeddings [G,E] float32 with entries in {-1, 0, +1} * 2^-k (planted SSL partner rows: 2^-(k-1)) and `nnz`
    non-zeros per ordinary row, for a power-of-two scale. Asserted here, from the inputs alone:
      * every embedding entry and every scaled entry is a bfloat16 value (the matrix-core hi/lo split has lo = 0);
      * every product is an integer multiple of one unit u, and max_ij sum_e |a_ie| |b_je| * scale / u < 2^24: every
        partial sum, in any order, is an integer multiple of u below 2^24 u, hence exact in float32;
      * for every planted tie (label, other): in BOTH directions the maximum of row `label` is attained at exactly the
        two columns {label, other}.
    Plain ties: rows label and other of both matrices carry one pattern with nnz + 1 non-zeros, so their dot products
    exceed any that involves an ordinary row. SSL ties: ind[label] != ind[other], and the dots differ
    by the factor that the per-pair scales {pseudo, sqrt(pseudo real), real} = {16, 32, 64} undo -- the tie exists only
    after the scale is applied. -> dict(img, txt, ind, scale or scales3, ties)."""
    assert float(scale) in (16.0, 64.0) and k >= 1 and 1 <= nnz < E
    s3 = np.asarray(scales3, dtype=np.float64)
    wide = min(E, 2 * nnz + 2) // 2 * 2 if ssl else nnz + 1    # non-zeros of a planted pattern (SSL: halved for one kind)
    mag = 2.0 ** -k
    for attempt in range(400):
        rng = np.random.default_rng(seed * 1000 + attempt)

        def sparse(n, count):
            x = np.zeros((n, E), dtype=np.float32)
            pos = np.argsort(rng.random((n, E)), axis=1)[:, :count]
            x[np.arange(n)[:, None], pos] = rng.choice(np.float32([-mag, mag]), size=(n, count))
            return x
        img, txt = sparse(G, nnz), sparse(G, nnz)
        ind = (rng.random(G) < 0.5).astype(np.int32)
        if G > 1:
            ind[0], ind[1] = 1, 0
        for n, (lab, oth, _, _) in enumerate(ties):
            p = sparse(1, wide)[0]
            q = p.copy()
            if ssl:
                t = n % 2
                ind[lab], ind[oth] = t, 1 - t
                if t == 0:          # label pair scaled by pseudo = 16, the other by 32: the other's dot is half
                    nz = np.flatnonzero(p)
                    q[nz[len(nz) // 2:]] = 0
                else:               # label pair scaled by real = 64, the other by 32: the other's dot is double
                    q = 2 * p
            img[lab] = txt[lab] = p
            img[oth] = txt[oth] = q
        if _ties_hold(img, txt, ind, scale, s3, ssl, ties):
            break
    else:
        raise AssertionError(f'no exact-tie inputs for B={B} G={G} E={E} row0={row0} ties={ties}')
    # exactness, from the inputs
    assert _is_bf16(img) and _is_bf16(txt)
    if not ssl:
        assert _is_bf16(np.float32(scale) * img) and _is_bf16(np.float32(scale) * txt)
    else:
        assert all(float(np.log2(v)).is_integer() for v in s3)
    unit = mag * mag * (1.0 if ssl else float(scale))          # planted SSL rows (2 mag) give multiples of it too
    for m in (img, txt):
        assert np.array_equal(np.round(m.astype(np.float64) / mag), m.astype(np.float64) / mag)
    top = (s3.max() if ssl else float(scale)) * np.abs(img).astype(np.float64).sum(1).max() * np.abs(txt).astype(np.float64).max()
    top = max(top, (s3.max() if ssl else float(scale)) * np.abs(txt).astype(np.float64).sum(1).max() * np.abs(img).astype(np.float64).max())
    assert top / unit < 2 ** 24, (top, unit)                 # bound on sum_e |a_e| |b_e| * scale for every pair
    out = {'img': img, 'txt': txt, 'ind': ind, 'ties': list(ties)}
    out['scales3' if ssl else 'scale'] = np.float32(s3) if ssl else np.float32([scale])
    return out


def _ties_hold(img, txt, ind, scale, s3, ssl, ties):
    a, b = img.astype(np.float64), txt.astype(np.float64)
    for lab, oth, _, _ in ties:
        for own, other in ((a, b), (b, a)):
            z = other @ own[lab]
            z = z * (s3[ind[lab] + ind] if ssl else float(scale))
            if set(np.flatnonzero(z == z.max()).tolist()) != {lab, oth}:
                return False
    return True


# ----------------------------------------------------------------------------------------------------------------------
# float32 restatements of the kernels' arithmetic (the source of the tolerances)
# ----------------------------------------------------------------------------------------------------------------------
F32 = np.float32


def stream_f32(z, layout, weights=None):
    """The forward kernels' streaming softmax in float32: per-thread (m, l, ex) recurrence over the thread's columns, then
    the merges (16 lanes by butterfly + 4 waves for 'mfma'; 64 lanes + 4 waves for 'valu'). z [R,G] float32 logits;
    weights: list of [R,G] float32 arrays w_k, ex_k accumulates p * w_k (default: one, the logits themselves).
    -> lse [R], [ex_k / l] list of [R]. exp / log are numpy's float32 ones."""
    z = np.ascontiguousarray(z, dtype=F32)
    R, G = z.shape
    ws = [z] if weights is None else [np.ascontiguousarray(w, dtype=F32) for w in weights]
    T = 256 if layout == 'valu' else 64
    t = np.arange(T)
    m = np.full((R, T), -np.inf, dtype=F32)
    l = np.zeros((R, T), dtype=F32)
    ex = [np.zeros((R, T), dtype=F32) for _ in ws]
    steps = (G + T - 1) // T
    with np.errstate(invalid='ignore', over='ignore'):
        for n in range(steps):
            cols = t + T * n if layout == 'valu' else ((t // 16) + 4 * n) * 16 + (t % 16)
            ok = cols < G
            cc = np.minimum(cols, G - 1)
            zz = z[:, cc]
            mn = np.maximum(m, zz)
            al = np.where(np.isneginf(m), F32(0), np.exp(m - mn))
            p = np.exp(zz - mn)
            l = np.where(ok, l * al + p, l)
            ex = [np.where(ok, e * al + p * w[:, cc], e) for e, w in zip(ex, ws)]
            m = np.where(ok, mn, m)

        def merge(m1, l1, e1, m2, l2, e2):
            mn = np.maximum(m1, m2)
            s1 = np.where(np.isneginf(m1), F32(0), np.exp(m1 - mn))
            s2 = np.where(np.isneginf(m2), F32(0), np.exp(m2 - mn))
            return mn, l1 * s1 + l2 * s2, [a * s1 + b * s2 for a, b in zip(e1, e2)]
        if layout == 'mfma':
            for o in (1, 2, 4, 8):
                m, l, ex = merge(m, l, ex, m[:, t ^ o], l[:, t ^ o], [e[:, t ^ o] for e in ex])
            m, l, ex = m[:, ::16], l[:, ::16], [e[:, ::16] for e in ex]          # [R,4]
        else:
            m4 = m.reshape(R, 4, 64)
            M = m4.max(-1)
            sc = np.where(np.isneginf(m4), F32(0), np.exp(m4 - M[..., None]))
            l = (l.reshape(R, 4, 64) * sc).sum(-1, dtype=F32)
            ex = [(e.reshape(R, 4, 64) * sc).sum(-1, dtype=F32) for e in ex]
            m = M
        MM = m.max(-1)
        ll = np.zeros(R, dtype=F32)
        ee = [np.zeros(R, dtype=F32) for _ in ex]
        for w in range(4):
            s2 = np.where(np.isneginf(m[:, w]), F32(0), np.exp(m[:, w] - MM))
            ll = ll + l[:, w] * s2
            ee = [a + e[:, w] * s2 for a, e in zip(ee, ex)]
        return MM + np.log(ll), [e / ll for e in ee]


def row_scale(z):
    """the magnitude the forward statistics of a row are measured against: max(1, max_j |logit_j|)"""
    return np.maximum(1.0, np.abs(z).max(-1))


# Measured by tests/test_clip_loss_reference_cpu.py over CLIP_SPECS + SSL_SPECS below (G <= 1025; it asserts measured <=
# recorded): worst |float32 restatement - float64| of lse / expectations over row_scale. The per-lane sums are sequential,
# so the error grows with G: the number is not valid for larger batches.
FWD_F32_ERR = 3.6e-7            # measured 3.33e-7
FWD_F32_ERR_CEILING = 1e-6      # 16 ulp of float32: what `recorded` may never exceed, whatever a host's exp / log measure
MARGIN = 8.0                    # __expf / __logf are the fast variants: their argument reduction adds error growing with |x|
MEASURED_G_MAX = 1025


def fwd_tol(G):
    """allowed |kernel - float64| of lse / expectations, per unit of row_scale"""
    assert G <= MEASURED_G_MAX
    return MARGIN * FWD_F32_ERR


# Measured by tests/test_clip_loss_reference_cpu.py per class of backward cases (it asserts measured <= recorded <=
# ceiling): worst |backward_f32 - float64| over the UN-CANCELLED magnitude |k| sum_j s (p + p' + 2 delta) |b| (not over
# sum |c| |b|: the kernel forms c_ii = (p + p') - 2 in float32, an absolute error of a few ulp of 2 however small |c_ii|
# is, and with sparse rows a gradient column can take its whole magnitude from the diagonal term alone). The gradient
# column is one sequential float32 sum over j = 0 .. G-1, so every number belongs to the G of its class.
BWD_F32_ERR = {
    'clip': 1.6e-6,             # measured 1.41e-6   BWD_SPECS clip + single-rank + one-indicator-value cases, G <= 1025
    'rows_only': 3.0e-6,        # measured 2.67e-6   the same cases under rows_only (the magnitude lacks p' and one delta)
    'ssl': 1.3e-6,              # measured 1.16e-6   BWD_SPECS ssl + the single-rank SSL case, G <= 1025
    'large': 1.8e-5,            # measured 1.63e-5   LARGE_SPECS, clip and ssl, 16376 <= G <= 38392
    'random14': 1.6e-6,         # measured 1.40e-6   RANDOM_BWD_SHAPES at scale 14.285714: clip, rows_only, ssl; f32, bf16
    'random100': 1.4e-5,        # measured 1.19e-5   the same at scale 100 (a logit near 100 carries ulp(100) = 7.6e-6)
    'paired100': 3.4e-5,        # measured 3.10e-5   the same at scale 100 with the diagonal holding the mass of a row
}
BWD_CLASS_G = {'clip': 1025, 'rows_only': 1025, 'ssl': 1025, 'large': 38392, 'random14': 1025, 'random100': 1025,
               'paired100': 1025}
BWD_CLASS_LOGIT = {'random14': (768, 14.285714), 'random100': (768, 100.0), 'paired100': (768, 100.0)}     # (E, scale) of the inexact logits
_EPS32 = float(np.finfo(np.float32).eps)


def bwd_ceiling(cls):
    """What a recorded backward number may never exceed, whatever a host's float32 exp measures. A sequential float32
    sum of G terms is off by at most (G - 1) eps / 2 of the sum of the terms' absolute values -- which IS the un-cancelled
    magnitude -- and the terms' own roundings (exp, the diagonal subtraction, the products with s and b) add a few eps / 2
    each: eps * G is twice the first bound and covers the second from G = 8 on. The random classes have logits that are
    not exact: a float32 dot product of E terms of unit rows is off by at most E eps / 2 * scale, and exp turns an
    absolute error of its argument into a relative one of p, hence the second summand there."""
    E, scale = BWD_CLASS_LOGIT.get(cls, (0, 0.0))
    return _EPS32 * (BWD_CLASS_G[cls] + 0.5 * E * scale)


def bwd_tol(cls, G):
    """allowed |kernel - float64| of a gradient element, per unit of its un-cancelled magnitude: the recurrence is the
    float32 restatement's, with __expf and fmaf in place of exp and multiply-add"""
    assert G <= BWD_CLASS_G[cls]
    return MARGIN * BWD_F32_ERR[cls]


# ----------------------------------------------------------------------------------------------------------------------
# the cases (shared by the CPU and the GPU file)
# ----------------------------------------------------------------------------------------------------------------------
# (B, G, E, row0): matrix-core forward, 2 to 4 shapes per width. (19, 37, 13) is there for the waves without tiles at
# 16 < G < 64: that needs at most 3 tiles, G <= 48 (at G = 50 each of the four waves still owns one)
MFMA_SHAPES = ((1, 1, 64, 0), (17, 83, 64, 66), (40, 129, 64, 3),
               (16, 16, 128, 0), (33, 50, 128, 17), (5, 300, 128, 295), (19, 37, 128, 13),
               (17, 83, 256, 66), (33, 50, 256, 17), (40, 129, 256, 3), (5, 300, 256, 295),
               (1, 1, 512, 0), (33, 50, 512, 17), (40, 129, 512, 3))
# VALU forward (and every SSL launch): B odd, row0 + B == G in several
VALU_SHAPES = ((1, 1, 8, 0), (5, 300, 8, 295), (7, 1025, 8, 500),
               (3, 63, 24, 11), (7, 257, 24, 250),
               (5, 257, 264, 100), (3, 1025, 264, 1022),
               (3, 63, 768, 60), (5, 300, 768, 7))
# the four shapes of test_clip_loss_slabs / test_ssl_clip_loss_slabs (random data there)
OLD_SHAPES = ((4, 4, 64, 0), (3, 12, 32, 6), (32, 256, 256, 64), (5, 300, 8, 295))


CLIP_SPECS = tuple(('clip',) + s + (n,) for n, s in enumerate(MFMA_SHAPES + VALU_SHAPES))
SSL_SPECS = tuple(('ssl',) + s + (n,) for n, s in enumerate(VALU_SHAPES))


@functools.lru_cache(maxsize=None)
def exact_case(kind, B, G, E, row0, n=0):
    """kind 'clip' | 'ssl'. The exact-logit inputs of one shape: scale 16 or 64 alternating with n, ties planned for the
    kernel that serves the shape. Cached: the arrays are shared and must not be written to."""
    mfma = kind == 'clip' and uses_mfma(E)
    rel_of = mfma_relation if mfma else valu_relation
    rels = MFMA_RELATIONS if mfma else VALU_RELATIONS
    limit = 2 if (kind == 'ssl' and E < 16) else 6
    ties = plan_ties(B, G, row0, rel_of, rels, first=n, limit=limit)
    scale = (16.0, 64.0)[n % 2]
    ssl = kind == 'ssl'
    nnz = 2 if E < 16 else 3
    d = exact_inputs(B, G, E, row0, scale, k=2 if (ssl or scale == 64.0) else 1, nnz=nnz, seed=1000 * G + E + n, ties=ties,
                     ssl=ssl)
    d.update(B=B, G=G, E=E, row0=row0, kind=kind, layout='mfma' if mfma else 'valu')
    return d


def tie_coverage(cases):
    """{(relation, position)} over the planted ties of a list of cases"""
    return {(r, p) for c in cases for _, _, r, p in c['ties']}


@functools.lru_cache(maxsize=None)
def random_case(kind, B, G, E, row0, scale=14.285714, corr=0.5):
    """Unit-norm random rows, each text loosely correlated with its image (the data of the older slab tests; `corr` is
    the weight of the unit image row added to a text row of norm ~ sqrt(E): cosine ~ corr / sqrt(E + corr^2)). SSL:
    indicators ~ Bernoulli(1/2), scales {12.5, sqrt(12.5 * scale), scale}."""
    rng = np.random.default_rng(7 * G + E + row0)
    img = rng.standard_normal((G, E))
    img /= np.linalg.norm(img, axis=1, keepdims=True)
    txt = rng.standard_normal((G, E)) + corr * img
    txt /= np.linalg.norm(txt, axis=1, keepdims=True)
    ind = (rng.random(G) < 0.5).astype(np.int32)
    d = dict(img=img.astype(np.float32), txt=txt.astype(np.float32), ind=ind, B=B, G=G, E=E, row0=row0, kind=kind)
    if kind == 'ssl':
        d['scales3'] = np.float32([12.5, np.sqrt(np.float32(12.5) * np.float32(scale)), scale])
    else:
        d['scale'] = np.float32([scale])
    return d


def case_forward(c):
    """float64 forward of a case -> dict(logits, lse, diag, expect [2,B] or bucket expectations [2,B,3], max, argmax,
    dots, stats = the kernel's layout)"""
    if c['kind'] == 'ssl':
        z, st, am, d = ssl_slab_forward(c['img'], c['txt'], c['ind'], c['scales3'], c['B'], c['row0'])
        return dict(logits=z, stats=st, argmax=am, dots=d, lse=st[..., 0], diag=st[..., 1], expect=st[..., 2:5],
                    diag_dot=st[..., 5], max=st[..., 6])
    z, st, am = slab_forward(c['img'], c['txt'], c['scale'], c['B'], c['row0'])
    return dict(logits=z, stats=stats4(st), argmax=am, **st)


def forward_f32_error(c):
    """worst distance of the float32 streaming restatement from float64 over a case: lse and expectation(s), each over
    the row's scale (max(1, max |logit|) -- for the SSL bucket expectations max(1, max |dot|))"""
    f = case_forward(c)
    worst = 0.0
    ssl = c['kind'] == 'ssl'
    for d in range(2):
        z = f['logits'][d]
        z32 = z.astype(F32)                                      # exact by construction
        rs = row_scale(z)
        if ssl:
            bucket = c['ind'][c['row0']:c['row0'] + c['B'], None] + c['ind'][None, :]
            zr = f['dots'][d].astype(F32)
            lse, ex = stream_f32(z32, c['layout'], [np.where(bucket == k, zr, F32(0)) for k in range(3)])
            ds = np.maximum(1.0, np.abs(f['dots'][d]).max(-1))
            for k in range(3):
                worst = max(worst, (np.abs(ex[k].astype(np.float64) - f['expect'][d][:, k]) / ds).max())
        else:
            lse, ex = stream_f32(z32, c['layout'])
            worst = max(worst, (np.abs(ex[0].astype(np.float64) - f['expect'][d]) / rs).max())
        worst = max(worst, (np.abs(lse.astype(np.float64) - f['lse'][d]) / rs).max())
    return float(worst)


# ----------------------------------------------------------------------------------------------------------------------
# the backward: cases, float64 reference of a case, float32 restatement
# ----------------------------------------------------------------------------------------------------------------------
def bwd_branches(B, G, E, row0):
    """what a shape makes clip_bwd_kernel / ssl_bwd_kernel do: thread t writes the gradient columns t, t + 256, ..."""
    return {'e_second_pass': E > 256, 'idle_column_threads': E < 256, 'stride': G > 256, 'ends_at_G': row0 + B == G,
            'lds_opt_in': (E + G) * 4 > 64 * 1024, 'lds_limit': (E + G) * 4 == LDS_LIMIT_BYTES}


# the clip backward is ONE VALU kernel for every E: all 23 shapes; the SSL backward takes the VALU list
BWD_SPECS = CLIP_SPECS + SSL_SPECS
# coefficient rows around the 64 KiB opt-in and at the 150 KiB limit, E = 8: (E + G) * 4 = 65536 (no opt-in), 65540 (the
# first opt-in), 153600 (the last accepted row). 2 or 3 rows x 2 directions = 4 to 6 workgroups
LARGE_SHAPES = ((3, 16376, 8, 0), (2, 16377, 8, 16375), (3, 38392, 8, 38389))
LARGE_SPECS = tuple((kind,) + s + (n,) for kind in ('clip', 'ssl') for n, s in enumerate(LARGE_SHAPES))
RANDOM_BWD_SHAPES = ((32, 256, 256, 64), (5, 300, 768, 7), (7, 1025, 24, 500))
RANDOM_SCALES = {'random14': 14.285714, 'random100': 100.0, 'paired100': 100.0}
UPSTREAM = np.float32([0.7])
# single rank (B = G, row0 = 0), one shape per forward kernel: matrix-core, VALU, SSL
SINGLE_RANK_SPECS = (('clip', 40, 40, 64, 0, 0), ('clip', 33, 33, 24, 0, 1), ('ssl', 33, 33, 24, 0, 2))


def one_value_case(c, value):
    """the clip case an SSL case turns into when every indicator is `value`: scale = scales3[2 * value]"""
    assert c['kind'] == 'ssl' and value in (0, 1)
    d = dict(c, kind='clip', scale=np.float32([c['scales3'][2 * value]]))
    del d['scales3']
    return d


def one_value_pair(B, G, E, row0, value):
    """(SSL case whose indicators all are `value`, the clip case at scales3[2 * value]) on the embeddings of the exact clip
    case built for scale 64 (entries +-1/4, at most 4 non-zeros: |logit| <= 16 at either scale, so z - L > -80 and no
    exp of the backward is subnormal; the SSL cases' doubled partner rows reach z - L = -112)"""
    base = exact_case('clip', B, G, E, row0, 1)
    assert float(base['scale'][0]) == 64.0 and value in (0, 1)
    s3 = np.float32([16.0, 32.0, 64.0])
    ssl = dict(base, kind='ssl', ind=np.full(G, value, dtype=np.int32), scales3=s3)
    del ssl['scale']
    return ssl, dict(base, scale=np.float32([s3[2 * value]]))


def round_bf16(x):
    """float32 array rounded to the nearest bfloat16 value (ties to even), as float32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def random_bwd_case(kind, B, G, E, row0, cls, bf16):
    """random_case at the scale of class `cls`, its embeddings rounded to the dtype the kernel is handed them in.
    'paired100': each text at cosine ~ 0.7 to its image instead of random_case's ~ 0.5 / sqrt(E) -- at scale 100 the
    diagonal then holds more than 0.99 of the softmax mass of some local row, so c_ii = (p + p') - 2 cancels. The loose
    pairs of 'random100' never get there: their rows peak too (mass up to 0.9996 on one column), but off the diagonal --
    the largest diagonal mass over these shapes is 0.979."""
    c = dict(random_case(kind, B, G, E, row0, RANDOM_SCALES[cls], float(np.sqrt(E)) if cls == 'paired100' else 0.5))
    if bf16:
        c['img'], c['txt'] = round_bf16(c['img']), round_bf16(c['txt'])
    return c


def case_lse32(c):
    """the float64 LSEs of a case (grouped lse_all) rounded to float32: the array the kernel AND the reference read"""
    ssl = c['kind'] == 'ssl'
    return lse_all(c['img'], c['txt'], None if ssl else c['scale'], c['ind'] if ssl else None,
                   c['scales3'] if ssl else None).astype(F32)


def case_backward(c, lse32, coef, upstream=UPSTREAM, rows_only=False):
    """float64 backward of a case from the given float32 LSEs -> grads [2,B,E], un-cancelled magnitudes [2,B,E]"""
    if c['kind'] == 'ssl':
        assert not rows_only
        o = ssl_slab_backward(c['img'], c['txt'], c['ind'], lse32, c['scales3'], upstream, coef, c['B'], c['row0'], True)
    else:
        o = slab_backward(c['img'], c['txt'], lse32, c['scale'], upstream, coef, c['B'], c['row0'], rows_only, True)
    return np.stack(o[0:2]), np.stack(o[4:6])


def backward_f32(c, lse32, coef, upstream=UPSTREAM, rows_only=False):
    """The backward kernels' arithmetic in float32: z as a sequential float32 dot product (clip: of the scaled row; SSL:
    times the pair scale), exp(z - L_own) (+ exp(z - L_other[j]) unless rows_only), the diagonal subtraction, for SSL the
    multiplication by the pair scale, a sequential accumulation over j = 0 .. G-1 per gradient column, the final factor
    k = coef * scale * upstream (SSL: coef * upstream). -> grads [2,B,E] float32. exp is numpy's float32 one."""
    B, G, E, row0 = c['B'], c['G'], c['E'], c['row0']
    ssl = c['kind'] == 'ssl'
    lse = np.ascontiguousarray(lse32, dtype=F32).reshape(2, G)
    up = F32(1) if upstream is None else F32(np.asarray(upstream).reshape(-1)[0])
    img, txt = np.ascontiguousarray(c['img'], dtype=F32), np.ascontiguousarray(c['txt'], dtype=F32)
    idx, rows = np.arange(row0, row0 + B), np.arange(B)
    out = []
    for d, (own, other) in enumerate(((img[idx], txt), (txt[idx], img))):
        if ssl:
            s3 = np.ascontiguousarray(c['scales3'], dtype=F32)
            ind = (np.asarray(c['ind']) != 0).astype(np.int64)
            s = s3[ind[idx][:, None] + ind[None, :]]
            k = F32(coef) * up
        else:
            own = F32(c['scale'][0]) * own
            k = F32(coef) * F32(c['scale'][0]) * up
        z = np.zeros((B, G), dtype=F32)
        for e in range(E):
            z = z + own[:, e, None] * other[None, :, e]
        if ssl:
            z = z * s
        with np.errstate(invalid='ignore'):
            cc = np.exp(z - lse[d, idx][:, None])
            if not rows_only:
                cc = cc + np.exp(z - lse[1 - d][None, :])
        cc[rows, idx] -= F32(1 if rows_only else 2)
        if ssl:
            cc = s * cc
        acc = np.zeros((B, E), dtype=F32)
        for j in range(G):
            acc = acc + cc[:, j, None] * other[j][None, :]
        assert acc.dtype == F32 and z.dtype == F32 and cc.dtype == F32
        out.append(k * acc)
    return np.stack(out)


def bwd_coef(c, rows_only=False):
    return 1.0 / (2 * c['B']) if rows_only else 3.0 / (2 * c['G'])


def backward_f32_error(c, rows_only=False):
    """worst |backward_f32 - float64| / un-cancelled magnitude over a case; an element of magnitude 0 must be exactly 0"""
    lse32 = case_lse32(c)
    coef = bwd_coef(c, rows_only)
    ref, umag = case_backward(c, lse32, coef, UPSTREAM, rows_only)
    got = backward_f32(c, lse32, coef, UPSTREAM, rows_only).astype(np.float64)
    assert (got[umag == 0] == 0).all() and (ref[umag == 0] == 0).all()
    err = np.abs(got - ref)
    return float((err[umag > 0] / umag[umag > 0]).max()) if (umag > 0).any() else 0.0


# ----------------------------------------------------------------------------------------------------------------------
# lo-bearing exact inputs for the matrix-core forward
# ----------------------------------------------------------------------------------------------------------------------
LO_FACTOR = np.float32(1 + 2.0 ** -9)             # 513 * 2^-9: needs 10 significand bits, bfloat16 has 8


def bf16_lo(x):
    """x - bf16(x) in float32: the lo fragment of the matrix-core kernel's operand split"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return x - round_bf16(x)


@functools.lru_cache(maxsize=None)
def lo_case(which, B, G, E, row0, n=0):
    """The exact clip case of a matrix-core shape with every entry of ONE matrix (`which` = 'img' | 'txt') multiplied by
    1 + 2^-9 in float32. Asserted here, from the inputs: every non-zero entry of that matrix has a non-zero bfloat16 lo
    part (the zeros contribute no product at all); the other matrix is bfloat16-exact, so no lo x lo product exists; every
    product a_hi b_hi, a_lo b_hi, a_hi b_lo -- and so every partial sum in any order -- is an integer multiple of
    u 2^-9 (u the unit of the base case) below 2^24 u 2^-9, hence exact in float32. The tie sets are those of the base
    case: every logit of a direction is the base logit times 513 / 512. Direction 0 (A = img, B = txt) then needs
    a.lo x b.hi for 'img' and a.hi x b.lo for 'txt'; direction 1 the other one."""
    base = exact_case('clip', B, G, E, row0, n)
    assert base['layout'] == 'mfma' and which in ('img', 'txt')
    c = dict(base)
    c[which] = (base[which] * LO_FACTOR).astype(np.float32)
    other = 'txt' if which == 'img' else 'img'
    scale = float(base['scale'][0])
    assert np.array_equal(c[which].astype(np.float64), base[which].astype(np.float64) * (1 + 2.0 ** -9))     # exact scaling
    nz = base[which] != 0
    assert nz.any() and (bf16_lo(c[which])[nz] != 0).all() and (bf16_lo(np.float32(scale) * c[which])[nz] != 0).all()
    assert _is_bf16(c[other]) and _is_bf16(np.float32(scale) * c[other])
    assert _is_bf16(round_bf16(c[which])) and _is_bf16(bf16_lo(c[which]))        # hi + lo IS the value: two fragments
    mag = np.abs(base['img'][base['img'] != 0]).min()
    assert mag == np.abs(base['txt'][base['txt'] != 0]).min()
    unit = float(mag) ** 2 * scale * 2.0 ** -9
    for m in (c['img'], c['txt'], round_bf16(c[which]), bf16_lo(c[which])):
        q = m.astype(np.float64) / (float(mag) * 2.0 ** -9)
        assert np.array_equal(np.round(q), q)                 # every fragment is a multiple of mag 2^-9 ...
    q = c[other].astype(np.float64) / float(mag)
    assert np.array_equal(np.round(q), q)                     # ... and the other matrix of mag: products of u 2^-9
    a, b = np.abs(c['img']).astype(np.float64), np.abs(c['txt']).astype(np.float64)
    top = scale * max(a.sum(1).max() * b.max(), b.sum(1).max() * a.max())
    assert top / unit < 2 ** 24, (top, unit)
    c['lo'] = which
    return c


def diag_mass(c):
    """softmax mass of each local row on its own diagonal column, [2,B], from the true float64 LSEs"""
    ssl = c['kind'] == 'ssl'
    lse = lse_all(c['img'], c['txt'], None if ssl else c['scale'], c['ind'] if ssl else None, c['scales3'] if ssl else None)
    f = case_forward(c)
    idx = np.arange(c['row0'], c['row0'] + c['B'])
    return np.exp(f['diag'] - lse[:, idx])
