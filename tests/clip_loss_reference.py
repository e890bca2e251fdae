"""Float64 restatement of the contrastive-head kernels (lavila_amd/csrc/clip_loss.hip, clip_loss_mfma.hip), slab-wise:
nothing here ever forms the G x G logit matrix. CPU only, numpy float64.

  slab_forward / ssl_slab_forward      logits [2,B,G], the statistics the kernels emit, argmax under "first maximum"
  slab_backward / ssl_slab_backward    the gradient of the local rows from the SAME lse_all array the kernel is handed
                                       (it is an input of the kernel), and the per-element magnitude sum
                                       |k| sum_j |c_ij| |b_je| that the tests use as the error scale
  lse_all                              all 2 G row / column log-sum-exps in float64 by column chunks
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
    """shared body: c_ij from the logits and the given LSEs, grad = k sum_j c_ij b_j, mag = |k| sum_j |c_ij| |b_j|.
    pair_scale(i_global [B,1], j [1,G]) -> the per-pair temperature [B,G]."""
    lse = _f64(lse_all).reshape(2, -1)
    G = lse.shape[1]
    idx, rows = np.arange(row0, row0 + B), np.arange(B)
    s = pair_scale(idx[:, None], np.arange(G)[None, :])
    grads, mags = [], []
    for d, (own, other) in enumerate(_sides(img_all, txt_all, B, row0)):
        z = s * (own @ other.T)
        own_l = lse[d, idx][:, None]
        if rows_only:                                   # the partner LSEs are not read (they may be NaN)
            c = np.exp(z - own_l)
            c[rows, idx] -= 1.0
        else:
            c = np.exp(z - own_l) + np.exp(z - lse[1 - d][None, :])
            c[rows, idx] -= 2.0
        c = c * s
        grads.append(k * (c @ other))
        mags.append(abs(k) * (np.abs(c) @ np.abs(other)))
    return grads[0], grads[1], mags[0], mags[1]


def slab_backward(img_all, txt_all, lse_all, scale, upstream, coef, B, row0, rows_only=False):
    """lvl_clip_loss_bwd in float64 -> dimg [B,E], dtxt [B,E], mag_img, mag_txt. With k = coef * upstream,
    d/d(own row) = k * scale * sum_j c_ij b_j; the per-pair temperature is the one scale."""
    scale = float(np.asarray(_f64(scale)).reshape(-1)[0])
    up = 1.0 if upstream is None else float(np.asarray(_f64(upstream)).reshape(-1)[0])
    return _backward(img_all, txt_all, lse_all, B, row0, coef * up, rows_only,
                     lambda i, j: np.full(np.broadcast(i, j).shape, scale))


def ssl_slab_backward(img_all, txt_all, ind_all, lse_all, scales3, upstream, coef, B, row0):
    ind = np.asarray(_f64(ind_all)).astype(np.int64)
    s3 = _f64(scales3).reshape(3)
    up = 1.0 if upstream is None else float(np.asarray(_f64(upstream)).reshape(-1)[0])
    return _backward(img_all, txt_all, lse_all, B, row0, coef * up, False, lambda i, j: s3[ind[i] + ind[j]])


def lse_all(img_all, txt_all, scale=None, ind_all=None, scales3=None, chunk=512):
    """All 2 G true LSEs in float64, [2,G]: row 0 = rows of logits_per_image, row 1 = rows of logits_per_text, visiting
    the columns `chunk` at a time (at most G x chunk logits exist at once)."""
    img, txt = _f64(img_all), _f64(txt_all)
    G = img.shape[0]
    ind = np.zeros(G, dtype=np.int64) if ind_all is None else np.asarray(_f64(ind_all)).astype(np.int64)
    if scales3 is None:
        s = float(np.asarray(_f64(scale)).reshape(-1)[0])
        s3 = np.array([s, s, s])
    else:
        s3 = _f64(scales3).reshape(3)
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
def random_case(kind, B, G, E, row0, scale=14.285714):
    """Unit-norm random rows, each text loosely correlated with its image (the data of the older slab tests). SSL:
    indicators ~ Bernoulli(1/2), scales {12.5, sqrt(12.5 * scale), scale}."""
    rng = np.random.default_rng(7 * G + E + row0)
    img = rng.standard_normal((G, E))
    img /= np.linalg.norm(img, axis=1, keepdims=True)
    txt = rng.standard_normal((G, E)) + 0.5 * img
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
