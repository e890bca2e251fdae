"""Float64 restatement of the contract of lvl_sample_next_token (the header comment of csrc/sampler.hip), shared by
tests/test_sampler_reference_cpu.py (which holds `kept` to transformers' own warpers) and tests/test_gpu_sampler_exact.py
(which holds the kernel to it). Nothing here comes from lavila_amd, and nothing reads the kernel's debug output.

One row x [V] (float64 copies of bf16 logits), top_k (0 / None: off), top_p (None / 1.0: off), temperature T:
  top-k   keep x >= (k-th largest x): entries tied with the k-th value stay. top_k == 1 is greedy decoding: the FIRST
          maximum alone (torch.argmax), whatever top_p says.
  top-p   on what is left, with weights w = exp((x - max) / T), Z = sum w, thr = (1 - top_p) Z: walk the distinct values
          in ascending order accumulating their mass; the boundary value v is the first whose cumulative mass exceeds thr.
          Everything below v goes; of the cnt entries equal to v the first r = clamp(floor((thr - below) / p_v), 0, cnt)
          in index order go; the largest entry always stays (r = cnt - 1 when v is the maximum and r >= cnt).
  Values are compared with == on the float64 values: +0 and -0 are one level (transformers' `scores < kth` and sort).
  draw    the kept entries in index order, inverse CDF: the token is the first index whose inclusive cumulative weight
          exceeds u * (kept weight).
  nll     entropy of softmax(x) (0 log 0 = 0), or the cross entropy against a target (0 and not counted when the target
          is the pad id or outside [0, V)).

The generators build LEVEL-STRUCTURED rows: a multiset of a few bf16-representable values with chosen multiplicities,
permuted differently per row, so that ties are everywhere, sit in different thread chunks per row, and ONE top_p --
solved so that x = (thr - below) / p_v sits at r + 0.5 for a chosen r -- fits every row of a case.
"""
import math

import numpy as np

ST = 1024                                   # threads per row of the kernel: thread t draws from indices [t*chunk, (t+1)*chunk)
SUM_REL_ERR = 1e-5                          # generous bound on the relative error of an f32 block sum of <= 53248 __expf terms
HALF_WIDTH = 1e-4                           # least half-width (relative to the kept weight) of an interval a test aims at
MAX_VOCAB = 52 * ST                         # what lvl_sample_max_vocab() must report


def bf16(m, e=1, sign=1.0):
    """The bf16 value sign * 2^e * (1 + m/128), m in 0..127 (7 mantissa bits): exactly representable by construction."""
    assert 0 <= m < 128
    return sign * 2.0 ** e * (1.0 + m / 128.0)


def chunk_of(V):
    return (V + ST - 1) // ST


# ----------------------------------------------------------------------------------------------------------------------
# the oracle
# ----------------------------------------------------------------------------------------------------------------------
def weights(x, T):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(under='ignore'):
        return np.exp((x - x.max()) / float(T))


def nucleus(x, keep, top_p, T):
    """(v, r, cnt, xq, thr, p_v): the boundary value, the ties dropped, the ties there are, the unrounded quotient
    (thr - below) / p_v, for the entries `keep` of row x."""
    w = np.where(keep, weights(x, T), 0.0)
    Z = w.sum()
    thr = (1.0 - float(top_p)) * Z
    levels = np.unique(x[keep])                                   # ascending; -0.0 == 0.0: one level
    below = 0.0
    for v in levels:
        tie = keep & (x == v)
        cnt = int(tie.sum())
        p = float(w[tie][0])
        if below + cnt * p > thr or v == levels[-1]:
            xq = (thr - below) / p
            r = int(min(max(math.floor(xq), 0), cnt))
            if v == levels[-1] and r >= cnt:
                r = cnt - 1
            return float(v), r, cnt, xq, thr, p
        below += cnt * p
    raise AssertionError('unreachable: the maximum level ends the walk')


def kept(logits64, top_k, top_p, temperature):
    x = np.asarray(logits64, dtype=np.float64)
    V = x.size
    T = 1.0 if temperature is None else float(temperature)
    keep = np.ones(V, dtype=bool)
    k = min(int(top_k), V) if top_k else 0
    if k == 1:
        keep[:] = False
        keep[int(np.argmax(x))] = True                             # np.argmax: the first maximum
        return keep
    if k:
        kth = np.sort(x)[V - k]
        keep = x >= kth
    if top_p is not None and float(top_p) < 1.0:
        v, r, _, _, _, _ = nucleus(x, keep, top_p, T)
        keep &= x >= v
        ties = np.nonzero(keep & (x == v))[0]
        keep[ties[:r]] = False
    return keep


def draw_interval(mask, logits64, T):
    """Inclusive float64 CDF (unnormalised) over the kept entries in index order; cum[-1] is the kept weight."""
    w = np.where(mask, weights(logits64, 1.0 if T is None else T), 0.0)
    return np.cumsum(w)


def u_for(token, cum):
    """(u, half): the midpoint of `token`'s interval over the total, and the interval's half-width over the total."""
    lo = cum[token - 1] if token > 0 else 0.0
    return (lo + cum[token]) / (2.0 * cum[-1]), (cum[token] - lo) / (2.0 * cum[-1])


def token_at(cum, u):
    """(token, slack): the token the inverse CDF gives at u, and the distance of u from the nearer end of that token's
    interval, relative to the total."""
    want = u * cum[-1]
    t = int(np.searchsorted(cum, want, side='right'))
    t = min(t, len(cum) - 1)
    lo = cum[t - 1] if t > 0 else 0.0
    return t, min(want - lo, cum[t] - want) / cum[-1]


def entropy(logits64):
    x = np.asarray(logits64, dtype=np.float64)
    w = weights(x, 1.0)
    p = w / w.sum()
    nz = p > 0
    return float(-(p[nz] * np.log(p[nz])).sum())


def xent(logits64, target, pad):
    """(nll, counted)."""
    x = np.asarray(logits64, dtype=np.float64)
    t = int(target)
    if t == pad or t < 0 or t >= x.size:
        return 0.0, 0.0
    m = x.max()
    return float(m + math.log(np.exp(x - m).sum()) - x[t]), 1.0


def chi2_quantile_upper(q, dof):
    """x with P(chi2_dof > x) = q (bisection on the regularised upper incomplete gamma function, float64)."""
    import torch
    a = torch.tensor(dof / 2.0, dtype=torch.float64)
    lo, hi = 0.0, dof + 100.0 * math.sqrt(2.0 * dof) + 100.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if torch.special.gammaincc(a, torch.tensor(mid / 2.0, dtype=torch.float64)).item() > q:
            lo = mid
        else:
            hi = mid
    return hi


# ----------------------------------------------------------------------------------------------------------------------
# level-structured cases
# ----------------------------------------------------------------------------------------------------------------------
class Case:
    """levels: distinct values, DESCENDING; counts: their multiplicities (one may be None: whatever is left of V).
    nucleus: None (top_p off), ('p', top_p) for a given top_p, or ('solve', level index, r): top_p solved so that level
    `index` is the boundary and (thr - below) / p_v = r + 0.5 (r < 0 counts from cnt: -1 is cnt - 1)."""

    def __init__(self, name, V, levels, counts, top_k=0, nucleus=None, T=1.0, rows=12, extra_stride=0, seed=0,
                 clamp=False):
        counts = list(counts)
        if None in counts:
            counts[counts.index(None)] = V - sum(c for c in counts if c is not None)
        assert sum(counts) == V and all(c > 0 for c in counts), (name, counts)
        assert all(a > b for a, b in zip(levels, levels[1:])), name
        import torch
        lv = torch.tensor(levels, dtype=torch.float64)
        assert torch.equal(lv.bfloat16().double(), lv), (name, 'levels must be bf16 values')
        self.name, self.V, self.levels, self.counts = name, V, [float(v) for v in levels], counts
        self.top_k, self.T, self.rows, self.extra_stride, self.seed, self.clamp = top_k, T, rows, extra_stride, seed, clamp
        self.top_p = self._top_p(nucleus)
        self.check_margins()

    def __repr__(self):
        return self.name

    def sorted_row(self):
        return np.repeat(np.array(self.levels, dtype=np.float64), self.counts)

    def _top_p(self, nuc):
        if nuc is None:
            return None
        if nuc[0] == 'p':
            return float(np.float32(nuc[1]))
        _, li, r = nuc
        x = self.sorted_row()
        keep = kept(x, self.top_k, None, self.T)
        assert keep[x == self.levels[li]].all(), (self.name, 'the boundary level must survive top-k')
        w = np.where(keep, weights(x, self.T), 0.0)
        cnt = self.counts[li]
        r = cnt + r if r < 0 else r
        assert 0 <= r < cnt
        thr = w[x < self.levels[li]].sum() + (r + 0.5) * w[x == self.levels[li]][0]
        return float(np.float32(1.0 - thr / w.sum()))            # what the kernel is handed is a float32

    def check_margins(self):
        """Conditions on the INPUTS (never on a kernel's output) that make the kept set and every aimed draw immune to
        f32 summation error; returns what the nucleus walk finds (None when top_p is off)."""
        x = self.sorted_row()
        keep = kept(x, self.top_k, self.top_p, self.T)
        w = weights(x, self.T)
        tot = w[keep].sum()
        rel = w[keep] / tot
        # no kept weight where float32 (denormals flushed or not) and float64 could disagree on "is it zero"
        assert ((rel >= 1e-30) | (rel <= 1e-60)).all(), (self.name, 'ambiguous underflow')
        assert rel.max() >= 2 * HALF_WIDTH, (self.name, 'the maximum must be a target')
        if self.top_p is None or self.top_p >= 1.0 or min(self.top_k or 0, self.V) == 1:
            return None
        v, r, cnt, xq, thr, p = nucleus(x, kept(x, self.top_k, None, self.T), self.top_p, self.T)
        assert SUM_REL_ERR * thr / p <= 0.05, (self.name, 'summation error too close to the margin', thr / p)
        if self.clamp:      # top_p so small that xq = cnt - (tiny): floor gives cnt - 1, and so does the clamp beyond cnt
            assert v == x.max() and cnt - 0.05 <= xq < cnt and r == cnt - 1, (self.name, xq, cnt)
        else:
            assert abs(xq - round(xq)) >= 0.25, (self.name, 'quotient too close to an integer', xq)
        assert p / tot >= 2 * HALF_WIDTH, (self.name, 'boundary ties must be targets', p / tot)
        return dict(v=v, r=r, cnt=cnt, xq=xq)

    def pins(self):
        """Indices every row gets a chosen level at: both ends of thread chunks 0 and 1, and of the last one."""
        c = chunk_of(self.V)
        last = (self.V - 1) // c
        return sorted({p for p in (0, c - 1, c, 2 * c - 1, last * c, self.V - 1, self.V // 2) if 0 <= p < self.V})

    def rows64(self):
        """[rows, V] float64: the multiset permuted per row; pin q of row i holds level (i + q) % nlev where the
        multiplicities allow, so that ties of every level -- the boundary's too -- meet every chunk edge in some row."""
        rng = np.random.default_rng(1000 + self.seed)
        base = self.sorted_row()
        out = np.empty((self.rows, self.V))
        pins = self.pins()
        for i in range(self.rows):
            x = base[rng.permutation(self.V)]
            for q, p in enumerate(pins):
                lvl = self.levels[(i + q) % len(self.levels)]
                free = np.nonzero(x == lvl)[0]
                free = free[~np.isin(free, pins[:q + 1])]
                if x[p] != lvl and free.size:
                    j = int(free[0])
                    x[p], x[j] = x[j], x[p]
            assert np.array_equal(np.sort(x), np.sort(base))
            out[i] = x
        return out


def targets(x, keep, cum, v=None, limit=28):
    """Kept entries a draw is aimed at (each at least HALF_WIDTH wide): the first and the last, the first kept tie of the
    boundary value v (rank r) and the last, kept entries with a dropped tie for a neighbour, the first and last heavy entry
    of thread chunks 0, 1 and the last chunk, and a spread of the rest."""
    V = x.size
    w = np.diff(np.concatenate([[0.0], cum])) / cum[-1]
    heavy = np.nonzero(keep & (w >= 2 * HALF_WIDTH))[0]
    assert heavy.size
    must = [heavy[0], heavy[-1]]
    if v is not None:
        tie = np.nonzero(keep & (x == v))[0]
        gone = np.nonzero(~keep & (x == v))[0]
        if tie.size:
            must += [tie[0], tie[-1]]
        for g in gone:
            must += [n for n in (g - 1, g + 1) if 0 <= n < V and keep[n] and w[n] >= 2 * HALF_WIDTH][:2]
    c = chunk_of(V)
    for t in (0, 1, (V - 1) // c):
        inside = heavy[(heavy >= t * c) & (heavy < (t + 1) * c)]
        if inside.size:
            must += [inside[0], inside[-1]]
    must = list(dict.fromkeys(int(m) for m in must))[:limit]
    rest = [int(h) for h in heavy if int(h) not in must]
    step = max(1, len(rest) // max(1, limit - len(must)))
    return must + rest[::step][:max(0, limit - len(must))]


def probes(x, keep, cum, T, limit=8):
    """[(u, token)]: for a DROPPED entry j that borders a kept one, a uniform inside the interval j would occupy if it
    were wrongly kept (with the total grown by w_j), and the token the oracle's CDF gives there. Only entries heavy enough
    to be seen (the hypothetical interval and the oracle's slack at u are both at least HALF_WIDTH) are probed: the
    dropped ties of the boundary value and the level under it."""
    V = x.size
    w = weights(x, T)
    out = []
    near = np.zeros(V, dtype=bool)
    near[1:] |= keep[:-1]
    near[:-1] |= keep[1:]
    cand = np.nonzero(~keep & near & (w / cum[-1] >= 8 * HALF_WIDTH))[0]
    order = np.argsort(-w[cand], kind='stable')
    for j in cand[order]:
        lo = cum[j - 1] if j > 0 else 0.0
        best = None
        for f in (0.25, 0.5, 0.75):
            u = (lo + f * w[j]) / (cum[-1] + w[j])
            slack_wrong = min(f, 1 - f) * w[j] / (cum[-1] + w[j])
            t, slack = token_at(cum, u)
            if slack_wrong >= HALF_WIDTH and slack >= HALF_WIDTH and (best is None or slack > best[2]):
                best = (u, t, slack)
        if best is not None:
            out.append((best[0], best[1], int(j)))
        if len(out) == limit:
            break
    return out


def _cases():
    B = bf16
    c = []
    small = dict(V=331)
    # ---- top-k: where the k-th largest sits in the two-level radix count (key & 31 is the level-2 bucket) -----------------
    c += [Case('k_l2_last', levels=[3.0, B(31), 2.0, 1.0], counts=[3, 4, 6, None], top_k=5, **small),
          Case('k_l2_first_l1_end', levels=[3.0, B(32), B(31), 1.0], counts=[3, 4, 5, None], top_k=7, **small),
          Case('k_l2_mid', levels=[3.0, B(40), B(36), 1.0], counts=[2, 3, 4, None], top_k=4, **small),
          Case('k_l1_end_negative', levels=[B(1, 0, -1.0), B(32, 0, -1.0), B(33, 0, -1.0), -4.0], counts=[2, 3, 5, None],
               top_k=5, **small),
          Case('k_tied_level_over_k', levels=[3.0, 1.0], counts=[40, None], top_k=5, **small),
          Case('k_tied_level_over_k2', levels=[3.0, 2.5, 1.0], counts=[1, 30, None], top_k=2, **small)]
    for V in (13, 331):
        for k in (1, 2, V - 1, V, V + 5):
            c.append(Case(f'k{k}_V{V}', V=V, levels=[2.0, 1.5, 1.0, 0.5], counts=[2, 3, None, 1], top_k=k))
    c.append(Case('k_vm1_tied_min', V=13, levels=[2.0, 1.0, 0.5], counts=[2, None, 3], top_k=12))
    # ---- signs, one level, one ulp apart --------------------------------------------------------------------------------------
    neg = [B(0, 0, -1.0), B(1, 0, -1.0), -1.5, -3.0]
    mix = [0.5, B(0, -7), 0.0, B(0, -7, -1.0), -1.0]
    c += [Case('neg_k', levels=neg, counts=[3, 4, 6, None], top_k=5, **small),
          Case('neg_p', levels=neg, counts=[3, 4, 6, None], nucleus=('solve', 2, 1), **small),
          Case('neg_kp', levels=neg, counts=[3, 4, 6, None], top_k=9, nucleus=('solve', 2, 2), **small),
          Case('mix_k', levels=mix, counts=[3, 4, 6, 5, None], top_k=15, **small),
          Case('mix_p', levels=mix, counts=[3, 4, 6, 5, None], nucleus=('solve', 2, 3), **small),
          Case('mix_p_neg_boundary', levels=mix, counts=[3, 4, 6, 5, None], nucleus=('solve', 3, -1), **small),
          Case('equal', levels=[1.25], counts=[None], **small),
          Case('equal_k', levels=[1.25], counts=[None], top_k=3, **small),
          Case('equal_p_r0', levels=[-1.25], counts=[None], nucleus=('solve', 0, 0), **small),
          Case('equal_p_r1', levels=[1.25], counts=[None], nucleus=('solve', 0, 1), V=1024),
          Case('equal_p_rlast', levels=[1.25], counts=[None], nucleus=('solve', 0, -1), V=1025),
          Case('ulp_l1_edge_k', levels=[B(32), B(31), 1.0], counts=[4, 5, None], top_k=3, **small),
          Case('ulp_l1_edge_p', levels=[B(32), B(31), 1.0], counts=[4, 5, None], nucleus=('solve', 1, 2), **small),
          Case('ulp_exponent_edge_kp', levels=[1.0, B(127, -1), 0.5], counts=[4, 5, None], top_k=6,
               nucleus=('solve', 1, 0), **small)]
    # ---- nucleus: r, the maximum as the boundary, top_p off, both warpers -------------------------------------------------------
    lv, ct = [3.0, 2.5, 2.0, 1.0, -2.0], [2, 5, 8, 16, None]
    c += [Case('p_r0', levels=lv, counts=ct, nucleus=('solve', 2, 0), **small),
          Case('p_r1', levels=lv, counts=ct, nucleus=('solve', 2, 1), **small),
          Case('p_rlast', levels=lv, counts=ct, nucleus=('solve', 2, -1), **small),
          Case('p_bulk_boundary', levels=lv, counts=ct, nucleus=('solve', 4, 150), **small),
          Case('p_max_rlast', levels=lv, counts=[6, 5, 8, 16, None], nucleus=('solve', 0, -1), **small),
          Case('p_max_all_survive', levels=lv, counts=[6, 5, 8, 16, None], nucleus=('solve', 0, 0), **small),
          Case('p_tiny_clamped', levels=lv, counts=[6, 5, 8, 16, None], nucleus=('p', 1e-9), clamp=True, **small),
          Case('p_one', levels=lv, counts=ct, nucleus=('p', 1.0), **small),
          Case('p_none', levels=lv, counts=ct, **small),
          Case('kp_straddle', levels=lv, counts=ct, top_k=10, nucleus=('solve', 2, 3), **small),
          Case('kp_straddle_r0', levels=lv, counts=ct, top_k=15, nucleus=('solve', 2, 0), **small),
          Case('kp_k_inside_p', levels=lv, counts=ct, top_k=20, nucleus=('solve', 1, 2), **small),
          Case('k1_with_p', levels=lv, counts=ct, top_k=1, nucleus=('p', 0.5), **small)]
    # ---- temperature -------------------------------------------------------------------------------------------------
    cold = [3.0, B(63), B(62), B(61), 2.0, -5.0]       # one ulp apart at the top; 1 / 0.05 and 8 / 0.05 below: e-20, e-160
    c += [Case('T0.05_p', levels=cold, counts=[3, 5, 7, 4, 12, None], nucleus=('solve', 2, 3), T=0.05, **small),
          Case('T0.05_none', levels=cold, counts=[3, 5, 7, 4, 12, None], T=0.05, **small),
          Case('T0.05_k', levels=cold, counts=[3, 5, 7, 4, 12, None], top_k=25, T=0.05, **small),
          Case('T0.7_kp', levels=lv, counts=ct, top_k=25, nucleus=('solve', 3, 5), T=0.7, **small),
          Case('T50_p', levels=lv, counts=ct, nucleus=('solve', 4, 100), T=50.0, **small),
          Case('T50_kp', levels=lv, counts=ct, top_k=12, nucleus=('solve', 2, 1), T=50.0, **small)]
    # ---- vocabulary sizes: 1 .. the kernel's limit, row strides beyond the padded size ---------------------------------------
    c += [Case('V1_p', V=1, levels=[0.75], counts=[1], nucleus=('solve', 0, 0), extra_stride=8),
          Case('V1_k', V=1, levels=[-0.75], counts=[1], top_k=1),
          Case('V5_kp', V=5, levels=[1.0, 0.5, -1.0], counts=[1, 3, 1], top_k=3, nucleus=('solve', 1, 1)),
          Case('V8_kp', V=8, levels=[1.0, 0.5, -1.0], counts=[2, 4, 2], top_k=5, nucleus=('solve', 1, 2), extra_stride=16),
          Case('V13_p', V=13, levels=[1.0, 0.5, -1.0], counts=[2, 6, 5], nucleus=('solve', 1, 4)),
          Case('V1024_kp', V=1024, levels=lv, counts=ct, top_k=14, nucleus=('solve', 2, 6)),
          Case('V1025_kp', V=1025, levels=lv, counts=ct, top_k=14, nucleus=('solve', 2, 6), extra_stride=24)]
    big, bct = [3.0, 2.5, 2.0, 1.5, -3.0], [3, 7, 12, 40, None]
    for V, xs in ((50257, 0), (53247, 8), (53248, 0)):
        c += [Case(f'V{V}_p', V=V, levels=big, counts=bct, nucleus=('solve', 2, 4), T=0.7, rows=8, extra_stride=xs),
              Case(f'V{V}_kp', V=V, levels=big, counts=bct, top_k=50, nucleus=('solve', 3, 17), T=0.7, rows=8,
                   extra_stride=xs),
              Case(f'V{V}_k', V=V, levels=big, counts=bct, top_k=22, rows=8, extra_stride=xs)]
    c.append(Case('V53248_none', V=53248, levels=big, counts=bct, rows=8))
    # ---- the count inside the level-1 bucket reaches top_k exactly at a level-2 bucket with more of the bucket below it -----
    c += [Case('k_l2_exact', levels=[3.0, B(40), B(36), 1.0], counts=[2, 3, 4, None], top_k=5, **small),
          Case('k_l2_exact_negative', levels=[B(33, 0, -1.0), B(40, 0, -1.0), B(50, 0, -1.0), -4.0], counts=[2, 3, 4, None],
               top_k=5, nucleus=('solve', 1, 1), **small)]
    for i, case in enumerate(c):
        case.seed = i
    assert len({case.name for case in c}) == len(c)
    return c


CASES = _cases()

# rows that are not level-generated: (name, row, top_k, top_p, T)
SIGNED_ZERO = ('signed_zero', [0.0, -0.0, -0.0, 1.0, -1.0, -2.0, 0.0, -3.0], 2, None, 1.0)
NEG_INF = ('neg_inf', [2.0, -math.inf, 1.0, -math.inf, 0.0, 0.0, 0.0, 0.0], None, None, 1.0)
EXPLICIT = [SIGNED_ZERO, NEG_INF,
            ('signed_zero_p', [0.0, -0.0, -0.0, 1.0, -1.0, -2.0, 0.0, -3.0], None, 0.55, 1.0),
            ('neg_inf_kp', [2.0, -math.inf, 1.0, -math.inf, 0.0, 0.0, 0.0, 0.0], 6, 0.8228, 1.0)]
