"""Tied-softmax attention problems with an exact float64 reference, for dQ / dK as well as out / dV.

The one-hot problems of test_gpu_parity_bf16.py pin `out` and `dV` bit for bit, but their dS = P o (dP - Delta) is
identically zero, so they cannot see the query / key gradients. Here every query's softmax has exactly 1, 2 or 4 EQUAL
nonzero entries over keys that are DIFFERENT vectors, so dS, dQ and dK are nonzero, and every input, intermediate and
result is a dyadic rational that bf16 (and, for q / k, OCP e4m3) represents exactly:

  * key code: token j of head (b, h) carries a code 64 (e_a + e_b), a < b < 62 (1891 unordered pairs). Tokens that
    share a code inside a query's group form a tie class; classes are laid out so that partners sit FAR apart (first
    key with last key of a group, the cls key in a class, pairs mirrored around the group's middle so they straddle
    16 / 32-key blocks and 64-key streaming tiles, frames 0 and F-1 of a time group);
  * bias lane: k[63] = 64 and q[63] = -128, so the target class scores exactly 0 (lse = ln m is accurate in float32),
    keys sharing one code index score <= -480 after the 1/8 scale and all others <= -992: exp() underflows to 0;
  * private offset: key j also gets +-2 / +-4 along one dim outside its code (distinct within a class), so tied keys
    differ and dQ = sum_j dS_ij k_j / 8 does not cancel;
  * v: members of a class share every v dim but one (`vdim`), where they take distinct values (2, -2) or (2, 1, -1, -2)
    in slot order, so dP_j - Delta = dout[vdim] (v_j[vdim] - mean) is small and never 0; dout is in {-2, -1, 1, 2}
    with dout[vdim of the target] in {1, 2} (exactly 1 for queries of the cls class: its dK sums over every group).
    Small dS keeps the sums that build dK (over queries) and the cls key's dK (over all groups) bf16-exact.

The builder returns the float64 reference (out, lse, dqkv, d(bias) thirds) and asserts its own preconditions; the CPU
suite (test_attention_problems_cpu.py) runs it on every shape the GPU tests use and compares it with the oracle.
"""
from dataclasses import dataclass

import torch

SCALE = 0.125          # head dim 64
_PATTERN = {1: (2.0,), 2: (2.0, -2.0), 4: (2.0, 1.0, -1.0, -2.0)}    # v[vdim] of a class's members in slot order
_OFFSETS = (2.0, -2.0, 4.0, -4.0)                                        # private key offsets by rank in the class
MIN_QUANTUM = 2.0 ** -6                                                  # smallest nonzero |reference| allowed
ZERO_SLACK = 2.0 ** -10                                                  # |got| allowed where the reference is 0
P_REL_NOISE = 2.0 ** -20       # relative error budget of a float32 P = exp2(s log2e - lse log2e) ~ 1/m (1 +- 1e-7)


def _codes():
    pairs = [(a, b) for a in range(62) for b in range(a + 1, 62)]
    return torch.tensor(pairs)                                           # [1891, 2]


def group_layout(n):
    """Tie classes of a group of n keys (slot 0 = the first key: the cls key of a divided-attention group).
    Slot s is paired with its mirror n-1-s (first with last, ...); for n >= 6 the pairs (4i, 4i+1) merge into one
    4-class {4i, 4i+1, n-2-4i, n-1-4i} (cls, first patch and the last two keys share one). The middle slot of an odd n
    stays alone. Returns (class id per slot [n] long, rank of the slot inside its class [n] long, class sizes)."""
    cls = torch.empty(n, dtype=torch.long)
    rank = torch.zeros(n, dtype=torch.long)
    npairs = n // 2
    merge = npairs >= 3
    sizes = []
    k = 0
    while k < npairs:
        if merge and k % 4 == 0 and k + 1 < npairs:
            members = [k, k + 1, n - 2 - k, n - 1 - k]
            k += 2
        else:
            members = [k, n - 1 - k]
            k += 1
        for r, s in enumerate(members):
            cls[s], rank[s] = len(sizes), r
        sizes.append(len(members))
    if n % 2:
        cls[npairs], rank[npairs] = len(sizes), 0
        sizes.append(1)
    return cls, rank, torch.tensor(sizes)


def causal_layout(L):
    """Tie classes of causal text: (0, 1) and (2, 3) so the early queries already see a tie, then blocks of 34 tokens
    whose first 17 pair with their last 17 (distance 17: across every 16-key tile; (4i, 4i+1) with their partners
    merge into a 4-class), the last partial block mirrored in itself."""
    cls = torch.empty(L, dtype=torch.long)
    rank = torch.zeros(L, dtype=torch.long)
    sizes = []

    def add(members):
        for r, s in enumerate(members):
            cls[s], rank[s] = len(sizes), r
        sizes.append(len(members))
    s0 = 0
    for a in range(0, min(L, 4) - 1, 2):
        add([a, a + 1])
        s0 = a + 2
    while s0 < L:
        w = min(34, L - s0)
        h = w // 2
        k = 0
        while k < h:
            if k % 4 == 0 and k + 1 < h:
                add([s0 + k, s0 + k + 1, s0 + k + h, s0 + k + 1 + h])
                k += 2
            else:
                add([s0 + k, s0 + k + h])
                k += 1
        if w % 2:
            add([s0 + w - 1])
        s0 += w
    return cls, rank, torch.tensor(sizes)


@dataclass
class Problem:
    kind: str                 # 'space' | 'time' | 'causal' | 'cls' | 'cross' | 'mq'
    shape: tuple
    heads: int
    qkv: torch.Tensor         # [B, T, 3D] float64, bf16- and (q, k) e4m3-exact
    dout: torch.Tensor        # [B, T, D] ('cls': only row 0 of each sample is used)
    out: torch.Tensor         # [B, T, D]
    lse: torch.Tensor         # [B, H, T] natural log (= ln m)
    mult: torch.Tensor        # [B, H, T] softmax multiplicity m of every query
    dqkv: torch.Tensor        # [B, T, 3D]
    dbias: torch.Tensor       # [3D]: sum dq | 0 | sum dout
    noise: torch.Tensor       # [B, T, 3D] bound on a float32 kernel's deviation caused by P ~ 1/m (1 +- P_REL_NOISE)
    out_noise: torch.Tensor   # [B, T, D]
    blocks: list              # [(qidx [G, nq], kidx [G, nk], causal)] the groups the reference used
    tok_class: torch.Tensor   # [T] tie class of every token (0: the cls key's class in every divided-attention group)
    key_tied: torch.Tensor    # [T] the token is one of 2 or 4 tied keys of its group
    group_slots: torch.Tensor  # [G, nk] token of every slot of a (space / time) group, None otherwise

    def as_cls(self):
        """cls-only operands: q [B, D] (token 0's q), kv [B, T, 2D]; reference out [B, D], dq [B, D], dkv [B, T, 2D]."""
        D = self.heads * 64
        return (self.qkv[:, 0, :D], self.qkv[:, :, D:], self.out[:, 0], self.dqkv[:, 0, :D], self.dqkv[:, :, D:])

    def as_cross(self):
        """'cross' operands in the C-ABI layout: q [contexts*qrep, D], kv [contexts, Tk, 2D], dout [contexts*qrep, D];
        reference out and dq [contexts*qrep, D], dkv [contexts, Tk, 2D]. Tokens 0..qrep-1 of a context are its query
        rows, the Tk tokens behind them its keys."""
        D = self.heads * 64
        qrep = self.shape[1]
        rows = lambda x: x[:, :qrep].reshape(-1, D)                       # noqa: E731
        return (rows(self.qkv[..., :D]), self.qkv[:, qrep:, D:], rows(self.dout), rows(self.out),
                rows(self.dqkv[..., :D]), self.dqkv[:, qrep:, D:])

    def as_mq(self):
        """'mq' operands of the pooler: q [B, NQ, H*64] (shared: [NQ, H*64], the same rows in every clip),
        kv [B, Tk, 128], dout [B, NQ, H*64]; reference out [B, NQ, H*64], dq like q (shared: the sum over the clips),
        dkv [B, Tk, 128]. Query token n*H + h of the single-head problem is head h of query n."""
        B, NQ, H, Tk, shared = self.shape
        fold = lambda x: x[:, :NQ * H].reshape(B, NQ, H * 64)            # noqa: E731
        q, dq = fold(self.qkv[..., :64]), fold(self.dqkv[..., :64])
        if shared:
            q, dq = q[0], dq.sum(0)
        return q, self.qkv[:, NQ * H:, 64:], fold(self.dout), fold(self.out), dq, self.dqkv[:, NQ * H:, 64:]


def _bf16_exact(x):
    return torch.equal(x.to(torch.bfloat16).double(), x)


def _e4m3_exact(x):
    return torch.equal(x.to(torch.float8_e4m3fn).double(), x)


def _ulp_bf16(x):
    e = torch.floor(torch.log2(x.abs().clamp_min(1e-30)))
    return torch.exp2(e - 7)


def _reference(q, k, v, dO, blocks):
    """Grouped float64 attention + backward on [B, H, T, 64] tensors. Returns out, lse, dq, dk, dv, their noise bounds
    and the P rows of every block."""
    B, H, T, _ = q.shape
    out = torch.zeros_like(v)
    lse = torch.zeros(B, H, T, dtype=torch.float64)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    nq_, nk_, nv_, no_ = (torch.zeros_like(q) for _ in range(4))
    probs = []
    for qidx, kidx, causal in blocks:
        G, nq = qidx.shape
        nk = kidx.shape[1]
        Q, K, V, dOq = q[:, :, qidx], k[:, :, kidx], v[:, :, kidx], dO[:, :, qidx]       # [B,H,G,n,64]
        s = Q @ K.transpose(-1, -2) * SCALE
        if causal:
            s = s.masked_fill(torch.ones(nq, nk, dtype=torch.bool).triu(1), float('-inf'))
        P = torch.softmax(s, -1)
        P = torch.where(P < 1e-100, torch.zeros_like(P), P)             # exp(-480) residue: exactly 0 in float32
        probs.append(P)
        ls = torch.logsumexp(s, -1)
        O = P @ V
        dP = dOq @ V.transpose(-1, -2)
        delta = (dOq * O).sum(-1, keepdim=True)
        dS = P * (dP - delta)
        dSa = P * (dP - delta).abs()
        fq, fk = qidx.reshape(-1), kidx.reshape(-1)
        out[:, :, fq] = O.reshape(B, H, -1, 64)
        lse[:, :, fq] = ls.reshape(B, H, -1)
        no_[:, :, fq] = (P @ V.abs()).reshape(B, H, -1, 64)
        dq.index_add_(2, fq, (dS @ K * SCALE).reshape(B, H, -1, 64))
        nq_.index_add_(2, fq, (dSa @ K.abs() * SCALE).reshape(B, H, -1, 64))
        dk.index_add_(2, fk, (dS.transpose(-1, -2) @ Q * SCALE).reshape(B, H, -1, 64))
        nk_.index_add_(2, fk, (dSa.transpose(-1, -2) @ Q.abs() * SCALE).reshape(B, H, -1, 64))
        dv.index_add_(2, fk, (P.transpose(-1, -2) @ dOq).reshape(B, H, -1, 64))
        nv_.index_add_(2, fk, (P.transpose(-1, -2) @ dOq.abs()).reshape(B, H, -1, 64))
    return out, lse, dq, dk, dv, (nq_, nk_, nv_, no_), probs


def _build(kind, shape, B, H, T, blocks, tok_class, tok_rank, class_size, class_groups, seed, group_slots=None,
           shared_q=False):
    """tok_class / tok_rank [T]: tie class and rank of every token (class sizes are group-local for divided attention;
    class 0 is the cls class there). Queries pick their target class in _targets; everything else follows here.
    shared_q: every sample uses the codes and targets of sample 0, so q is the same tensor in all of them (v, the
    private offsets and dout still differ)."""
    g = torch.Generator().manual_seed(seed)
    C = int(class_size.numel())
    codes = _codes()
    assert C <= codes.shape[0], f'{C} tie classes need more than {codes.shape[0]} codes'
    # per (b, h): a random code per class, a random v dim per class, random offset dims
    code_of = torch.argsort(torch.rand(B, H, codes.shape[0], generator=g), -1)[..., :C]          # [B,H,C]
    if shared_q:
        code_of = code_of[:1].expand(B, H, C)
    ab = codes[code_of]                                                                          # [B,H,C,2]
    vdim = torch.randint(0, 64, (B, H, C), generator=g)
    target = _targets(kind, B, H, T, blocks, tok_class, class_size, class_groups, g)             # [B,H,T]
    if shared_q:
        target = target[:1].expand(B, H, T).contiguous()

    def code_vec(cab, val):
        x = torch.zeros(*cab.shape[:-1], 64, dtype=torch.float64)
        x.scatter_(-1, cab, val)
        return x
    tab = ab[:, :, tok_class]                                                                    # [B,H,T,2]
    k = code_vec(tab, 64.0)
    k[..., 63] = 64.0
    # private offset along a dim outside the token's own code (and not the bias lane)
    od = torch.randint(0, 62, (B, H, T), generator=g)
    od = torch.where((od == tab[..., 0]) | (od == tab[..., 1]), torch.full_like(od, 62), od)   # dim 62: in no code
    offs = torch.tensor(_OFFSETS, dtype=torch.float64)[tok_rank % 4].expand(B, H, T)
    k.scatter_add_(-1, od[..., None], offs[..., None])
    q = code_vec(ab.gather(2, target[..., None].expand(B, H, T, 2)), 64.0)
    q[..., 63] = -128.0
    # v: class base in {-1, 0, 1}, the class's vdim by rank
    base = torch.randint(-1, 2, (B, H, C, 64), generator=g).double()
    v = base[:, :, tok_class].clone()
    pat = torch.zeros(5, 4, dtype=torch.float64)
    for m, p in _PATTERN.items():
        pat[m, :m] = torch.tensor(p)
    tvd = vdim[:, :, tok_class]
    v.scatter_(-1, tvd[..., None], pat[class_size[tok_class], tok_rank].expand(B, H, T)[..., None].clone())
    sgn = torch.where(torch.rand(B, H, T, 64, generator=g) < 0.5, -1.0, 1.0).double()
    dO = sgn * torch.randint(1, 3, (B, H, T, 64), generator=g).double()
    tvdim = vdim.gather(2, target)
    one = (target == 0) if kind in ('space', 'time') else torch.zeros_like(target, dtype=torch.bool)
    dval = torch.randint(1, 3, (B, H, T), generator=g).double()
    dval = torch.where(one, torch.ones_like(dval), dval)
    dO.scatter_(-1, tvdim[..., None], dval[..., None])

    out, lse, dq, dk, dv, (nq_, nk_, nv_, no_), probs = _reference(q, k, v, dO, blocks)
    pack = lambda x: x.permute(0, 2, 1, 3).reshape(B, T, H * 64)          # noqa: E731  head-major inside a third
    flush = lambda x: torch.where(x.abs() < 1e-100, torch.zeros_like(x), x)  # noqa: E731
    qkv = torch.cat([pack(q), pack(k), pack(v)], -1)
    dqkv = flush(torch.cat([pack(dq), pack(dk), pack(dv)], -1))
    noise = torch.cat([pack(nq_), pack(nk_), pack(nv_)], -1) * P_REL_NOISE
    dout = pack(dO)
    rows_q = sorted({int(i) for qidx, _, _ in blocks for i in qidx.reshape(-1)})
    dbias = torch.cat([dqkv[:, rows_q, :H * 64].sum((0, 1)), torch.zeros(H * 64, dtype=torch.float64),
                       dout[:, rows_q].sum((0, 1))])
    mult = torch.zeros(B, H, T, dtype=torch.long)
    for (qidx, _, _), P in zip(blocks, probs):
        mult[:, :, qidx.reshape(-1)] = (P > 0).sum(-1).reshape(B, H, -1)
    key_tied = (class_size[tok_class] == 2) | (class_size[tok_class] == 4)
    p = Problem(kind, shape, H, qkv, dout, flush(pack(out)), lse, mult, dqkv, dbias, noise,
                pack(no_) * P_REL_NOISE, blocks, tok_class, key_tied, group_slots)
    _check(p, probs, rows_q)
    return p


def _targets(kind, B, H, T, blocks, tok_class, class_size, class_groups, g):
    """Target class of every query [B, H, T] (tokens that are no query: their own class, unused)."""
    target = tok_class.expand(B, H, T).clone()
    tied = (class_size == 2) | (class_size == 4)
    if kind in ('space', 'time', 'cls'):
        for qidx, kidx, _ in blocks:
            G, nq = qidx.shape
            if nq == 1 and kidx.shape[1] == T:              # the cls query: any class tied over ALL tokens
                glob = torch.bincount(tok_class, minlength=class_size.numel())
                cand = torch.nonzero(tied & (glob == class_size) & (torch.arange(class_size.numel()) != 0)).flatten()
                if kind == 'cls' and bool(tied[tok_class[0]]):
                    cand = torch.cat([tok_class[:1], cand])
                if cand.numel() == 0 and int(glob[0]) in (2, 4):
                    cand = torch.zeros(1, dtype=torch.long)
                if cand.numel() == 0:
                    continue
                pick = torch.randint(0, cand.numel(), (B, H), generator=g)
                if kind == 'cls':
                    pick[0, 0] = 0                             # one (b, h) targets the first key's class
                target[:, :, qidx[0, 0]] = cand[pick]
                continue
            # group queries: one random query per group targets the cls class (0), the others cover the group's
            # other tied classes in a random order, so every tied key is some query's target
            cand = class_groups                                # [G, nc] tied classes of each group other than 0
            r = torch.argsort(torch.rand(B, H, G, nq, generator=g), -1)
            if cand.shape[1] == 0:
                t = torch.zeros(B, H, G, nq, dtype=torch.long)
            else:
                t = cand[torch.arange(G)[:, None], (r - 1).clamp_min(0) % cand.shape[1]]
                t = torch.where(r == 0, torch.zeros_like(t), t)
            if not bool(tied[0]):
                t = tok_class[qidx].expand(B, H, G, nq)
            target[:, :, qidx.reshape(-1)] = t.reshape(B, H, -1)
        return target
    if kind in ('cross', 'mq'):
        # round-robin over the tied classes, from a start that differs per (b, h) -- (0, 0) starts at class 0, the one
        # of the first and the last key: with at least as many queries as tied classes every tied key is some query's
        # target, and a class collects at most ceil(queries / classes) queries
        (qidx, _, _), = blocks
        cand = torch.nonzero(tied).flatten()
        if cand.numel():
            start = torch.randint(0, cand.numel(), (B, H), generator=g)
            start[0, 0] = 0
            target[:, :, qidx[0]] = cand[(torch.arange(qidx.shape[1]) + start[..., None]) % cand.numel()]
        return target
    # causal: count of each class visible to query t
    C = class_size.numel()
    vis = torch.zeros(T, C, dtype=torch.long)
    vis[torch.arange(T), tok_class] = 1
    vis = vis.cumsum(0)
    ok = (vis == 2) | (vis == 4)
    completes = ok[torch.arange(T), tok_class]                 # token t completes its own class's tie
    r = torch.rand(B, H, T, C, generator=g) * ok
    pick = r.argmax(-1)
    pick = torch.where(completes, tok_class.expand(B, H, T), pick)
    none = ~ok.any(-1)
    return torch.where(none, tok_class.expand(B, H, T), pick)


def _check(p, probs, rows_q):
    """The builder's own preconditions (see the module docstring)."""
    D = p.heads * 64
    for name, x in (('qkv', p.qkv), ('dout', p.dout), ('out', p.out), ('dqkv', p.dqkv)):
        assert _bf16_exact(x), f'{name} is not bf16-exact'
    assert _e4m3_exact(p.qkv[..., :2 * D]), 'q / k are not e4m3-exact'
    for P in probs:
        nz = P > 0
        m = nz.sum(-1)
        assert bool(((m == 1) | (m == 2) | (m == 4)).all()), 'a softmax row has a multiplicity other than 1, 2, 4'
        want = torch.where(nz, 1.0 / m[..., None].double(), torch.zeros_like(P))
        assert torch.equal(P, want), 'a softmax row is not {1}, {1/2, 1/2} or {1/4 x4}'
    assert torch.allclose(p.lse[:, :, rows_q], torch.log(p.mult[:, :, rows_q].double()), rtol=0, atol=1e-12)
    # nonzero values: at least the 2^-6 quantum, and a float32 kernel's P noise rounds away in bf16
    for name, x, nb in (('out', p.out, p.out_noise), ('dqkv', p.dqkv, p.noise)):
        nz = x != 0
        if bool(nz.any()):
            assert x[nz].abs().min().item() >= MIN_QUANTUM, f'{name}: nonzero value below 2^-6'
            assert bool((nb[nz] <= _ulp_bf16(x[nz]) / 4).all()), f'{name}: P noise reaches a quarter bf16 ulp'
        if bool((~nz).any()):
            assert nb[~nz].max().item() <= ZERO_SLACK / 4, f'{name}: P noise of a zero reference reaches 2^-12'
    # gradients: dq on (almost) every query row whose softmax is tied, dk on (almost) every key in a tied class
    qrows = torch.zeros(p.qkv.shape[1], dtype=torch.bool)
    qrows[rows_q] = True
    dq = p.dqkv[..., :D].reshape(*p.dqkv.shape[:2], p.heads, 64)
    dk = p.dqkv[..., D:2 * D].reshape(*p.dqkv.shape[:2], p.heads, 64)
    tied_q = (p.mult.permute(0, 2, 1) > 1) & qrows[None, :, None]
    dq_nz = (dq != 0).any(-1)
    assert bool((dq_nz <= tied_q).all()), 'dq != 0 on a row with a one-hot softmax'
    assert not tied_q.any() or dq_nz[tied_q].double().mean().item() >= 0.9, \
        'fewer than 90 % of the tied query rows have dq != 0'
    tied_k = p.key_tied[None, :, None].expand_as(dk[..., 0])
    if p.kind in ('cross', 'mq'):
        # fewer queries than tied classes (5 rows over 256 keys) leave classes that no softmax of this (b, h) ties: the
        # tied keys are those some query gives 1/2 or 1/4 -- all of key_tied once the queries go round
        (qidx, kidx, _), = p.blocks
        hit = ((probs[0] > 0) & (probs[0] < 1)).any(-2)[:, :, 0]                                   # [B, H, nk]
        tied_k = torch.zeros_like(tied_k)
        tied_k[:, kidx[0]] = hit.permute(0, 2, 1)
        assert bool((tied_k <= p.key_tied[None, :, None]).all())
        if qidx.shape[1] >= p.tok_class[p.key_tied].unique().numel():
            assert torch.equal(tied_k, p.key_tied[None, :, None].expand_as(tied_k)), 'a tied key is no query\'s target'
        assert not p.key_tied.any() or bool(tied_k.any(1).all()), 'a (b, h) without a tied key'
    dk_nz = (dk != 0).any(-1)
    if p.kind != 'cls':
        assert dk_nz[tied_k].double().mean().item() >= 0.9, 'fewer than 90 % of the tied keys have dk != 0'
        assert bool((dk_nz <= tied_k).all()), 'dk != 0 on a key outside every tie'
    if p.kind in ('space', 'time', 'cls') and p.mult[:, :, 0].max().item() > 1:
        assert bool(dq_nz[:, 0].any()), 'the cls row has dq == 0'
        assert bool(dk_nz[:, 0].any()), 'the cls key has dk == 0'


def divided_problem(B, F, N, H, mode, seed=0):
    """Space (groups = frames) or time (groups = locations) attention over T = 1 + F N tokens; cls query over all."""
    T = 1 + F * N
    n = 1 + (N if mode == 'space' else F)
    G = F if mode == 'space' else N
    lcls, lrank, lsize = group_layout(n)
    if mode == 'space':
        patches = 1 + torch.arange(F)[:, None] * N + torch.arange(N)[None]           # [G=F, N]
    else:
        patches = 1 + torch.arange(F)[None, :] * N + torch.arange(N)[:, None]        # [G=N, F]
    slots = torch.cat([torch.zeros(G, 1, dtype=torch.long), patches], 1)             # [G, n]
    # global class ids: the cls key's class is 0 in every group, every other (group, local class) its own id
    c0 = int(lcls[0])
    other = [c for c in range(lsize.numel()) if c != c0]
    loc2glob = torch.zeros(G, lsize.numel(), dtype=torch.long)
    loc2glob[:, other] = 1 + torch.arange(G)[:, None] * len(other) + torch.arange(len(other))[None]
    tok_class = torch.empty(T, dtype=torch.long)
    tok_rank = torch.empty(T, dtype=torch.long)
    tok_class[slots.reshape(-1)] = loc2glob[:, lcls].reshape(-1)
    tok_rank[slots.reshape(-1)] = lrank.expand(G, n).reshape(-1)
    class_size = torch.empty(1 + G * len(other), dtype=torch.long)      # group-local sizes
    class_size[0] = lsize[c0]
    class_size[1:] = lsize[other].repeat(G)
    tied_other = [c for c in other if int(lsize[c]) in (2, 4)]
    class_groups = loc2glob[:, tied_other]
    blocks = [(patches, slots, False), (torch.zeros(1, 1, dtype=torch.long), torch.arange(T)[None], False)]
    return _build(mode, (B, F, N, H), B, H, T, blocks, tok_class, tok_rank, class_size, class_groups, seed, slots)


def causal_problem(B, L, H, seed=0):
    cls, rank, size = causal_layout(L)
    blocks = [(torch.arange(L)[None], torch.arange(L)[None], True)]
    return _build('causal', (B, L, H), B, H, L, blocks, cls, rank, size, None, seed)


def cls_problem(B, T, H, seed=0):
    """The cls query (token 0's q) over all T keys: the cls-only kernels of the last block."""
    cls, rank, size = group_layout(T)
    blocks = [(torch.zeros(1, 1, dtype=torch.long), torch.arange(T)[None], False)]
    return _build('cls', (B, T, H), B, H, T, blocks, cls, rank, size, None, seed)


def _query_key_problem(kind, shape, B, H, nq, Tk, seed, shared_q=False):
    """nq query tokens (0..nq-1, one untied class of their own that is no key) over Tk key tokens laid out by
    group_layout(Tk): partners mirrored around the middle, so they straddle every 16- and 64-key boundary."""
    lcls, lrank, lsize = group_layout(Tk)
    tok_class = torch.cat([torch.full((nq,), lsize.numel()), lcls])
    tok_rank = torch.cat([torch.zeros(nq, dtype=torch.long), lrank])
    class_size = torch.cat([lsize, torch.ones(1, dtype=torch.long)])
    blocks = [(torch.arange(nq)[None], nq + torch.arange(Tk)[None], False)]
    return _build(kind, shape, B, H, nq + Tk, blocks, tok_class, tok_rank, class_size, None, seed, shared_q=shared_q)


def cross_problem(contexts, qrep, H, Tk, seed=0):
    """Decoder cross-attention: qrep query rows per context over that context's Tk keys (Problem.as_cross())."""
    return _query_key_problem('cross', (contexts, qrep, H, Tk), contexts, H, qrep, Tk, seed)


def mq_problem(B, NQ, H, Tk, shared, seed=0):
    """The pooler: ONE 64-channel key / value head for all H query heads -- a single-head problem with NQ * H queries
    per clip (Problem.as_mq()). shared: one [NQ, H*64] query tensor for every clip; its reference dq is the sum over the
    clips, which must meet the same preconditions as every other reference value."""
    p = _query_key_problem('mq', (B, NQ, H, Tk, bool(shared)), B, 1, NQ * H, Tk, seed, shared_q=bool(shared))
    if shared:
        nq = NQ * H
        q = p.qkv[:, :nq, :64]
        assert torch.equal(q, q[:1].expand_as(q)), 'shared queries differ between the clips'
        dq, nb = p.dqkv[:, :nq, :64].sum(0), p.noise[:, :nq, :64].sum(0)
        assert _bf16_exact(dq), 'the summed dq is not bf16-exact'
        nz = dq != 0
        if bool(nz.any()):
            assert dq[nz].abs().min().item() >= MIN_QUANTUM
            assert bool((nb[nz] <= _ulp_bf16(dq[nz]) / 4).all()), 'summed dq: P noise reaches a quarter bf16 ulp'
        assert nb[~nz].numel() == 0 or nb[~nz].max().item() <= ZERO_SLACK / 4
        tied_q = p.mult[:, 0, :nq].max(0).values > 1
        assert not tied_q.any() or nz.any(-1)[tied_q].double().mean().item() >= 0.9, \
            'fewer than 90 % of the tied shared queries have a summed dq != 0'
    return p


# --------------------------------------------------------------------------------------------------------------------
# the shapes of tests/test_gpu_attention_ties.py (one list per kernel family; the CPU suite builds every one of them)
# --------------------------------------------------------------------------------------------------------------------
SPACE_RESIDENT = [(2, 3, 1, 2), (2, 2, 31, 1), (2, 4, 32, 2), (2, 1, 63, 12), (2, 2, 64, 1), (2, 4, 196, 12),
                  (1, 1, 256, 2), (2, 1, 287, 1)]                    # (B, F, N, H): N + 1 in {2, 32, ..., 257, 288}
SPACE_RESIDENT_273 = [(1, 1, 272, 1), (1, 2, 287, 1)]               # bf16 resident forward, 273-288 keys
SPACE_STREAM = [(1, 1, 288, 1), (1, 2, 576, 2), (1, 1, 591, 1), (1, 1, 640, 1)]
SPACE_LARGE_RESIDENT = [(2, 1, 576, 1), (1, 1, 590, 1)]             # 577 / 591 keys, 4-wave resident backward
SPACE_FP8 = [(1, 2, 576, 2)]
TIME_REGISTER = [(2, 1, 3, 2), (2, 2, 3, 1), (2, 3, 7, 1), (2, 4, 9, 2), (1, 8, 9, 3), (1, 16, 9, 2)]
TIME_MFMA = [(1, 16, 196, 12), (2, 5, 9, 4), (1, 12, 7, 8), (1, 8, 20, 16)]
TIME_GENERIC = [(2, 6, 5, 3)]
F32_GENERIC = [('space', (2, 2, 31, 1)), ('time', (2, 3, 7, 1))]
CAUSAL = [(2, 5, 2), (3, 77, 8), (2, 130, 12), (2, 256, 2), (2, 272, 2)]    # (B, L, H)
CLS = [(2, 1, 2), (2, 99, 2), (2, 785, 12), (2, 3137, 12)]                 # (B, T, H)
# the shapes of tests/test_gpu_narrator_ties.py
# (contexts, qrep, H, Tk) of lvl_cross_attn_rows_fwd, one per dispatch branch and tail
CROSS_FWD_BF16 = [(2, 2, 1, 2), (2, 16, 2, 16), (2, 17, 1, 33), (1, 65, 2, 255), (2, 5, 3, 256),    # MFMA kernel
                  (2, 4, 2, 300), (1, 2, 1, 600),           # keys of a context in LDS, 257..600 of them
                  (2, 3, 2, 601), (3, 1, 2, 37)]            # one workgroup per row: past LDS with qrep >= 2, qrep = 1
CROSS_FWD_F32 = [(2, 5, 2, 37), (1, 2, 1, 300), (2, 3, 1, 301), (3, 1, 2, 37)]
# lvl_cross_attn_rows_bwd: the MFMA shapes of the forward, three rounds with 2 rows in the last, twelve heads at 256 keys
CROSS_BWD = [s for s in CROSS_FWD_BF16 if s[3] <= 256 and s[1] >= 2] + [(1, 130, 1, 200), (2, 64, 12, 256)]
MQ = [(2, 5, 3, 9), (2, 24, 4, 65), (1, 11, 3, 33), (2, 32, 8, 128)]         # (B, NQ, H, Tk), shared and per-sample
DECODE = [(2, 5, 2, 5), (3, 77, 8, 77), (2, 130, 2, 160)]                      # (B, L, H, cache capacity)


def all_cases():
    """(kind, shape) of every problem the GPU tests build."""
    sp = SPACE_RESIDENT + SPACE_RESIDENT_273 + SPACE_STREAM + SPACE_LARGE_RESIDENT + SPACE_FP8
    sp += [s for m, s in F32_GENERIC if m == 'space']
    tm = TIME_REGISTER + TIME_MFMA + TIME_GENERIC + [s for m, s in F32_GENERIC if m == 'time']
    return ([('space', s) for s in dict.fromkeys(sp)] + [('time', s) for s in dict.fromkeys(tm)] +
            [('causal', s) for s in CAUSAL] + [('cls', s) for s in CLS])


def narrator_cases():
    """(kind, shape) of every problem tests/test_gpu_narrator_ties.py builds."""
    cross = dict.fromkeys(CROSS_FWD_BF16 + CROSS_FWD_F32 + CROSS_BWD)
    causal = [s[:3] for s in DECODE if s[:3] not in CAUSAL]
    return ([('cross', s) for s in cross] + [('mq', s + (sh,)) for s in MQ for sh in (False, True)] +
            [('causal', s) for s in causal])


def make(kind, shape, seed=0):
    if kind in ('space', 'time'):
        B, F, N, H = shape
        return divided_problem(B, F, N, H, kind, seed)
    if kind == 'causal':
        return causal_problem(*shape, seed=seed)
    if kind == 'cross':
        return cross_problem(*shape, seed=seed)
    if kind == 'mq':
        return mq_problem(*shape, seed=seed)
    return cls_problem(*shape, seed=seed)
