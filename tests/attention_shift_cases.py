"""Attention problems whose softmax rows sit far from zero, a float64 reference and a DERIVED per-element error bound.

Every other attention test keeps its row maxima at or near zero (tied-softmax and one-hot problems: exactly 0; random
cases: below about 8), so the max subtraction, the online-softmax rescale, the merge of partial records, the backward's
P = exp2(s kExp2 - lse log2e) and the overflow masks of padded keys only ever see values that cannot show an error. Here
the inputs are the usual random ones (q, k, v ~ 1.5 N(0, 1), dout ~ N(0, 1), rounded to the tested type; float32 cases
keep q and k bf16-exact so that the score products of the f32-class kernels are exact before accumulation) with two
channels of every head overwritten:

  * row-shift lane (channel 63): k[..., 63] = 8 and q[b, i, h, 63] = PAL[(7 i + 3 h + 5 b) % 11]: every score of row i
    moves by exactly that palette entry (0, +-8, +-24, +-48, +-96, +-120). Any 11 consecutive rows hold all of them.
  * key-staircase lane (channel 62): q[..., 62] = 8 and k[token, 62] = stair * step(slot), slot = the key's position in
    its group, step = slot // 16 (time groups, at most 17 keys: step = slot), stair in {0, +4, -4}. With +4 the running
    maximum rises in every key tile and everything accumulated so far is rescaled by e^-4; with -4 the first tile dominates.

All lane values are bf16-exact (asserted). They are NOT e4m3-exact, so the fp8 QK path is out of scope here.

Key-masked cases carry a visibility mask per context; HIDE_LOUD additionally gives every hidden key a staircase value 32
above every visible key's, so that hidden keys hold the largest scores of their context.

Reference: grouped float64 attention and backward over the same `blocks` lists as attention_problems._reference. Next to
every result X it returns the abs-companion A_X, the same contraction over absolute values:

    A_out = P |v|      aS = P o (|dO| |v|^T + sum |dO| o (P |v|))      A_dq = aS |k| / 8      A_dk = aS^T |q| / 8
    A_dv = P^T |dO|

Bound, per element:   bound(X) = rowwise(u + eps_i) A_X + u |X_ref| + 2^-20     (dk, dv: the row factor inside the sum
over queries)

  * eps_i = 4 ulp_f32(log2e (|c_i| + D_i + 8)), c_i the row's shift, D_i the largest |staircase value| among the keys
    the row sees: the two float32 roundings of the exponent argument (s kExp2 and lse log2e, or mk). The only term
    that grows with the shift.
  * u = 2^-7 for bf16: P rounded to bf16 (2^-9), dS rounded (2^-9), delta taken from the rounded out (2^-9, inside aS)
    and the result's own rounding.
  * u = 2^-15 for float32: three f32-class products at the 2^-17 the header states, plain-f32 accumulation over
    <= 1024 terms.
  * lse: |got - ref| <= eps_i + 2^-20.

The constants follow from the documented arithmetic; they are not fitted to a run.

emulate() is a float32 model of the kernels' softmax (online forward over 64-key tiles with the exp2 forms, float32 lse,
backward from that lse; bf16 mode rounds P, dS and the results as the kernels do), with four switchable faults. The CPU
suite holds it inside 0.6 x bound on every case and requires every fault to be rejected.
"""
import functools
import math
from dataclasses import dataclass

import torch

SCALE = 0.125
LOG2E = 1.4426950408889634
PAL = (0.0, 8.0, -8.0, 24.0, -24.0, 48.0, -48.0, 96.0, -96.0, 120.0, -120.0)
STAIRS = (0.0, 4.0, -4.0)
U = {torch.bfloat16: 2.0 ** -7, torch.float32: 2.0 ** -15}
FLOOR = 2.0 ** -20
LOUD = 32.0                      # HIDE_LOUD: hidden keys' staircase value above the largest visible one
NAMES = ('out', 'dq', 'dk', 'dv')


def ulp_f32(x):
    """ulp of a positive float32 of magnitude x (float64 tensor in, float64 out)."""
    return torch.exp2(torch.floor(torch.log2(x)) - 23)


def _round(x, dt):
    return x.to(dt).double()


# ----------------------------------------------------------------------------------------------------------------------
# the two engines: one block of G groups, Q [B,H,G,nq,64], K / V [B,H,G,nk,64], dO like Q, vis [B,H|1,G,nq|1,nk] bool
# ----------------------------------------------------------------------------------------------------------------------
def _block_reference(Q, K, V, dO, vis, u):
    s = Q @ K.transpose(-1, -2) * SCALE
    vis = vis.expand(s.shape)
    empty = ~vis.any(-1, keepdim=True)                                # a row without a visible key: uniform, dS = 0
    s = torch.where(vis | empty, s.masked_fill(empty.expand_as(s), 0.0), torch.full_like(s, -math.inf))
    ls = torch.logsumexp(s, -1, keepdim=True)
    P = torch.exp(s - ls)
    aV, adO = V.abs(), dO.abs()
    O, aO = P @ V, P @ aV
    dP = dO @ V.transpose(-1, -2)
    delta = (dO * O).sum(-1, keepdim=True)
    live = (~empty).to(P.dtype)
    dS = P * (dP - delta) * live
    aS = P * (adO @ aV.transpose(-1, -2) + (adO * aO).sum(-1, keepdim=True)) * live
    # the row factor u + eps_i
    c = Q[..., 63:64].abs() * K[..., :1, 63:64].abs().transpose(-1, -2) * SCALE                  # [.., nq, 1]
    stair = (Q[..., 62:63].abs() * K[..., 62].abs()[..., None, :] * SCALE).expand(s.shape)       # [.., nq, nk]
    D = torch.where(vis, stair, torch.zeros_like(stair)).max(-1, keepdim=True).values
    eps = 4 * ulp_f32(LOG2E * (c + D + 8.0))
    r = u + eps
    return {'out': O, 'lse': ls[..., 0], 'dq': dS @ K * SCALE, 'dk': dS.transpose(-1, -2) @ Q * SCALE,
            'dv': P.transpose(-1, -2) @ dO,
            'b_out': r * aO, 'b_lse': eps[..., 0], 'b_dq': r * (aS @ K.abs()) * SCALE,
            'b_dk': (r * aS).transpose(-1, -2) @ Q.abs() * SCALE, 'b_dv': (r * P).transpose(-1, -2) @ adO}


def _block_emulation(Q, K, V, dO, vis, bf, fault):
    """float32 model of the kernels. fault: None | 'nomax' | 'pad' | 'stale' | 'lse'."""
    f32 = torch.float32
    r = (lambda x: x.to(torch.bfloat16).to(f32)) if bf else (lambda x: x)
    Q, K, V, dO = (x.to(f32) for x in (Q, K, V, dO))
    c = torch.tensor(SCALE * LOG2E, dtype=f32)
    l2e = torch.tensor(LOG2E, dtype=f32)
    ninf = torch.tensor(-math.inf, dtype=f32)
    S = Q @ K.transpose(-1, -2)
    vis = vis.expand(S.shape)
    empty = ~vis.any(-1, keepdim=True)
    S = torch.where(vis, S, ninf)
    nk = K.shape[-2]
    m = torch.full(S.shape[:-1] + (1,), -math.inf, dtype=f32)
    l = torch.zeros_like(m)
    acc = torch.zeros(S.shape[:-1] + (64,), dtype=f32)
    for t in range(0, nk, 64):
        st = S[..., t:t + 64]
        mn = torch.maximum(m, st.max(-1, keepdim=True).values)
        ms = torch.where(mn == ninf, torch.zeros_like(mn), mn)       # a tile without a visible key so far
        if fault == 'nomax':
            ms = torch.zeros_like(ms)
        stale = fault == 'stale' and t > 0 and t + 64 >= nk                      # the last tile: the maximum before its update
        al = torch.exp2((m - (m if stale else ms)) * c)
        if fault == 'nomax':
            al = torch.ones_like(al)
        p = torch.exp2(st * c - ms * c)
        l = l * al + p.sum(-1, keepdim=True)
        acc = acc * al + r(p) @ V[..., t:t + 64, :]
        m = mn
    mean_v = V.mean(-2, keepdim=True).expand_as(acc)
    O = r(torch.where(empty, mean_v, acc / l))
    ms = torch.where(m == ninf, torch.zeros_like(m), m)
    if fault == 'nomax':
        ms = torch.zeros_like(ms)
    lse = (ms * c + torch.log2(l)) / l2e
    lse = torch.where(empty, torch.full_like(lse, math.log(nk)), lse)
    if fault == 'lse':
        lse = lse + (2.0 ** -4 if bf else 2.0 ** -10)
    Kb, Vb, Sb = K, V, torch.where(empty, torch.zeros_like(S), S)    # empty rows: uniform (every score equal)
    if fault == 'pad' and nk % 16:
        pad = 16 - nk % 16
        zk = torch.zeros(K.shape[:-2] + (pad, 64), dtype=f32)
        Kb, Vb = torch.cat([K, zk], -2), torch.cat([V, zk], -2)
        Sb = torch.cat([Sb, torch.zeros(S.shape[:-1] + (pad,), dtype=f32)], -1)    # score 0, left unmasked
    P = torch.exp2(Sb * c - lse * l2e)
    dP = dO @ Vb.transpose(-1, -2)
    delta = (dO * O).sum(-1, keepdim=True)
    dS = r(P * (dP - delta))
    dS = torch.where(empty, torch.zeros_like(dS), dS)
    dk = (dS.transpose(-1, -2) @ Q * SCALE)[..., :nk, :]
    dv = (r(P).transpose(-1, -2) @ dO)[..., :nk, :]
    return {'out': O, 'lse': lse[..., 0], 'dq': r(dS @ Kb * SCALE), 'dk': dk, 'dv': dv}


# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    kind: str                 # 'space' | 'time' | 'causal' | 'cls' | 'cross' | 'mq' | 'keymask'
    shape: tuple
    heads: int
    dtype: torch.dtype
    stair: float
    q: torch.Tensor           # [B, H, T, 64] float64, exact in dtype (float32 cases: q and k bf16-exact)
    k: torch.Tensor
    v: torch.Tensor
    dO: torch.Tensor
    blocks: list              # [(qidx [G, nq], kidx [G, nk], causal)]
    vis: torch.Tensor         # [B, T] bool visibility of every key token per context, or None
    ref: dict                 # 'out' 'dq' 'dk' 'dv' [B, H, T, 64], 'lse' [B, H, T]
    acc: dict                 # the rowwise(u + eps) A_X part of every bound, 'lse': eps_i

    @property
    def u(self):
        return U[self.dtype]

    def pack(self, x):
        """[B, H, T, 64] -> [B, T, H*64] (head-major inside a third); [B, H, T] stays."""
        B, H, T = x.shape[:3]
        return x.permute(0, 2, 1, 3).reshape(B, T, H * 64) if x.dim() == 4 else x

    def bound_of(self, ref, acc):
        return acc + self.u * ref.abs() + FLOOR

    def packed(self, name):
        """(reference, bound) of 'out' | 'dq' | 'dk' | 'dv' as [B, T, H*64], of 'lse' as [B, H, T]."""
        if name == 'lse':
            return self.ref['lse'], self.acc['lse'] + FLOOR
        ref, acc = self.pack(self.ref[name]), self.pack(self.acc[name])
        return ref, self.bound_of(ref, acc)

    @property
    def qkv(self):
        return torch.cat([self.pack(self.q), self.pack(self.k), self.pack(self.v)], -1)

    @property
    def dout(self):
        return self.pack(self.dO)

    def query_rows(self):
        return sorted({int(i) for qidx, _, _ in self.blocks for i in qidx.reshape(-1)})

    def as_cross(self):
        """The C-ABI layout of attention_problems.Problem.as_cross(): operands q [contexts*qrep, D], kv [contexts, Tk, 2D],
        dout [contexts*qrep, D]; then (reference, bound) of out, dq [contexts*qrep, D] and dk, dv [contexts, Tk, D]."""
        D = self.heads * 64
        qrep = self.shape[1]
        rows = lambda x: x[:, :qrep].reshape(-1, D)                       # noqa: E731
        keys = lambda x: x[:, qrep:]                                      # noqa: E731
        kv = torch.cat([keys(self.pack(self.k)), keys(self.pack(self.v))], -1)
        res = {n: tuple((rows if n in ('out', 'dq') else keys)(x) for x in self.packed(n)) for n in NAMES}
        return rows(self.pack(self.q)), kv, rows(self.dout), res

    def as_mq(self):
        """The pooler's layout (attention_problems.Problem.as_mq()): q [B, NQ, H*64] (shared: [NQ, H*64]), kv [B, Tk, 128],
        dout [B, NQ, H*64]; (reference, bound) of out, dq (shared: summed over the clips, bound terms summed) and dk, dv."""
        B, NQ, H, Tk, shared = self.shape
        fold = lambda x: x[:, :NQ * H].reshape(B, NQ, H * 64)            # noqa: E731
        keys = lambda x: x[:, NQ * H:]                                    # noqa: E731
        q = fold(self.pack(self.q))
        res = {}
        for n in NAMES:
            ref, acc = self.pack(self.ref[n]), self.pack(self.acc[n])
            ref, acc = (fold(ref), fold(acc)) if n in ('out', 'dq') else (keys(ref), keys(acc))
            if shared and n == 'dq':
                ref, acc = ref.sum(0), acc.sum(0)
            res[n] = (ref, self.bound_of(ref, acc))
        kv = torch.cat([keys(self.pack(self.k)), keys(self.pack(self.v))], -1)
        return (q[0] if shared else q), kv, fold(self.dout), res


def _run(case_or_args, engine):
    """Runs `engine` on every block and scatters the per-block results into [B, H, T, ...] tensors (q-side results are
    assigned, k-side results summed over the blocks that hold the key)."""
    q, k, v, dO, blocks, vis = case_or_args
    B, H, T, _ = q.shape
    res = {}
    for qidx, kidx, causal in blocks:
        G, nq = qidx.shape
        nk = kidx.shape[1]
        m = torch.ones(1, 1, G, nq, nk, dtype=torch.bool)
        if causal:
            m = m & torch.ones(nq, nk, dtype=torch.bool).tril()
        if vis is not None:
            m = m & vis[:, kidx][:, None, :, None, :]
        r = engine(q[:, :, qidx], k[:, :, kidx], v[:, :, kidx], dO[:, :, qidx], m)
        fq, fk = qidx.reshape(-1), kidx.reshape(-1)
        for name, x in r.items():
            side = fk if name.endswith(('dk', 'dv')) else fq
            tail = x.shape[4:]
            if name not in res:
                res[name] = torch.zeros((B, H, T) + tail, dtype=x.dtype)
            res[name].index_add_(2, side, x.reshape((B, H, -1) + tail))
    return res


def emulate(case, fault=None):
    """The float32 (bf16 mode for bf16 cases) kernel model on a case: dict of out, lse, dq, dk, dv like case.ref."""
    bf = case.dtype == torch.bfloat16
    res = _run((case.q, case.k, case.v, case.dO, case.blocks, case.vis),
               lambda Q, K, V, dO, m: _block_emulation(Q, K, V, dO, m, bf, fault))
    if bf:
        res = {n: (x if n == 'lse' else x.to(torch.bfloat16)) for n, x in res.items()}
    return {n: x.double() for n, x in res.items()}


def ratios(case, got):
    """Worst err / bound per tensor; got: dict of [B, H, T, ...] tensors like case.ref. Non-finite values give inf."""
    rows = case.query_rows()
    out = {}
    for n in NAMES + ('lse',):
        ref = case.ref[n]
        bound = case.acc[n] + FLOOR + (0 if n == 'lse' else case.u * ref.abs())
        ratio = (got[n] - ref).abs() / bound
        ratio = torch.where(torch.isfinite(got[n]), ratio, torch.full_like(ratio, math.inf))
        if n in ('out', 'dq', 'lse'):
            ratio = ratio[:, :, rows]
        out[n] = ratio.max().item()
    return out


# ----------------------------------------------------------------------------------------------------------------------
# builders
# ----------------------------------------------------------------------------------------------------------------------
def _step(kind, slot):
    return slot if kind == 'time' else slot // 16


def _build(kind, shape, B, H, T, blocks, slot, dtype, stair, seed, vis=None, loud=False, shared_q=False):
    """slot [T]: position of every token in its key group (tokens that are no key: 0)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, T, 64, generator=g) * 1.5
    k = torch.randn(B, H, T, 64, generator=g) * 1.5
    v = torch.randn(B, H, T, 64, generator=g) * 1.5
    dO = torch.randn(B, H, T, 64, generator=g)
    q, k = _round(q, torch.bfloat16 if dtype == torch.float32 else dtype), _round(k, torch.bfloat16)
    v, dO = _round(v, dtype), _round(dO, dtype)
    b, h, i = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(T), indexing='ij')
    q[..., 63] = torch.tensor(PAL, dtype=torch.float64)[(7 * i + 3 * h + 5 * b) % 11]
    k[..., 63] = 8.0
    q[..., 62] = 8.0
    k[..., 62] = (stair * _step(kind, slot).double()).expand(B, H, T)
    if loud:
        top = torch.where(vis, k[:, 0, :, 62], torch.full((B, T), -math.inf, dtype=torch.float64)).max(-1).values
        top = torch.where(torch.isfinite(top), top, torch.zeros_like(top))
        k[..., 62] = torch.where(vis[:, None], k[..., 62], (top + LOUD)[:, None, None].expand(B, H, T))
    if shared_q:
        q = q[:1].expand(B, H, T, 64).contiguous()
    lanes = torch.cat([q[..., 62:], k[..., 62:]], -1)
    assert torch.equal(_round(lanes, torch.bfloat16), lanes), 'a lane value is not bf16-exact'
    u = U[dtype]
    res = _run((q, k, v, dO, blocks, vis), lambda Q, K, V, dOq, m: _block_reference(Q, K, V, dOq, m, u))
    ref = {n: res[n] for n in NAMES + ('lse',)}
    acc = {n: res['b_' + n] for n in NAMES + ('lse',)}
    return Case(kind, shape, H, dtype, stair, q, k, v, dO, blocks, vis, ref, acc)


def divided_case(B, F, N, H, mode, dtype, stair, seed=0):
    """Space (groups = frames) or time (groups = locations) attention over T = 1 + F N tokens; the cls query over all."""
    T = 1 + F * N
    G = F if mode == 'space' else N
    if mode == 'space':
        patches = 1 + torch.arange(F)[:, None] * N + torch.arange(N)[None]
    else:
        patches = 1 + torch.arange(F)[None, :] * N + torch.arange(N)[:, None]
    slots = torch.cat([torch.zeros(G, 1, dtype=torch.long), patches], 1)
    slot = torch.zeros(T, dtype=torch.long)
    slot[patches.reshape(-1)] = (1 + torch.arange(patches.shape[1])).expand(G, -1).reshape(-1)
    blocks = [(patches, slots, False), (torch.zeros(1, 1, dtype=torch.long), torch.arange(T)[None], False)]
    return _build(mode, (B, F, N, H), B, H, T, blocks, slot, dtype, stair, seed)


def causal_case(B, L, H, dtype, stair, seed=0):
    blocks = [(torch.arange(L)[None], torch.arange(L)[None], True)]
    return _build('causal', (B, L, H), B, H, L, blocks, torch.arange(L), dtype, stair, seed)


def cls_case(B, T, H, dtype, stair, seed=0):
    blocks = [(torch.zeros(1, 1, dtype=torch.long), torch.arange(T)[None], False)]
    return _build('cls', (B, T, H), B, H, T, blocks, torch.arange(T), dtype, stair, seed)


def _query_key_case(kind, shape, B, H, nq, Tk, dtype, stair, seed, shared_q=False):
    """nq query tokens (0..nq-1) over the Tk key tokens behind them."""
    blocks = [(torch.arange(nq)[None], nq + torch.arange(Tk)[None], False)]
    slot = torch.cat([torch.zeros(nq, dtype=torch.long), torch.arange(Tk)])
    return _build(kind, shape, B, H, nq + Tk, blocks, slot, dtype, stair, seed, shared_q=shared_q)


def cross_case(contexts, qrep, H, Tk, dtype, stair, seed=0):
    return _query_key_case('cross', (contexts, qrep, H, Tk), contexts, H, qrep, Tk, dtype, stair, seed)


def mq_case(B, NQ, H, Tk, shared, dtype, stair, seed=0):
    """The pooler: one 64-channel key / value head for all H query heads, a single-head problem with NQ * H queries."""
    return _query_key_case('mq', (B, NQ, H, Tk, bool(shared)), B, 1, NQ * H, Tk, dtype, stair, seed, shared_q=bool(shared))


RAGGED, EMPTY, HIDE_LOUD = 'ragged', 'empty', 'loud'
MASKS = (RAGGED, EMPTY, HIDE_LOUD)


def keymask(contexts, Tk, which):
    """[contexts, Tk] bool. RAGGED: prefixes of 1, Tk - 3 and Tk // 2 + 1 keys (in turn); EMPTY: the same with no visible
    key in context 1; HIDE_LOUD: holes -- key 0 of context 0 hidden, only the last key of the last context visible,
    elsewhere every third key and a run in the middle hidden."""
    m = torch.zeros(contexts, Tk, dtype=torch.bool)
    counts = (1, max(Tk - 3, 1), Tk // 2 + 1)
    if which in (RAGGED, EMPTY):
        for c in range(contexts):
            m[c, :counts[c % 3]] = True
        if which == EMPTY:
            m[1] = False
        return m
    j = torch.arange(Tk)
    m[:] = (j % 3 != 1) & ~((j >= Tk // 2) & (j < Tk // 2 + 9))
    m[0, 0] = False
    m[-1] = False
    m[-1, Tk - 1] = True
    return m


def keymask_case(contexts, Tk, H, which, dtype, stair, seed=0):
    """Self-attention of `contexts` samples of Tk tokens (qrep = Tk) under keymask(contexts, Tk, which)."""
    vis = keymask(contexts, Tk, which)
    blocks = [(torch.arange(Tk)[None], torch.arange(Tk)[None], False)]
    return _build('keymask', (contexts, Tk, H, which), contexts, H, Tk, blocks, torch.arange(Tk), dtype, stair, seed,
                  vis=vis, loud=which == HIDE_LOUD)


# ----------------------------------------------------------------------------------------------------------------------
# the shapes of tests/test_gpu_attention_shift.py (one list per kernel family; the CPU suite builds every one of them)
# ----------------------------------------------------------------------------------------------------------------------
BF, F32 = torch.bfloat16, torch.float32
SPACE_RESIDENT = [(2, 2, 31, 1), (2, 4, 32, 2), (2, 2, 64, 1), (1, 2, 196, 2), (1, 1, 287, 1)]       # (B, F, N, H)
SPACE_RESIDENT_273 = [(1, 1, 272, 1)]
SPACE_LARGE_RESIDENT = [(1, 1, 576, 1)]
SPACE_STREAM = [(1, 1, 288, 1), (1, 2, 576, 2), (1, 1, 640, 1)]
SPACE_STREAM_VARIANTS = (1, 2, 576, 2)
SPACE_STREAM_F32 = [(1, 1, 288, 1)]
TIME_REGISTER = [(2, 2, 3, 1), (2, 4, 9, 2), (1, 8, 9, 3), (1, 16, 9, 2)]
TIME_RIDERS = (2, 4, 9, 2)
TIME_MFMA = [(2, 5, 9, 4), (1, 12, 7, 8)]
TIME_GENERIC = [(2, 6, 5, 3)]
F32_GENERIC = [('space', (2, 2, 31, 1)), ('time', (2, 3, 7, 1))]
CAUSAL = [(2, 5, 2), (3, 77, 8), (2, 130, 2), (2, 256, 2), (2, 272, 2)]                             # (B, L, H)
CLS = [(2, 1, 2), (2, 99, 2), (2, 785, 2)]                                                          # (B, T, H)
CROSS_FWD_BF16 = [(2, 17, 1, 33), (1, 65, 2, 255), (2, 5, 3, 256), (2, 4, 2, 300), (2, 3, 2, 601), (3, 1, 2, 37)]
CROSS_FWD_F32 = [(2, 5, 2, 37), (2, 3, 1, 301)]                                                     # (contexts, qrep, H, Tk)
CROSS_BWD = [s for s in CROSS_FWD_BF16 if s[3] <= 256 and s[1] >= 2]
MQ = [(2, 5, 3, 9), (2, 24, 4, 65)]                                                                 # (B, NQ, H, Tk)
DECODE = [(2, 5, 2, 5), (2, 130, 2, 160)]                                                           # (B, L, H, capacity)
KEYMASK = [(BF, (3, 37, 2)), (BF, (3, 256, 1)), (BF, (3, 300, 1)), (F32, (3, 37, 2))]               # (contexts, Tk, H)


def all_cases():
    """(kind, shape, dtype) of every case the GPU tests build, each at every stair of STAIRS."""
    cases = []
    for s in SPACE_RESIDENT:
        cases += [('space', s, BF), ('space', s, F32)]
    cases += [('space', s, BF) for s in SPACE_RESIDENT_273 + SPACE_LARGE_RESIDENT + SPACE_STREAM]
    cases += [('space', s, F32) for s in SPACE_STREAM_F32]
    for s in TIME_REGISTER:
        cases += [('time', s, BF), ('time', s, F32)]
    cases += [('time', s, BF) for s in TIME_MFMA + TIME_GENERIC]
    cases += [(m, s, F32) for m, s in F32_GENERIC]
    for s in CAUSAL:
        cases += [('causal', s, BF), ('causal', s, F32)]
    for s in CLS:
        cases += [('cls', s, BF), ('cls', s, F32)]
    cases += [('cross', s, BF) for s in CROSS_FWD_BF16] + [('cross', s, F32) for s in CROSS_FWD_F32]
    for s in MQ:
        cases += [('mq', s + (sh,), dt) for sh in (False, True) for dt in (BF, F32)]
    for s in DECODE:
        cases += [('causal', s[:3], BF), ('causal', s[:3], F32)]
    for dt, s in KEYMASK:
        cases += [('keymask', s + (w,), dt) for w in MASKS]
    return list(dict.fromkeys(cases))


def row_shifts(kind, shape):
    """The palette entries of the case's query rows (what _build writes into q[..., 63] there), without building it."""
    if kind in ('space', 'time'):
        B, H, rows = shape[0], shape[3], range(1 + shape[1] * shape[2])
    elif kind == 'causal':
        B, H, rows = shape[0], shape[2], range(shape[1])
    elif kind == 'cls':
        B, H, rows = shape[0], shape[2], range(1)
    elif kind == 'cross':
        B, H, rows = shape[0], shape[2], range(shape[1])
    elif kind == 'mq':
        B, H, rows = (1 if shape[4] else shape[0]), 1, range(shape[1] * shape[2])
    else:
        B, H, rows = shape[0], shape[2], range(shape[1])
    return {PAL[(7 * i + 3 * h + 5 * b) % 11] for b in range(B) for h in range(H) for i in rows}


def group_keys(kind, shape):
    """Keys of a group of the case's first block (causal: of the last row)."""
    return {'space': lambda: shape[2] + 1, 'time': lambda: shape[1] + 1, 'causal': lambda: shape[1],
            'cls': lambda: shape[1], 'cross': lambda: shape[3], 'mq': lambda: shape[3], 'keymask': lambda: shape[1]}[kind]()


@functools.lru_cache(maxsize=None)
def make(kind, shape, dtype, stair, seed=0):
    if kind in ('space', 'time'):
        B, F, N, H = shape
        return divided_case(B, F, N, H, kind, dtype, stair, seed)
    if kind == 'causal':
        return causal_case(*shape, dtype=dtype, stair=stair, seed=seed)
    if kind == 'cross':
        return cross_case(*shape, dtype=dtype, stair=stair, seed=seed)
    if kind == 'mq':
        return mq_case(*shape, dtype=dtype, stair=stair, seed=seed)
    if kind == 'keymask':
        contexts, Tk, H, which = shape
        return keymask_case(contexts, Tk, H, which, dtype, stair, seed)
    return cls_case(*shape, dtype=dtype, stair=stair, seed=seed)
