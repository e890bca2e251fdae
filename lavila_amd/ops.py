"""autograd-aware wrappers around the C-ABI kernels (liblavila_hip.so).

Each `*_raw` function is a 1:1 call of one C entry point on torch device tensors; each
`torch.autograd.Function` pairs a forward kernel with its hand-written backward kernel so that the
reference's training loop (loss.backward(), DDP hooks, AdamW) works unchanged. Parameters
(gamma/beta/bias/embeddings) are always passed to the kernels as float32.
"""
import os
import weakref
from typing import Optional

import torch

from . import _cabi as C
from .ingest import PendingClip, refuse_pending


def _f32(p: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if p is None:
        return None
    p = p.detach()
    if p.dtype != torch.float32:
        p = p.float()
    return p.contiguous()




def _rows_cols(x: torch.Tensor):
    cols = x.shape[-1]
    return x.numel() // cols, cols


def autocast_dtype():
    """The activation dtype of an active autocast region, or None. The kernels compute in f32 or bf16: the reference
    drivers' fp16 autocast (`torch.cuda.amp.autocast()`, main_pretrain.py:490) means bf16 here."""
    if not torch.is_autocast_enabled():
        return None
    dt = torch.get_autocast_dtype('cuda')
    return torch.bfloat16 if dt == torch.float16 else dt


def lowp(x: torch.Tensor) -> torch.Tensor:
    """fp16 activations (model.half() + images.half(): eval_zeroshot.py:212-213,256-257,293-304) are computed in bf16;
    the model wrappers hand fp16 back to the caller."""
    return x.to(torch.bfloat16) if x.dtype == torch.float16 else x


def _act(x: torch.Tensor) -> torch.Tensor:
    """Activation entering a GEMM: f32 -> the autocast dtype when autocast is on, fp16 -> bf16."""
    if x.dtype == torch.float16:
        return x.to(torch.bfloat16)
    lp = autocast_dtype()
    return x.to(lp) if (lp is not None and x.dtype == torch.float32) else x


# --------------------------------------------------------------------------------------------------
# Linear layers: hand-written MFMA GEMMs (forward / input gradient: lvl_linear_tn, weight gradient: lvl_linear_wgrad)
# --------------------------------------------------------------------------------------------------
_warned = set()
_copies = {}          # (id(parameter), shape) -> (version, bf16 copy, transposed bf16 copy, data_ptr, generation)
_generation = 0       # bumped whenever parameter VALUES may have changed behind the version counter's back


def warn_once(key, msg):
    """One line per process when a bf16 call leaves the fast kernels (shape not tiled, generic attention, ...)."""
    if key not in _warned:
        _warned.add(key)
        import warnings
        warnings.warn('lavila_amd: ' + msg, stacklevel=3)


def invalidate_weight_cache():
    """Forget every cached bf16 weight copy (they are re-cast on their next use).

    The cache key (tensor version counter + storage pointer) does not see writes through `param.data`
    (ZeroRedundancyOptimizer's broadcast of updated shards into `param.data`, `logit_scale.data.clamp_`-style edits,
    bucket-view updates). Two automatic triggers cover the training loop: every optimizer step (a global
    `register_optimizer_step_post_hook`, installed on import) and the start of every grad-enabled model forward
    (`training_forward_begins`). Call this by hand after any other out-of-band write to a Linear weight."""
    global _generation
    _generation += 1


def training_forward_begins():
    """Called by the model wrappers (CLIP.forward / encode_*, SpaceTimeTransformer.forward*) at the top of a forward:
    with gradients enabled the copies are re-cast once per forward -- the same one lvl_cast_transpose pass per optimizer
    step as before, now independent of HOW the optimizer wrote the parameters -- and then shared by that forward, its
    backward and activation checkpointing's recomputation (which re-enters the blocks, not the wrappers)."""
    if torch.is_grad_enabled():
        invalidate_weight_cache()
        refresh_weight_copies()


_forward_depth = __import__('threading').local()


class model_forward:
    """`with ops.model_forward():` around a model-level forward (CLIP.forward / encode_*, SpaceTimeTransformer.forward*,
    VCLM_HF.encode_image): the OUTERMOST one of a grad-enabled forward bumps the weight-copy generation; nested ones
    (CLIP.forward -> encode_image -> visual.forward, the text tower started from inside the video forward) do not, so
    every weight is cast exactly once per training forward and activation checkpointing's recomputation finds the
    copies of its own forward."""

    def __enter__(self):
        d = getattr(_forward_depth, 'd', 0)
        if d == 0:
            training_forward_begins()
        _forward_depth.d = d + 1

    def __exit__(self, *exc):
        _forward_depth.d -= 1
        return False


def _optimizer_stepped(optimizer, args, kwargs):
    invalidate_weight_cache()


try:        # every torch.optim.Optimizer (ZeroRedundancyOptimizer included) announces its step() here
    from torch.optim.optimizer import register_optimizer_step_post_hook as _reg_post_hook
    _reg_post_hook(_optimizer_stepped)
except ImportError:         # older torch: the per-forward trigger alone
    pass


# float32 activations (the parity configuration, north_star "within 1e-3 fp32"): the SAME MFMA GEMM kernels in their
# f32-class mode -- operands as bf16 term images (split3 / lvl_split_bf16x3), float32 results; ~2^-17 relative per
# product instead of bf16's 2^-9. LAVILA_F32_MFMA=0 sends float32 Linears to the library GEMM instead (A/B only).
F32_MFMA = os.environ.get('LAVILA_F32_MFMA', '1') != '0'


def split3(x2: torch.Tensor, role: int, stack: bool = False) -> torch.Tensor:
    """float32 [R, C] -> its three bf16 term images (h, h, l) (role 0: the x / dy side of a product) or (h, l, h)
    (role 1: the w / x side): side by side along the contraction, [R, 3C] (operand of lvl_linear_tn's f32-class mode),
    or -- stack=True -- one under the other, [3*Rp, C] (operands of lvl_linear_wgrad, which contracts over rows; rows
    padded with zeros so that the kernel sees at least one 32-row step)."""
    C.require_device(x2)
    R, Cc = x2.shape
    if stack:
        Rp = max(R, 11)
        out = (torch.zeros if Rp != R else torch.empty)(3 * Rp, Cc, dtype=torch.bfloat16, device=x2.device)
        rs, ts = Cc, Rp * Cc
    else:
        out = torch.empty(R, 3 * Cc, dtype=torch.bfloat16, device=x2.device)
        rs, ts = 3 * Cc, Cc
    C.check(C.lib().lvl_split_bf16x3(C.ptr(x2), C.ptr(out), R, Cc, Cc, rs, ts, role, C.stream_ptr()), 'lvl_split_bf16x3')
    return out


def _split_pair(src):
    src = src.float().contiguous()
    return split3(src, 1), split3(src.t().contiguous(), 1)


def _cast_pair(src):
    if src.dtype == torch.float32 and src.is_contiguous():
        w = torch.empty_like(src, dtype=torch.bfloat16)
        wt = torch.empty(src.shape[1], src.shape[0], dtype=torch.bfloat16, device=src.device)
        C.check(C.lib().lvl_cast_transpose(C.ptr(src), C.ptr(w), C.ptr(wt), src.shape[0], src.shape[1], C.stream_ptr()),
                'lvl_cast_transpose')
    else:                   # fp16 parameters (model.half(), eval_zeroshot.py --use-half) and views
        w = src.to(torch.bfloat16).contiguous()
        wt = w.t().contiguous()
    return w, wt


def weight_copies(weight: torch.Tensor, f32: bool = False):
    """f32=True: the f32-class operands instead -- (w3 [out, 3 in], wt3 [in, 3 out]) term images of the weight and of its
    transpose (split3 role 1) -- cached under the same rules.
    (w, wt): the bf16 copy [out,in] the forward GEMM reads and the transposed bf16 copy [in,out] the input-gradient
    GEMM reads (both operands of lvl_linear_tn are contraction-contiguous). One lvl_cast_transpose pass per optimizer
    step: the pair is cached per parameter and keyed by (version counter, storage pointer, cache generation), so
    activation checkpointing's second forward and every backward reuse it; see invalidate_weight_cache for what bumps
    the generation. Under hipGraph capture the cache is bypassed: the cast is recorded INTO the graph (into
    graph-owned buffers), so a replay after a weight update reads the updated weights."""
    src = weight.detach()
    make = _split_pair if f32 else _cast_pair
    if src.is_cuda and torch.cuda.is_current_stream_capturing():
        return make(src)
    # keyed by the identity of the parameter (a 2-D view of one -- the Conv2d weight of the patch embedding -- keys on
    # its base); a weakref finaliser drops the entry with the parameter, nothing is attached to the parameter itself
    # (pickling / deepcopy of the model see no extra state)
    holder = weight._base if weight._base is not None else weight
    ver, key = weight._version, (id(holder), tuple(weight.shape), tuple(weight.stride()), f32)
    c = _copies.get(key)
    if c is not None and c[0] == ver and c[3] == weight.data_ptr() and c[4] == _generation:
        return c[1], c[2]
    if c is None:
        weakref.finalize(holder, _copies.pop, key, None)
    w, wt = make(src)
    # (the parameter itself, weakly, when it is one -- refresh_weight_copies re-casts those entries in one launch)
    _copies[key] = (ver, w, wt, weight.data_ptr(), _generation, weakref.ref(weight) if weight._base is None else None)
    return w, wt


# LAVILA_WEIGHT_REFRESH=1: every stale weight copy is re-cast by ONE launch at the top of the training forward instead of one
# lvl_cast_transpose launch per weight at its first use. Off by default: measured neutral to slightly slower (same box,
# alternating: 163.86 ms per step lazily, 164.21 with the refresh -- the ~120 five-microsecond launches already hide between the
# step's kernels, the single 0.3-ms pass at the top does not; profiles/r06_weight_refresh.txt).
WEIGHT_REFRESH = os.environ.get('LAVILA_WEIGHT_REFRESH', '0') == '1'


def refresh_weight_copies():
    """Re-cast, in ONE lvl_cast_transpose_multi launch per device, every cached (bf16, transposed bf16) pair that the new
    cache generation made stale. Called at the top of a grad-enabled model forward (training_forward_begins), i.e. exactly
    where the first use of each weight would otherwise re-cast it: the same values at the same point of the step, 1 launch
    instead of ~120 (main_pretrain.py:520-533: optimizer.step(), then the next model(...)). Entries whose parameter is gone,
    moved, not float32-contiguous, a view (the patch embedding's reshaped Conv2d weight) or an f32-class image pair keep the
    lazy path; so does everything under hipGraph capture."""
    if not WEIGHT_REFRESH or not _copies or not torch.cuda.is_available() or torch.cuda.is_current_stream_capturing():
        return
    by_dev = {}
    for key, c in list(_copies.items()):
        if key[3] or len(c) < 6 or c[5] is None or c[4] < _generation - 3:      # (not used by the last step: lazily)
            continue
        w = c[5]()
        if (w is None or not w.is_cuda or w.dtype != torch.float32 or w.dim() != 2 or not w.is_contiguous()
                or w.data_ptr() != c[3]):
            continue
        by_dev.setdefault(w.device, []).append((key, w))
    for dev, items in by_dev.items():
        if len(items) < 2 or dev != torch.device('cuda', torch.cuda.current_device()):
            continue
        rows, outs, tile0 = [], [], 0
        for key, w in items:
            src = w.detach()
            n, k = src.shape
            a = torch.empty_like(src, dtype=torch.bfloat16)
            b = torch.empty(k, n, dtype=torch.bfloat16, device=dev)
            rows.append([src.data_ptr(), a.data_ptr(), b.data_ptr(), n | (k << 32), tile0])
            tile0 += ((n + 63) // 64) * ((k + 63) // 64)
            outs.append((key, w, a, b))
        table = torch.tensor(rows, dtype=torch.int64, device=dev)
        C.check(C.lib().lvl_cast_transpose_multi(C.ptr(table), len(rows), tile0, C.stream_ptr()), 'lvl_cast_transpose_multi')
        for key, w, a, b in outs:
            _copies[key] = (w._version, a, b, w.data_ptr(), _generation, weakref.ref(w))


def _tn_ok(rows: int, n_out: int, n_in: int) -> bool:
    """lvl_linear_tn tiles N in 256s and K in 64s (every width of the CLIP_OPENAI_TIMESFORMER_* towers)."""
    return rows > 0 and n_out % 256 == 0 and n_in % 64 == 0 and rows * max(n_in, n_out) * 2 < (1 << 32)


def _tn_ragged_ok(rows: int, n_out: int, n_in: int) -> bool:
    """lvl_linear_tn_ragged: plain GEMM (+ bias) for N in 64s -- the full 256-column tiles on lvl_linear_tn's kernel, the
    64 / 128 / 192 columns behind them on the edge kernel (the 1600 / 3200 / 4800 of the GPT-2 XL narrators' decoder).
    Callers ask _tn_ok first: where it holds, lvl_linear_tn runs exactly as before.
    Both widths must reach one full tile (256): the entry point itself serves N = 64 / 128 / 192 too, but a decoder narrower
    than that is no published model, and the 192-wide narrator of the golden fixtures keeps the routing (library GEMMs) its
    recorded gradients were checked on -- a single gate's gradient there sits within rounding noise of its per-tensor bar."""
    return (rows > 0 and n_out % 64 == 0 and n_in % 64 == 0 and min(n_out, n_in) >= 256
            and rows * max(n_in, n_out) * 2 < (1 << 32))


def _wgrad(dy2, x2, wdt):
    """dW = dy^T x: the MFMA weight-gradient kernel; shapes it does not tile fall back to a library GEMM (logged)."""
    rows, n_out, n_in = dy2.shape[0], dy2.shape[1], x2.shape[1]
    ws_floats = -1
    if (rows > 0 and dy2.dtype == torch.bfloat16 and x2.dtype == torch.bfloat16 and dy2.is_contiguous()
            and x2.is_contiguous() and dy2.is_cuda):
        ws_floats = C.lib().lvl_workspace_floats(b'linear_wgrad', n_out, n_in)
    if ws_floats >= 0:
        if rows < 32:       # the class-token / EOT-row Linears of a small batch: zero rows up to the kernel's one 32-row step
            dy2 = torch.cat([dy2, dy2.new_zeros(32 - rows, n_out)])
            x2 = torch.cat([x2, x2.new_zeros(32 - rows, n_in)])
        return linear_wgrad_raw(dy2, x2, False, int(ws_floats))[0].to(wdt)
    if dy2.dtype == torch.bfloat16 and rows >= 4096:
        warn_once(('wgrad', n_out, n_in), f'weight gradient [{n_out},{n_in}] falls back to a library GEMM '
                                          '(lvl_linear_wgrad tiles multiples of 192/288/384, 128/256 or 160/320)')
    return (dy2.t() @ x2).to(wdt)


def _wgrad_f32(dy2, x2, wdt):
    """dW = dy^T x for float32 operands: lvl_linear_wgrad on row-stacked term images (f32-class, see split3)."""
    n_out, n_in = dy2.shape[1], x2.shape[1]
    ws_floats = C.lib().lvl_workspace_floats(b'linear_wgrad', n_out, n_in) if (F32_MFMA and dy2.is_cuda) else -1
    if ws_floats < 0 or not _wgrad_f32_ok(dy2.shape[0], n_out, n_in):
        return (dy2.t() @ x2).to(wdt)
    dy2 = dy2 if dy2.is_contiguous() else dy2.contiguous()
    x2 = x2 if x2.is_contiguous() else x2.contiguous()
    return linear_wgrad_raw(split3(dy2, 0, stack=True), split3(x2, 1, stack=True), False, int(ws_floats))[0].to(wdt)


def _tn_ok_f32(rows: int, n_out: int, n_in: int) -> bool:
    return F32_MFMA and _tn_ok(rows, n_out, 3 * n_in)


def _wgrad_f32_ok(rows: int, n_out: int, n_in: int) -> bool:
    """The size gate of _wgrad_f32: the row-stacked term images (3 x rows of bf16) of both operands stay below 4 GiB.
    lvl_linear_wgrad itself has no such limit (64-bit row pointers; DESIGN.md, "Operand-size limits"): the gate keeps the
    float32 path inside what the suite runs."""
    return rows * max(n_in, n_out) * 6 < (1 << 32)


def _skinny_ok(rows: int, n_out: int, n_in: int) -> bool:
    """Inference Linears that lvl_linear_tn does not tile go to lvl_linear_skinny: operands below 2 GiB."""
    return (rows > 0 and not _tn_ok(rows, n_out, n_in) and n_out % 16 == 0 and n_in % 64 == 0
            and rows * max(n_in, n_out) * 2 < (1 << 31))


def _skinny_f32_ok(rows: int, n_out: int, n_in: int) -> bool:
    """The same for float32 rows on lvl_linear_skinny_f32c (term images of 3 x n_in, float32 output): below 2 GiB."""
    return (rows > 0 and not _tn_ok_f32(rows, n_out, n_in) and n_out % 16 == 0 and n_in % 32 == 0
            and rows * max(3 * n_in, n_out) * 4 < (1 << 31))


# --------------------------------------------------------------------------------------------------
# Activation checkpointing modes (the `use_checkpoint` argument of the model wrappers)
# --------------------------------------------------------------------------------------------------
# What `use_checkpoint=True` means: 'block' (torch.utils.checkpoint around every block of the video tower / the text tower)
# or 'selective' (see checkpoint_mode). The reference's drivers pass a bool (main_pretrain.py --use-checkpoint), so this is how
# they reach the selective mode.
CHECKPOINT = os.environ.get('LAVILA_CHECKPOINT', 'block')
CHECKPOINT_MODES = ('block', 'selective')


def checkpoint_mode(use_checkpoint):
    """The one place that decides what a `use_checkpoint` argument means: None (keep every activation), 'block' (re-run the
    whole block in backward) or 'selective'.

    False / None -> None; 'block' / 'selective' -> themselves; True -> LAVILA_CHECKPOINT (ops.CHECKPOINT), 'block' by
    default. Anything else, as the argument or in the variable, raises ValueError.

    'selective' runs the video tower's blocks as the plain step does but keeps neither the three LayerNorm outputs of a
    block nor its MLP hidden activation (7 of the 22 [tokens, D] units a block keeps); each is rebuilt elementwise
    (lvl_layernorm_apply / lvl_quickgelu_apply) right before the weight-gradient GEMM that reads it. No GEMM and no
    attention kernel runs twice. The text tower runs its plain path under 'selective'."""
    if use_checkpoint is None or use_checkpoint is False:
        return None
    mode = CHECKPOINT if use_checkpoint is True else use_checkpoint
    if isinstance(mode, str) and mode in CHECKPOINT_MODES:
        return mode
    if use_checkpoint is True:
        raise ValueError(f'LAVILA_CHECKPOINT={mode!r}: expected one of {CHECKPOINT_MODES}')
    raise ValueError(f'use_checkpoint={use_checkpoint!r}: expected False, None, True or one of {CHECKPOINT_MODES}')


class LnRecipe:
    """What a LayerNorm output h is rebuilt from (selective activation recompute): the operands the LayerNorm function keeps
    for its own backward anyway -- the input as x, or x + x2 + xbias summed in the forward's order -- with mean, rstd,
    gamma, and beta. The LayerNorm function fills it, the caller hands it to the Linear that consumes h (`ln=`), and that
    Linear saves these tensors (through save_for_backward) instead of h."""

    __slots__ = ('x', 'x2', 'xbias', 'gamma', 'beta', 'mean', 'rstd', 'dtype')

    def fill(self, x, x2, xbias, gamma, beta, mean, rstd):
        d = lambda t: None if t is None else t.detach()
        self.x, self.x2, self.xbias, self.gamma, self.beta = d(x), d(x2), d(xbias), d(gamma), d(beta)
        self.mean, self.rstd, self.dtype = mean, rstd, x.dtype

    def saved(self):
        return self.x, self.x2, self.xbias, self.gamma, self.beta, self.mean, self.rstd


def _ln_for(ln, x):
    """The recipe when `x` is the kernel's own output (same dtype: no cast between the LayerNorm and the Linear), else None:
    the Linear then keeps x itself."""
    return ln if (ln is not None and ln.dtype == x.dtype) else None


def _ln_rebuild(saved, shape):
    x, x2, xbias, gamma, beta, mean, rstd = saved
    return layernorm_apply_raw(x, x2, xbias, gamma, beta, mean, rstd).reshape(shape)


# The Linear layers' routing rule, GEMM and backward, shared by _LinearFn, _LinearTokenFn, the fused MLP and LayerNorm forms
# below, and the decoder's and the classifier's Functions (gpt2_gated.py, models.py).
OWN_BF16, OWN_F32 = 'bf16', 'f32'       # what _route answers; None: the library GEMM


def _route(x, rows, n_out, n_in, want_dx=True, ragged=(False, False)):
    """Which GEMMs run a Linear [n_in -> n_out] on `rows` rows of the activation x: OWN_BF16 (lvl_linear_tn), OWN_F32 (its
    f32-class mode) or None (the library). The forward must tile, and the input gradient -- N and K swapped -- too if it is
    wanted. ragged = (forward, input gradient): lvl_linear_tn_ragged may serve that direction (the bf16 layers that say so
    have no f32-class mode)."""
    if x.is_cuda and x.dtype == torch.bfloat16:
        mode, (fwd, bwd) = OWN_BF16, ((_tn_rows_ok if r else _tn_ok) for r in ragged)
    elif x.is_cuda and x.dtype == torch.float32 and not any(ragged):
        mode, fwd, bwd = OWN_F32, _tn_ok_f32, _tn_ok_f32
    else:
        return None
    return mode if fwd(rows, n_out, n_in) and (not want_dx or bwd(rows, n_in, n_out)) else None


def _gemm(mode, x2, w, bias=None, epilogue=C.EPI_BIAS, aux_in=None, ragged=False):
    """One own GEMM of a Linear in `mode` (_route) on contiguous rows x2: lvl_linear_tn, in OWN_F32 on the term images of x2
    against the term images w (weight_copies(f32=True)); ragged: the entry linear_tn_rows picks by the shape."""
    if mode == OWN_F32:
        return linear_tn_raw(split3(x2, 0), w, bias, epilogue, aux_in=aux_in, f32=True)
    if ragged:
        return linear_tn_rows(x2, w, bias)
    return linear_tn_raw(x2, w, bias, epilogue, aux_in=aux_in)


def _linear_backward(need, dy2, x2, wt, mode, wdt, bdt=None, recipe=None, ragged=False, swap=False):
    """(dx, dw, db) of y = x W^T (+ b) for the gradient dy2 [rows, out] (contiguous). need: needs_input_grad of (x, W, b).
    dx = dy2 wt^T on the own GEMMs (`mode`, `ragged`: as _gemm) or, mode None, the library's; wt [in, out] is the transposed
    weight copy. dw = dy2^T x2 on lvl_linear_wgrad (swap: x2^T dy2, the Conv1D layout) with x2 the kept rows or, recipe (the
    saved tensors of an LnRecipe), rebuilt right before this GEMM, their only reader, and only if dw is wanted. db (bdt: the
    bias dtype, None: no bias): float32 column sums of dy2."""
    if mode == OWN_F32:
        dy2 = dy2.float()
    dx = dw = db = None
    if need[0]:
        dx = _gemm(mode, dy2, wt, ragged=ragged) if mode else dy2 @ wt.t()
    if need[1]:
        if recipe is not None:
            x2 = _ln_rebuild(recipe, (-1, wt.shape[0]))
        wgrad = _wgrad_f32 if x2.dtype == torch.float32 else _wgrad
        dw = wgrad(x2, dy2, wdt) if swap else wgrad(dy2, x2, wdt)
    if bdt is not None and need[2]:
        db = dy2.sum(0, dtype=torch.float32).to(bdt)      # f32 accumulation AND f32 result
    return dx, dw, db


class _LinearFn(torch.autograd.Function):
    """y = x W^T (+ b) for token-major activations [rows, in].

    bf16: forward and input gradient are lvl_linear_tn calls (the input gradient multiplies by the cached transposed
    weight copy, so both GEMMs read contraction-contiguous operands), the weight gradient is lvl_linear_wgrad. f32
    (the parity configuration): the same three kernels in f32-class mode (bf16 term images in, float32 out: split3).
    Widths the kernels do not tile use the library GEMM.
    ln (an LnRecipe): x is a LayerNorm output that is not to be kept; the recipe's tensors are saved in its place and x is
    rebuilt right before the weight-gradient GEMM, its only reader in backward."""

    @staticmethod
    def forward(ctx, x, weight, bias, ln=None):
        x2 = x.reshape(-1, x.shape[-1])
        rows, n_in, n_out = x2.shape[0], x2.shape[1], weight.shape[0]
        mode = ctx.mode = _route(x, rows, n_out, n_in, ctx.needs_input_grad[0])
        ctx.meta = (weight.dtype, None if bias is None else bias.dtype, x.shape)
        ctx.ln = ln is not None
        if mode:
            w, wt = weight_copies(weight, mode == OWN_F32)
            x2 = x2 if x2.is_contiguous() else x2.contiguous()
            ctx.save_for_backward(*(ln.saved() if ctx.ln else (x2,)), wt)
            return _gemm(mode, x2, w, _f32(bias)).reshape(*x.shape[:-1], n_out)
        if x.dtype == torch.bfloat16 and rows >= 4096:
            warn_once(('linear', n_out, n_in), f'Linear [{n_out},{n_in}] runs on the library GEMM (lvl_linear_tn needs '
                                               'out % 256 == 0 and in % 64 == 0)')
        w = weight if weight.dtype == x.dtype else weight.to(x.dtype)
        b = None if bias is None else (bias if bias.dtype == x.dtype else bias.to(x.dtype))
        ctx.save_for_backward(*(ln.saved() if ctx.ln else (x2,)), w)
        with torch.autocast('cuda', enabled=False):
            return torch.nn.functional.linear(x, w, b)

    @staticmethod
    def backward(ctx, dy):
        *kept, w = ctx.saved_tensors              # own modes: w is the TRANSPOSED copy [in, out]
        wdt, bdt, xshape = ctx.meta
        dy2 = dy.reshape(-1, dy.shape[-1])
        if not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        with torch.autocast('cuda', enabled=False):
            dx, dw, db = _linear_backward(ctx.needs_input_grad, dy2, None if ctx.ln else kept[0], w if ctx.mode else w.t(),
                                          ctx.mode, wdt, bdt, recipe=kept if ctx.ln else None)
        return None if dx is None else dx.reshape(xshape), dw, db, None


# The activations of the fused MLP: the epilogues of lvl_linear_tn that apply them (keeping u / keeping act'(u) / the backward
# on a kept u) and the kernel that rebuilds the hidden activation from a kept u (selective recompute). The bf16 backward on a
# kept DERIVATIVE is LVL_EPI_MUL_AUX_COLSUM for both.
ACT_QUICKGELU, ACT_GELU = 'quickgelu', 'gelu'
_MLP_EPILOGUES = {act: tuple(C.TN_EPILOGUES[name.format(act.upper())][0] for name in ('EPI_BIAS_{}', 'EPI_BIAS_{}_DERIV', 'EPI_{}_BWD'))
                  for act in (ACT_QUICKGELU, ACT_GELU)}


def _mlp_epilogues(act):
    if act not in _MLP_EPILOGUES:
        raise ValueError(f'act={act!r}: the fused MLP takes {ACT_QUICKGELU!r} (x * sigmoid(1.702 x)) or {ACT_GELU!r} (the exact '
                         'erf GELU, nn.GELU())')
    return _MLP_EPILOGUES[act]


def gelu_apply_raw(u):
    """a = GELU(u) (exact, erf) with the arithmetic of linear_tn_raw's EPI_BIAS_GELU epilogue (lvl_act_fwd,
    LVL_ACT_GELU_ERF): rebuilds the hidden activation from the kept pre-activation to the bit."""
    C.require_device(u)
    a = torch.empty_like(u)
    C.check(C.lib().lvl_act_fwd(C.ptr(u), C.ptr(a), u.numel(), C.ACT_GELU_ERF, C.dtype_code(u), C.stream_ptr()), 'lvl_act_fwd')
    return a


class _MlpFn(torch.autograd.Function):
    """y = fc2(act(fc1(x) + b1)), act = QuickGELU or the exact GELU (`act`), without fc2's bias (the caller leaves it pending for the next fused
    residual + LayerNorm): timesformer.py:52-58 / openai_model.py:189-192. Two lvl_linear_tn calls forward (the
    first one adds the bias, applies the activation and keeps what the backward needs), and in backward the QuickGELU
    derivative and the fc1 bias gradient are the epilogue of fc2's input-gradient GEMM: the [rows, 4D] tensors are
    touched by GEMM epilogues only. What is kept: bf16 keeps quickgelu'(u) itself -- the forward epilogue has
    sigmoid(1.702 u) in a register, the backward epilogue then is one multiply (LVL_EPI_BIAS_QUICKGELU_DERIV /
    LVL_EPI_MUL_AUX_COLSUM); the f32-class mode keeps the pre-activation u (LVL_EPI_BIAS_QUICKGELU /
    LVL_EPI_QUICKGELU_BWD). The exact GELU runs the same way on its own epilogues (LVL_EPI_BIAS_GELU_DERIV, whose one erf
    serves gelu(u) and gelu'(u), then LVL_EPI_MUL_AUX_COLSUM; LVL_EPI_BIAS_GELU / LVL_EPI_GELU_BWD where u is kept)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, ln=None, act=ACT_QUICKGELU):
        y, saved = _mlp_forward(ctx, x, w1, b1, w2, ln, act)
        ctx.save_for_backward(*saved)
        ctx.meta = (w1.dtype, None if b1 is None else b1.dtype, w2.dtype, x.shape)
        return y.reshape(*x.shape[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dy):
        if ctx.sel:
            *kept, u, w1t, w2t = ctx.saved_tensors
            x2 = a = None
        else:
            x2, u, a, w1t, w2t = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        if not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        if ctx.mode == OWN_F32:
            dy2 = dy2.float()
        dx, dw1, db1, dw2 = _mlp_backward(ctx, dy2, x2, u, a, w1t, w2t, kept if ctx.sel else None)
        return dx, dw1, db1, dw2, None, None


def _mlp_forward(ctx, x, w1, b1, w2, ln, act, b2=None, res2=None):
    """The two GEMMs of fc2(act(fc1(x) + b1)) shared by _MlpFn and _MlpResidualLayerNormFn (res2: the residual rows fc2 adds
    in its epilogue, with its bias b2): (fc2's output, what backward keeps of them -- the head of save_for_backward).
    ctx.mode: bf16, or the f32-class mode (term images in, float32 u / a / y); ctx.sel: selective recompute (ln, the
    LnRecipe of x): keep u, neither x (a LayerNorm output) nor a."""
    x2 = x.reshape(-1, x.shape[-1])
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    mode = ctx.mode = OWN_F32 if x.dtype == torch.float32 else OWN_BF16
    sel = ctx.sel = ln is not None
    ctx.act = act
    keep_u, keep_deriv, _ = _mlp_epilogues(act)
    w1b, w1t = weight_copies(w1, mode == OWN_F32)
    w2b, w2t = weight_copies(w2, mode == OWN_F32)
    a, u = _gemm(mode, x2, w1b, _f32(b1), keep_u if (mode == OWN_F32 or sel) else keep_deriv)
    y = _gemm(mode, a, w2b, _f32(b2), C.EPI_BIAS if res2 is None else C.EPI_BIAS_RESIDUAL, aux_in=res2)
    return y, ((*ln.saved(), u, w1t, w2t) if sel else (x2, u, a, w1t, w2t))


def _mlp_backward(ctx, dy2, x2, u, a, w1t, w2t, kept, need=(0, 1, 2, 3)):
    """The backward of fc2(act(fc1(x) + b1)) (ctx.act) shared by _MlpFn and _MlpResidualLayerNormFn: (dx, dw1, db1, dw2) for
    the gradient dy2 [rows, D] of fc2's output. need: positions of x, w1, b1, w2 among the Function's inputs.
    Plain: x2 and a were kept; u is act'(u) in bf16 (one multiply in the epilogue) and the pre-activation in f32.
    Selective (ctx.sel): u is the pre-activation in both; a = act(u) and then x = the LayerNorm output of the recipe
    `kept` are rebuilt one after the other, each right before the weight-gradient GEMM that reads it and only if that
    gradient is wanted, so that at most one [rows, 4D] and one [rows, D] rebuilt tensor are alive at a time."""
    w1dt, b1dt, w2dt, xshape = ctx.meta[0], ctx.meta[1], ctx.meta[2], ctx.meta[-1]
    mode, sel = ctx.mode, ctx.sel
    gx, gw1, gb1, gw2 = (ctx.needs_input_grad[i] for i in need)
    bwd_on_u = _mlp_epilogues(ctx.act)[2]
    du, db1 = _gemm(mode, dy2, w2t, None, bwd_on_u if (mode == OWN_F32 or sel) else C.EPI_MUL_AUX_COLSUM, aux_in=u)
    dw2 = None
    if gw2:
        if sel:
            a = quickgelu_apply_raw(u) if ctx.act == ACT_QUICKGELU else gelu_apply_raw(u)
        dw2 = (_wgrad_f32 if mode == OWN_F32 else _wgrad)(dy2, a, w2dt)
    del a, u
    dx, dw1, _ = _linear_backward((gx, gw1, False), du, x2, w1t, mode, w1dt, recipe=kept)      # fc1: db1 left the epilogue above
    return (None if dx is None else dx.reshape(xshape), dw1, (db1.to(b1dt) if (b1dt is not None and gb1) else None), dw2)


def _mlp_fused_ok(x, w1, b1, w2):
    """Whether _MlpFn takes the MLP: both Linears, forward and input gradient, on the own kernels (bf16, or float32 on their
    f32-class mode)."""
    rows = x.numel() // x.shape[-1]
    if b1 is None or (x.dtype == torch.float32 and w1.dtype != torch.float32):
        return False
    return _route(x, rows, *w1.shape) is not None and _route(x, rows, *w2.shape) is not None


def mlp(x, w1, b1, w2, act, ln=None):
    """fc2(act(fc1(x))) minus fc2's bias for act = ACT_QUICKGELU or ACT_GELU, the exact erf GELU of nn.GELU(): fused GEMM
    epilogues (bf16 and f32-class), and where the fused form does not take the shapes or dtypes, the composed form: Linear,
    the activation (bias_quick_gelu / a torch op), Linear.
    ln: the LnRecipe of x (selective activation recompute: neither x nor the hidden activation is kept by the fused
    function; the composed form keeps the hidden activation and rebuilds x only)."""
    _mlp_epilogues(act)
    x = _act(x)
    ln = _ln_for(ln, x)
    if _mlp_fused_ok(x, w1, b1, w2):
        return _MlpFn.apply(x, w1, b1, w2, ln, act)      # bf16, or the same fused epilogues in f32-class mode
    if act == ACT_QUICKGELU:
        return linear(bias_quick_gelu(linear(x, w1, ln=ln), b1), w2)
    return linear(torch.nn.functional.gelu(linear(x, w1, b1, ln=ln)), w2)


def mlp_quickgelu(x, w1, b1, w2, ln=None):
    """mlp with ACT_QUICKGELU (the models' call)."""
    return mlp(x, w1, b1, w2, ACT_QUICKGELU, ln=ln)


def linear_wgrad_raw(dy, x, want_dbias: bool, ws_floats: int = -1):
    """dW [N,K] f32 = dy[M,N]^T x[M,K] (+ dbias [N] f32) through lvl_linear_wgrad (bf16 operands)."""
    C.require_device(dy, x)
    M, N = dy.shape
    K = x.shape[1]
    if ws_floats < 0:
        ws_floats = C.lib().lvl_workspace_floats(b'linear_wgrad', N, K)
        if ws_floats < 0:
            raise C.HipExtensionError(f'lvl_linear_wgrad: no tiling for N={N} K={K}')
    ws = torch.empty(int(ws_floats), dtype=torch.float32, device=dy.device)
    dw = torch.empty(N, K, dtype=torch.float32, device=dy.device)
    db = torch.empty(N, dtype=torch.float32, device=dy.device) if want_dbias else None
    C.check(C.lib().lvl_linear_wgrad(C.ptr(dy), C.ptr(x), C.ptr(dw), C.ptr(db), C.ptr(ws),
                                     C.ptr(sched_block(dy.device, 1024)), M, N, K, C.dtype_code(dy), C.stream_ptr()),
            'lvl_linear_wgrad')
    return dw, db


# Tile-counter blocks of the persistent GEMM (lvl_linear_tn `sched`): 16 x uint32, zero on entry, zeroed again by the
# kernel's last workgroup. One zero-filled pool per (device, stream), handed out round-robin: launches of one stream
# run in order, so a block is long back to zero when its turn comes again (4096 launches later), and the two towers'
# streams never share a block. Under hipGraph capture the block is allocated (and zeroed) inside the graph.
# lvl_linear_wgrad's chunk-counter blocks (1024 words) come from a second pool of the same kind.
_SCHED_BLOCKS = {16: 4096, 1024: 512}
_sched_pools = {}
# LAVILA_DYNAMIC_TILES: '1' always, '0' never, unset = when this process is one rank of a multi-GPU job (an initialised
# torch.distributed group of more than one rank: RCCL's channel kernels then share the GPU with the step -- that is
# the situation the counters are for; measured with 16 CUs held by another kernel: -5..8 % instead of -26..30 %,
# profiles/r03_cu_contention.txt). A single-GPU run keeps the static ranges: the counters cost 0.8 % of the step
# (the one synchronous hand-out per launch and the claims' round trips).
DYNAMIC_TILES = {'1': True, '0': False}.get(os.environ.get('LAVILA_DYNAMIC_TILES', ''), None)


def dynamic_tiles() -> bool:
    if DYNAMIC_TILES is not None:
        return DYNAMIC_TILES
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


def sched_block(device, words=16):
    if not dynamic_tiles():
        return None
    if torch.cuda.is_current_stream_capturing():
        return torch.zeros(words, dtype=torch.int32, device=device)
    key = (device, torch.cuda.current_stream(device).cuda_stream, words)
    pool = _sched_pools.get(key)
    if pool is None:
        pool = _sched_pools[key] = [torch.zeros(_SCHED_BLOCKS[words], words, dtype=torch.int32, device=device), 0]
    pool[1] = (pool[1] + 1) % _SCHED_BLOCKS[words]
    return pool[0][pool[1]]


_TN_TWO_OUT = tuple(code for code, two_out, _, _ in C.TN_EPILOGUES.values() if two_out)      # write aux_out
_TN_COLSUM = tuple(code for code, _, colsum, _ in C.TN_EPILOGUES.values() if colsum)        # read aux_in, leave column sums


def linear_tn_raw(x, w, bias=None, epilogue=C.EPI_BIAS, aux_in=None, f32=False):
    """One lvl_linear_tn call on bf16 tensors: y[M,N] = epilogue(x[M,K] . w[N,K]^T).
    Returns y (EPI_BIAS; EPI_BIAS_RESIDUAL: + aux_in [M,N]), (y, u) (EPI_BIAS_QUICKGELU, EPI_BIAS_GELU), (y, act'(u))
    (EPI_BIAS_QUICKGELU_DERIV, EPI_BIAS_GELU_DERIV) or (y, colsum) (EPI_QUICKGELU_BWD, EPI_GELU_BWD, EPI_MUL_AUX_COLSUM).
    f32=True: the kernel's f32-class mode -- x, w are bf16 term images (split3), y / u / aux_in float32."""
    C.require_device(x, w, bias, aux_in)
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty(M, N, dtype=torch.float32 if f32 else torch.bfloat16, device=x.device)
    aux_out = colsum = ws = None
    if epilogue in _TN_TWO_OUT:
        aux_out = torch.empty_like(y)
    elif epilogue in _TN_COLSUM:
        colsum = torch.empty(N, dtype=torch.float32, device=x.device)
        ws = C.workspace('linear_tn', M, N, x.device)
    C.check(C.lib().lvl_linear_tn(C.ptr(x), C.ptr(w), C.ptr(bias), C.ptr(y), C.ptr(aux_out), C.ptr(aux_in),
                                  C.ptr(colsum), C.ptr(ws), C.ptr(sched_block(x.device)), M, N, K, epilogue,
                                  C.LVL_F32 if f32 else C.LVL_BF16, C.stream_ptr()), 'lvl_linear_tn')
    if epilogue in _TN_TWO_OUT:
        return y, aux_out
    if epilogue in _TN_COLSUM:
        return y, colsum
    return y


def linear_tn_ragged_raw(x, w, bias=None, epilogue=C.EPI_BIAS):
    """One lvl_linear_tn_ragged call on bf16 tensors: y[M,N] = x[M,K] . w[N,K]^T (+ bias) for N % 64 == 0, K % 64 == 0.
    The entry takes LVL_EPI_BIAS only; `epilogue` is passed through so that its refusal is the library's."""
    C.require_device(x, w, bias)
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    C.check(C.lib().lvl_linear_tn_ragged(C.ptr(x), C.ptr(w), C.ptr(bias), C.ptr(y), C.ptr(sched_block(x.device)), M, N, K,
                                         epilogue, C.dtype_code(x), C.stream_ptr()), 'lvl_linear_tn_ragged')
    return y


def linear_tn_rows(x, w, bias=None):
    """y = x . w^T (+ bias) on the project's GEMMs for bf16 rows: lvl_linear_tn where _tn_ok holds (exactly as before),
    lvl_linear_tn_ragged where only _tn_ragged_ok does. None when neither tiles the shape (the caller decides, loudly)."""
    rows, n_out, n_in = x.shape[0], w.shape[0], w.shape[1]
    if _tn_ok(rows, n_out, n_in):
        return linear_tn_raw(x, w, bias, C.EPI_BIAS)
    if _tn_ragged_ok(rows, n_out, n_in):
        return linear_tn_ragged_raw(x, w, bias)
    return None


def _tn_rows_ok(rows: int, n_out: int, n_in: int) -> bool:
    return _tn_ok(rows, n_out, n_in) or _tn_ragged_ok(rows, n_out, n_in)


def linear_skinny_raw(x, w, bias=None, act=None):
    """One lvl_linear_skinny call on bf16 tensors: y[M,N] = act(x[M,K] . w[N,K]^T + bias) -- few rows: strips, many rows
    or 50432 columns: LDS-staged tiles (gemm_skinny.hip). act: None, C.ACT_GELU_NEW or C.ACT_SQRELU."""
    C.require_device(x, w, bias)
    M, K = x.shape
    y = torch.empty(M, w.shape[0], dtype=torch.bfloat16, device=x.device)
    C.check(C.lib().lvl_linear_skinny(C.ptr(x), C.ptr(w), C.ptr(bias), C.ptr(y), M, w.shape[0], K,
                                      -1 if act is None else act, C.stream_ptr()), 'lvl_linear_skinny')
    return y


def linear_skinny_f32c_raw(x3, w3, bias=None, act=None):
    """One lvl_linear_skinny_f32c call: y[M,N] float32 = act(x . w^T + bias) for float32 x [M,K], w [N,K] handed over as
    their bf16 term images x3 = split3(x, 0) [M,3K], w3 = split3(w, 1) [N,3K] (f32-class mode, ~2^-17 per product)."""
    C.require_device(x3, w3, bias)
    M, K3 = x3.shape
    y = torch.empty(M, w3.shape[0], dtype=torch.float32, device=x3.device)
    C.check(C.lib().lvl_linear_skinny_f32c(C.ptr(x3), C.ptr(w3), C.ptr(bias), C.ptr(y), M, w3.shape[0], K3,
                                           -1 if act is None else act, C.stream_ptr()), 'lvl_linear_skinny_f32c')
    return y


def linear_f32_rows(x2, w3, bias=None, act=None):
    """float32 x2 [M,K] against the term images w3 [N,3K] of a float32 weight: the 256-column-panel kernel's f32-class mode
    where it tiles and there are enough rows to fill it, lvl_linear_skinny_f32c otherwise (N % 16 == 0, K % 32 == 0).
    Inference helper (no autograd): the narrator's float32 decoder and ops.linear under no_grad."""
    M, K = x2.shape
    N = w3.shape[0]
    x3 = split3(x2 if x2.is_contiguous() else x2.contiguous(), 0)
    if M > 256 and _tn_ok(M, N, 3 * K):
        y = linear_tn_raw(x3, w3, bias, C.EPI_BIAS, f32=True)
        if act is not None:
            C.check(C.lib().lvl_act_inplace(C.ptr(y), y.numel(), act, C.dtype_code(y), C.stream_ptr()), 'lvl_act_inplace')
        return y
    return linear_skinny_f32c_raw(x3, w3, bias, act)


# Column-sum tokens (round 5). The bias gradient of a qkv Linear needs sum_rows(dout) of its attention core (the v third:
# every softmax row sums to 1). dout is the INPUT gradient of the projection Linear behind the attention, dout = dy W, so
# sum_rows(dout) = sum_rows(dy) W -- and sum_rows(dy) is the projection's own bias gradient, which the LayerNorm backward
# behind it produces anyway. A "token" is a [width] float32 tensor that travels beside an activation through the own
# autograd Functions (attention core -> projection -> fused add / LayerNorm); its GRADIENT is defined as the column sums of
# the activation's gradient, each Function computing it from what it already has (a [D] x [D, D] vector-matrix product,
# lvl_vec_mat_f32, a few microseconds) instead of a 300 MB pass over dout per attention. Exact in real arithmetic; in
# floating point it is the more accurate of the two (float32 sums of float32 column sums against sums of bf16-rounded
# rows). COLSUM_TOKENS = False switches the tokens off (the attention backward then reduces dout itself, as before): the
# tests compare the two paths.
COLSUM_TOKENS = True


def vec_mat(v, weight):
    """v [N] float32 . weight [N, K] -> [K] float32 (lvl_vec_mat_f32)."""
    w = weight.detach()
    if w.dtype != torch.float32 or not w.is_contiguous():
        w = w.float().contiguous()
    v = v.detach().float().contiguous()
    C.require_device(v, w)
    out = torch.empty(w.shape[1], dtype=torch.float32, device=w.device)
    C.check(C.lib().lvl_vec_mat_f32(C.ptr(v), C.ptr(w), C.ptr(out), w.shape[0], w.shape[1], C.stream_ptr()), 'lvl_vec_mat_f32')
    return out


class _LinearTokenFn(torch.autograd.Function):
    """(y, ytoken) = (x W^T, token of y) for a bf16 activation x that carries the column-sum token `xtoken`: _LinearFn's
    own-kernel path without a bias (the caller leaves it pending for the fused add + LayerNorm), plus the token rule
    d(xtoken) = d(ytoken) . W."""

    @staticmethod
    def forward(ctx, x, weight, xtoken):
        x2 = x.reshape(-1, x.shape[-1])
        x2 = x2 if x2.is_contiguous() else x2.contiguous()
        w, wt = weight_copies(weight)
        ctx.save_for_backward(x2, wt, weight)
        ctx.meta = (weight.dtype, x.shape)
        ctx.set_materialize_grads(False)        # an unused token arrives as None, not as zeros
        y = linear_tn_raw(x2, w, None, C.EPI_BIAS)
        return y.reshape(*x.shape[:-1], weight.shape[0]), x.new_zeros(weight.shape[0], dtype=torch.float32)   # token VALUE: unused, defined (zeros)

    @staticmethod
    def backward(ctx, dy, dytoken):
        x2, wt, weight = ctx.saved_tensors
        wdt, xshape = ctx.meta
        if dy is None:
            return None, None, None
        dy2 = dy.reshape(-1, dy.shape[-1])
        dy2 = dy2 if dy2.is_contiguous() else dy2.contiguous()
        with torch.autocast('cuda', enabled=False):
            dx, dw, _ = _linear_backward(ctx.needs_input_grad[:2], dy2, x2, wt, OWN_BF16, wdt)
            dtok = vec_mat(dytoken, weight) if (dytoken is not None and ctx.needs_input_grad[2]) else None
        return None if dx is None else dx.reshape(xshape), dw, dtok


def linear_with_token(x, weight, xtoken):
    """(y, ytoken) of a bias-free Linear on a token-carrying bf16 activation, or (linear(x, weight), None) when the shapes
    are not the own kernels' (the token chain then simply ends: consumers fall back to reducing their rows)."""
    x = _act(x)
    rows, n_in, n_out = x.numel() // x.shape[-1], x.shape[-1], weight.shape[0]
    if xtoken is not None and weight.dtype == torch.float32 and _route(x, rows, n_out, n_in) == OWN_BF16:
        return _LinearTokenFn.apply(x, weight, xtoken)
    return linear(x, weight), None


def project(x, proj):
    """x @ proj for the [width, embed_dim] projection parameters (models.py:146,161): the Linear kernels against the
    transposed view (its gradient flows back to `proj` through the view)."""
    return linear(x, proj.t())


def linear(x, weight, bias=None, ln=None):
    """nn.Linear forward with hand-written forward / input-gradient / weight-gradient GEMMs behind it.
    Activation dtype = x.dtype (the autocast dtype when autocast is on; fp16 -> bf16); parameters stay masters.
    ln: the LnRecipe of x when x is a LayerNorm output that is to be rebuilt in backward instead of kept (_LinearFn)."""
    x = _act(x)
    if x.dtype == torch.bfloat16 and x.is_cuda and not (torch.is_grad_enabled() and (
            x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad))):
        # inference, widths the 256-column-panel kernel does not tile (the narrator's pooling projection to_kv
        # [128 x 768], coca.py:78): the strip / LDS-tile kernel of the decoder (lvl_linear_skinny) instead of the library
        rows, n_in, n_out = x.numel() // x.shape[-1], x.shape[-1], weight.shape[0]
        if _skinny_ok(rows, n_out, n_in):
            x2 = x.reshape(-1, n_in)
            return linear_skinny_raw(x2 if x2.is_contiguous() else x2.contiguous(), weight_copies(weight)[0],
                                     _f32(bias)).reshape(*x.shape[:-1], n_out)
    if F32_MFMA and x.dtype == torch.float32 and x.is_cuda and weight.dtype == torch.float32 and not (
            torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or
                                         (bias is not None and bias.requires_grad))):
        # float32 inference on widths the panel kernel does not tile (small towers, the narrator's pooling projections,
        # round 5): the strip kernel's f32-class mode instead of the library GEMM
        rows, n_in, n_out = x.numel() // x.shape[-1], x.shape[-1], weight.shape[0]
        if _skinny_f32_ok(rows, n_out, n_in):
            return linear_f32_rows(x.reshape(-1, n_in), weight_copies(weight, f32=True)[0],
                                   _f32(bias)).reshape(*x.shape[:-1], n_out)
    return _LinearFn.apply(x, weight, bias, _ln_for(ln, x))


# --------------------------------------------------------------------------------------------------
# LayerNorm (optionally fused with residual + bias add)
# --------------------------------------------------------------------------------------------------
def _mixed_dtypes(x, x2, dy=None, dadd=None):
    # the mixed entry points take no dtype tag: a tensor of another element size would be read past its end
    for name, t, dt in (('x', x, torch.float32), ('x2', x2, torch.bfloat16), ('dy', dy, torch.bfloat16),
                        ('dadd', dadd, torch.float32)):
        if t is not None and (t.dtype != dt or not t.is_contiguous()):
            raise TypeError(f'layernorm (mixed): {name} must be a contiguous {dt} tensor, got {t.dtype}')
    for name, t in (('x2', x2), ('dy', dy), ('dadd', dadd)):
        if t is not None and t.numel() != x.numel():
            raise ValueError(f'layernorm (mixed): {name} has {t.numel()} elements, x has {x.numel()}')


def _ln_fwd_launch(mixed, x, x2, xbias, gamma, beta, eps, keep_sum, flags=0):
    """The one forward launch under layernorm_fwd_raw and layernorm_fwd_mixed_raw (their entry points take the same
    arguments but the last, the dtype code or, mixed, the flags): checks, y (bf16 if mixed), the sum, the statistics, the call."""
    C.require_device(x, x2, xbias, gamma, beta)
    if mixed:
        _mixed_dtypes(x, x2)
    name = 'lvl_layernorm_fwd_mixed' if mixed else 'lvl_layernorm_fwd'
    rows, cols = _rows_cols(x)
    y = torch.empty_like(x, dtype=torch.bfloat16 if mixed else x.dtype)
    s = torch.empty_like(x) if keep_sum else None
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    C.check(getattr(C.lib(), name)(C.ptr(x), C.ptr(x2), C.ptr(xbias), C.ptr(gamma), C.ptr(beta), C.ptr(s), C.ptr(y),
                                   C.ptr(mean), C.ptr(rstd), rows, cols, float(eps), flags if mixed else C.dtype_code(x),
                                   C.stream_ptr()), name)
    return y, s, mean, rstd


def _ln_bwd_launch(mixed, dy, x, x2, xbias, gamma, mean, rstd, dadd, want_dxsum, want_branch, flags=0):
    """The one backward launch under layernorm_bwd_raw and layernorm_bwd_mixed_raw, as _ln_fwd_launch: (dx, dgamma, dbeta,
    dxsum or None, the branch's own gradient -- dx_plain, or bf16 dx2 if mixed -- or None)."""
    C.require_device(dy, x, x2, xbias, gamma, mean, rstd, dadd)
    if mixed:
        _mixed_dtypes(x, x2, dy, dadd)
    name = 'lvl_layernorm_bwd_mixed' if mixed else 'lvl_layernorm_bwd'
    rows, cols = _rows_cols(x)
    dx = torch.empty_like(x)
    dbranch = torch.empty_like(x, dtype=torch.bfloat16 if mixed else x.dtype) if want_branch else None
    dgamma = torch.empty(cols, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(cols, dtype=torch.float32, device=x.device)
    dxsum = torch.empty(cols, dtype=torch.float32, device=x.device) if want_dxsum else None
    ws = C.workspace('layernorm_bwd', rows, cols, x.device)
    C.check(getattr(C.lib(), name)(C.ptr(dy), C.ptr(x), C.ptr(x2), C.ptr(xbias), C.ptr(gamma), C.ptr(mean), C.ptr(rstd),
                                   C.ptr(dadd), C.ptr(dx), C.ptr(dbranch), C.ptr(dgamma), C.ptr(dbeta), C.ptr(dxsum),
                                   C.ptr(ws), rows, cols, flags if mixed else C.dtype_code(x), C.stream_ptr()), name)
    return dx, dgamma, dbeta, dxsum, dbranch


def layernorm_fwd_raw(x, x2, xbias, gamma, beta, eps, keep_sum):
    return _ln_fwd_launch(False, x, x2, xbias, gamma, beta, eps, keep_sum)


def layernorm_apply_raw(x, x2, xbias, gamma, beta, mean, rstd):
    """One lvl_layernorm_apply call: the y of the layernorm_fwd_raw call that had these operands and returned this
    mean / rstd, to the bit (pass its kept sum as x with x2 = xbias = None)."""
    C.require_device(x, x2, xbias, gamma, beta, mean, rstd)
    rows, cols = _rows_cols(x)
    y = torch.empty_like(x)
    C.check(C.lib().lvl_layernorm_apply(C.ptr(x), C.ptr(x2), C.ptr(xbias), C.ptr(gamma), C.ptr(beta), C.ptr(mean),
                                        C.ptr(rstd), C.ptr(y), rows, cols, C.dtype_code(x), C.stream_ptr()),
            'lvl_layernorm_apply')
    return y


def quickgelu_apply_raw(u):
    """One lvl_quickgelu_apply call: a = QuickGELU(u) with the arithmetic of linear_tn_raw's EPI_BIAS_QUICKGELU epilogue
    (whose second result is u)."""
    C.require_device(u)
    rows, cols = _rows_cols(u)
    a = torch.empty_like(u)
    C.check(C.lib().lvl_quickgelu_apply(C.ptr(u), C.ptr(a), rows, cols, C.dtype_code(u), C.stream_ptr()),
            'lvl_quickgelu_apply')
    return a


def layernorm_bwd_raw(dy, x, x2, xbias, gamma, mean, rstd, dadd, want_dxsum, want_plain=False):
    """(dx, dgamma, dbeta, dxsum): dx with dadd added, dxsum its column sums (want_dxsum). want_plain: a fifth value, the
    normalisation's own input gradient without dadd (dx = dx_plain + dadd); dxsum then sums that one."""
    out = _ln_bwd_launch(False, dy, x, x2, xbias, gamma, mean, rstd, dadd, want_dxsum, want_plain)
    return out if want_plain else out[:4]


def layernorm_fwd_mixed_raw(x, x2, xbias, gamma, beta, eps, keep_sum, general=False):
    """One lvl_layernorm_fwd_mixed call: x float32 (the residual stream), x2 bf16 or None. Returns y in bf16, the sum in
    float32 (keep_sum) and the statistics: layernorm_fwd_raw on x and x2.float() with y rounded once, to the bit.
    general: the general kernel also where there is an exact-width one (they agree to the bit)."""
    return _ln_fwd_launch(True, x, x2, xbias, gamma, beta, eps, keep_sum, C.LN_GENERAL if general else 0)


def layernorm_bwd_mixed_raw(dy, x, x2, xbias, gamma, mean, rstd, dadd, want_dxsum, want_dx2=False, plain=False,
                            general=False):
    """One lvl_layernorm_bwd_mixed call: dy bf16, x float32, x2 bf16 or None, dadd float32 or None. Returns
    (dx, dgamma, dbeta, dxsum, dx2): dx float32 (dadd added); dx2 (want_dx2 or plain) the branch gradient in bf16 -- dx
    rounded once, or with plain the gradient without dadd rounded once (dxsum then sums that one, in float32)."""
    flags = (C.LN_PLAIN if plain else 0) | (C.LN_GENERAL if general else 0)
    return _ln_bwd_launch(True, dy, x, x2, xbias, gamma, mean, rstd, dadd, want_dxsum, want_dx2 or plain, flags)


# The forward and the backward of every LayerNorm Function below ("The LayerNorm host layer"). Both reach
# the kernels through the four launchers above by their module-level names, looked up at each call.
def _ln_forward(x, x2, xbias, gamma, beta, eps, keep_sum, mixed=False, rec=None):
    """h = LayerNorm(x + x2 + xbias) on the plain kernels or, mixed, on the lvl_layernorm_*_mixed pair (float32 x, bf16 x2 and
    h). Returns (h, s, kept): s the sum (keep_sum, else None) and kept = (x, x2, xbias, gamma, mean, rstd), the tensors
    _ln_backward runs on -- the kept sum as x with x2 = xbias = None if there is one, else the operands in the forward's
    order. The recipe `rec` (an LnRecipe or None) is filled with those same operands: one rule for what rebuilds h and for
    what its backward reads."""
    x, x2 = x.contiguous(), (None if x2 is None else x2.contiguous())
    xb, g, b = _f32(xbias), _f32(gamma), _f32(beta)
    h, s, mean, rstd = (layernorm_fwd_mixed_raw if mixed else layernorm_fwd_raw)(x, x2, xb, g, b, eps, keep_sum)
    operands = (s, None, None) if keep_sum else (x, x2, xb)
    if rec is not None:
        rec.fill(*operands, g, b, mean, rstd)
    return h, s, (*operands, g, mean, rstd)


def _ln_backward(dh, kept, dadd, want_colsum, mixed=False, split=False, branch=True):
    """(dx, dbranch, dgamma, dbeta, colsum) of _ln_forward from its `kept` tensors for the gradient dh of h. dadd: the
    gradient that reaches the stream on another path (of the kept sum, or of the stream handed through), added to dx inside
    the kernel. dbranch is the gradient of the branch x2 (+ xbias) and colsum (want_colsum) its column sums in float32:
    without split dbranch is dx -- the same tensor on the plain kernels, dx rounded once to bf16 on the mixed ones; with split
    it excludes dadd (the pass form when the stream's own gradient arrived). branch=False: there is no branch, dbranch is
    not written. dgamma and dbeta are float32."""
    x, x2, xbias, g, mean, rstd = kept
    dh = dh.reshape(x.shape).contiguous()
    dadd = None if dadd is None else dadd.reshape(x.shape).contiguous()
    operands = (dh, x, x2, xbias, g, mean, rstd, dadd, want_colsum)
    if mixed:
        dx, dgamma, dbeta, colsum, dbranch = layernorm_bwd_mixed_raw(*operands, want_dx2=branch, plain=split)
    elif split:
        dx, dgamma, dbeta, colsum, dbranch = layernorm_bwd_raw(*operands, want_plain=True)
    else:
        dx, dgamma, dbeta, colsum = layernorm_bwd_raw(*operands)
        dbranch = dx
    return dx, dbranch, dgamma, dbeta, colsum


def _param_grads(pdt, *grads):
    """The float32 gradients the row kernels leave for parameters (dgamma, dbeta, a bias gradient that is a column sum) in
    those parameters' dtypes pdt; None where there is no such parameter (its dtype is None) or no gradient."""
    return tuple(None if (g is None or dt is None) else g.to(dt) for g, dt in zip(grads, pdt))


class _LayerNormFn(torch.autograd.Function):
    """y = LN(x) ; see lvl_layernorm_fwd/bwd. mixed (here and in the two fused forms below): the lvl_layernorm_*_mixed
    pair -- float32 stream, bf16 normalised rows and branch, no cast node on either side (_mixed_ln)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, rec=None, mixed=False):
        y, _, kept = _ln_forward(x, None, None, weight, bias, eps, False, mixed, rec)
        ctx.save_for_backward(*kept)
        ctx.pdt, ctx.mixed = (weight.dtype, bias.dtype), mixed
        return y

    @staticmethod
    def backward(ctx, dy):
        dx, _, dg, db, _ = _ln_backward(dy, ctx.saved_tensors, None, False, ctx.mixed, branch=False)
        return (dx, *_param_grads(ctx.pdt, dg, db), None, None, None)


# Residual stream dtype under autocast. Default: the autocast dtype (bf16) from the patch embedding to the final norm
# (INTEGRATION.md section 3). LAVILA_RESIDUAL_F32=1 (or ops.RESIDUAL_F32 = True) keeps the stream -- and its gradient --
# in float32 as the reference's AMP does (timesformer.py:353-366, 183-196: cat with the f32 cls_token, f32 LayerNorm
# outputs, only GEMM outputs are half): the LayerNorm sites then run the mixed kernels (lvl_layernorm_*_mixed), which read
# the float32 stream and the bf16 branch and write bf16 normalised rows -- and in backward the float32 stream gradient
# and the bf16 branch gradient -- themselves: the bits of the float32 kernels between a widening and a narrowing pass,
# without those passes. The stochastic-depth sites stay composed that way.
RESIDUAL_F32 = os.environ.get('LAVILA_RESIDUAL_F32', '0') == '1'


def _narrow(h):
    """A LayerNorm output that feeds GEMMs takes the autocast dtype (none: it is left as it is)."""
    lp = autocast_dtype()
    return h.to(lp) if (lp is not None and h.dtype == torch.float32) else h


def _mixed_ln(x, y=None):
    """Does this LayerNorm site take the mixed kernels? A float32 stream x, a bf16 branch y (if any), and a consumer that
    wants bf16 rows."""
    return (x.dtype == torch.float32 and x.is_cuda and (y is None or y.dtype == torch.bfloat16)
            and autocast_dtype() == torch.bfloat16)


def layer_norm(x, weight, bias, eps, stream=False, recipe=False):
    """stream=True: the output IS the residual stream (ln_pre): it keeps the dtype of x.
    recipe=True (here and in the fused forms below): the result is followed by the LnRecipe from which the Linear that
    consumes the normalised rows rebuilds them instead of keeping them (`ln=` of linear / mlp_quickgelu / ...)."""
    rec = LnRecipe() if recipe else None
    x = lowp(x)
    y = _LayerNormFn.apply(x, weight, bias, eps, rec, not stream and _mixed_ln(x))
    y = y if stream else _narrow(y)
    return (y, rec) if recipe else y


class _AddLayerNormFn(torch.autograd.Function):
    """(s, h) = (res + y + ybias, LN(res + y + ybias)); s is only materialised when keep_sum."""

    @staticmethod
    def forward(ctx, res, y, ybias, weight, bias, eps, keep_sum, rec=None, mixed=False):
        h, s, kept = _ln_forward(res, y, ybias, weight, bias, eps, keep_sum, mixed, rec)
        ctx.save_for_backward(*kept)
        ctx.keep_sum, ctx.mixed = keep_sum, mixed
        ctx.pdt = (weight.dtype, bias.dtype, ybias.dtype if ybias is not None else None)
        if keep_sum:
            return s, h
        dummy = h.new_empty(0)
        ctx.mark_non_differentiable(dummy)
        return dummy, h

    @staticmethod
    def backward(ctx, ds, dh):
        # ds: the gradient of the kept sum (the dummy has none); the branch's gradient is the stream's
        dx, dy, dg, db, colsum = _ln_backward(dh, ctx.saved_tensors, ds if ctx.keep_sum else None, ctx.pdt[2] is not None,
                                              ctx.mixed)
        dg, db, dyb = _param_grads(ctx.pdt, dg, db, colsum)
        return dx, dy, dyb, dg, db, None, None, None, None


# Residual adds in GEMM epilogues (LVL_EPI_BIAS_RESIDUAL; LAVILA_RESIDUAL_EPILOGUE=0 restores the composed form): the space
# attention's output projection and the MLP's fc2 add the residual stream in their epilogue -- in f32, before the one
# rounding of the sum -- and the LayerNorm behind reads the sum, instead of the GEMM writing y and a fused add + LayerNorm
# reading res and y: one [rows, D] pass less per site. Same-box A/B: 171.56 -> 170.96 ms per step.
RESIDUAL_EPILOGUE = os.environ.get('LAVILA_RESIDUAL_EPILOGUE', '1') != '0'


class _LinearResidualLayerNormFn(torch.autograd.Function):
    """(s, h) = (res + x W^T + b, LayerNorm(s)): `x1 = x + attn(norm1(t)); h2 = norm2(x1)` of SpaceTimeBlock
    (timesformer.py:192-196) as one GEMM with the residual epilogue + one plain LayerNorm pass. Backward: the LayerNorm
    backward kernel adds the stream's own gradient ds (the core's dadd) and leaves dsum, the gradient of the sum, whose
    column sums (colsum) are the bias gradient; dsum is the residual's gradient AND the GEMM's output gradient (input
    gradient: lvl_linear_tn on the transposed weight copy, weight gradient: lvl_linear_wgrad)."""

    @staticmethod
    def forward(ctx, x, weight, lbias, res, gamma, beta, eps, xtoken=None, rec=None):
        x2 = x.reshape(-1, x.shape[-1])
        x2 = x2 if x2.is_contiguous() else x2.contiguous()
        res2 = res.reshape(-1, res.shape[-1])
        res2 = res2 if res2.is_contiguous() else res2.contiguous()
        w, wt = weight_copies(weight)
        s = linear_tn_raw(x2, w, _f32(lbias), C.EPI_BIAS_RESIDUAL, aux_in=res2)
        h, _, kept = _ln_forward(s, None, None, gamma, beta, eps, False, rec=rec)
        ctx.has_token = xtoken is not None
        ctx.save_for_backward(x2, wt, *kept, *((weight,) if ctx.has_token else ()))
        ctx.meta = (weight.dtype, (gamma.dtype, beta.dtype, None if lbias is None else lbias.dtype), x.shape)
        return s.reshape(res.shape), h.reshape(res.shape)

    @staticmethod
    def backward(ctx, ds, dh):
        saved = ctx.saved_tensors             # ONE access: torch.utils.checkpoint's unpack hook refuses a second one
        x2, wt = saved[:2]
        wdt, pdt, xshape = ctx.meta
        want_tok = ctx.has_token and ctx.needs_input_grad[7]
        dsum, _, dg, dbeta, colsum = _ln_backward(dh, saved[2:8], ds, pdt[2] is not None or want_tok)
        with torch.autocast('cuda', enabled=False):
            dx = linear_tn_raw(dsum, wt, None, C.EPI_BIAS).reshape(xshape) if ctx.needs_input_grad[0] else None
            dw = _wgrad(dsum, x2, wdt) if ctx.needs_input_grad[1] else None
            # token rule: column sums of dx = (column sums of dsum) . W  (dx = dsum W)
            dtok = vec_mat(colsum, saved[8]) if want_tok else None
        dg, dbeta, db = _param_grads(pdt, dg, dbeta, colsum if ctx.needs_input_grad[2] else None)
        return dx, dw, db, dsum.reshape(ds.shape if ds is not None else dh.shape), dg, dbeta, None, dtok, None


def linear_residual_layer_norm(x, weight, lbias, res, gamma, beta, eps, xtoken=None, recipe=False):
    """(s, h) = (res + Linear(x), LayerNorm(s)) through the GEMM's residual epilogue, or None when the shapes / dtypes are
    not the benched bf16 configuration (the caller then composes linear + add_layer_norm as before). xtoken: the
    column-sum token of x (see COLSUM_TOKENS)."""
    x, res = _act(x), lowp(res)
    rows = x.numel() // x.shape[-1]
    n_out, n_in = weight.shape
    if not (RESIDUAL_EPILOGUE and res.dtype == torch.bfloat16 and _route(x, rows, n_out, n_in) == OWN_BF16):
        return None
    if xtoken is not None and weight.dtype != torch.float32:
        xtoken = None
    rec = LnRecipe() if recipe else None
    s, h = _LinearResidualLayerNormFn.apply(x, weight, lbias, res, gamma, beta, eps, xtoken, rec)
    return (s, _narrow(h), rec) if recipe else (s, _narrow(h))


def linear_add_layer_norm(x, weight, lbias, res, gamma, beta, eps, xtoken=None, recipe=False, keep_sum=True):
    """(s, h[, recipe]) = (res + Linear(x), LayerNorm(s)): linear_residual_layer_norm where it takes the configuration, else
    the composed form -- the Linear without its bias, then add_layer_norm with it (keep_sum=False: s may then be None)."""
    fused = linear_residual_layer_norm(x, weight, lbias, res, gamma, beta, eps, xtoken=xtoken, recipe=recipe)
    if fused is not None:
        return fused
    return add_layer_norm(res, linear(x, weight), lbias, gamma, beta, eps, keep_sum=keep_sum, recipe=recipe)


class _MlpResidualLayerNormFn(torch.autograd.Function):
    """(s, h) = (res + fc2(act(fc1(x) + b1)) + b2, LayerNorm(s)): `x = x + mlp(norm2(x))` of one block and the first
    LayerNorm of the NEXT consumer (timesformer.py:196 / 183; openai_model.py:200 / 199) -- _MlpFn with the residual
    epilogue on its second GEMM, then one plain LayerNorm pass. Backward = LayerNorm backward (adds the stream's own
    gradient ds, leaves dsum and its column sums = d b2), then _MlpFn's backward on dsum."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, res, gamma, beta, eps, ln=None, rec=None, act=ACT_QUICKGELU):
        res2 = res.reshape(-1, res.shape[-1])
        res2 = res2 if res2.is_contiguous() else res2.contiguous()
        s, saved = _mlp_forward(ctx, x, w1, b1, w2, ln, act, b2, res2)      # bf16 (the caller's condition)
        h, _, kept = _ln_forward(s, None, None, gamma, beta, eps, False, rec=rec)
        ctx.save_for_backward(*saved, *kept)
        ctx.meta = (w1.dtype, None if b1 is None else b1.dtype, w2.dtype,
                    (gamma.dtype, beta.dtype, None if b2 is None else b2.dtype), x.shape)
        return s.reshape(res.shape), h.reshape(res.shape)

    @staticmethod
    def backward(ctx, ds, dh):
        *mlp_kept, s, _, _, g, mean, rstd = ctx.saved_tensors
        pdt = ctx.meta[3]
        dsum, _, dg, dbeta, colsum = _ln_backward(dh, (s, None, None, g, mean, rstd), ds, pdt[2] is not None)
        del ds, s             # the sum and the stream's own gradient are done with: released before the MLP's GEMMs
        recipe = x2 = a = None
        if ctx.sel:
            *recipe, u, w1t, w2t = mlp_kept
        else:
            x2, u, a, w1t, w2t = mlp_kept
        with torch.autocast('cuda', enabled=False):
            dx, dw1, db1, dw2 = _mlp_backward(ctx, dsum, x2, u, a, w1t, w2t, recipe)
        dg, dbeta, db2 = _param_grads(pdt, dg, dbeta, colsum if ctx.needs_input_grad[4] else None)
        return dx, dw1, db1, dw2, db2, dsum.reshape(dh.shape), dg, dbeta, None, None, None, None


def mlp_residual_layer_norm(x, w1, b1, w2, b2, res, gamma, beta, eps, ln=None, recipe=False, act=ACT_QUICKGELU):
    """(s, h) = (res + Mlp(x), LayerNorm(s)) with the residual add in fc2's GEMM epilogue, or None when the configuration
    is not the benched bf16 one (the caller then composes mlp + add_layer_norm). ln: the LnRecipe of x (see
    mlp_quickgelu); recipe: see layer_norm; act: ACT_QUICKGELU or ACT_GELU (see mlp)."""
    _mlp_epilogues(act)
    x, res = _act(x), lowp(res)
    if not (RESIDUAL_EPILOGUE and x.dtype == torch.bfloat16 and res.dtype == torch.bfloat16 and _mlp_fused_ok(x, w1, b1, w2)):
        return None
    rec = LnRecipe() if recipe else None
    s, h = _MlpResidualLayerNormFn.apply(x, w1, b1, w2, b2, res, gamma, beta, eps, _ln_for(ln, x), rec, act)
    return (s, _narrow(h), rec) if recipe else (s, _narrow(h))


class _AddLayerNormPassFn(torch.autograd.Function):
    """(res, h) = (res, LN(res + y + ybias)): the sum is not materialised and `res` is handed through, so that a
    SECOND consumer of res (SpaceTimeBlock: x feeds both x + time_out and x + space_out, timesformer.py:183-196) can
    take it from here. Its gradient then arrives in THIS node and is added inside the LayerNorm backward kernel
    (dx = dx_plain + d_res_out) instead of by a separate full-size add of the autograd engine."""

    @staticmethod
    def forward(ctx, res, y, ybias, weight, bias, eps, ytoken=None, rec=None, mixed=False):
        h, _, kept = _ln_forward(res, y, ybias, weight, bias, eps, False, mixed, rec)
        ctx.save_for_backward(*kept)
        ctx.mixed, ctx.has_token = mixed, ytoken is not None
        ctx.pdt = (weight.dtype, bias.dtype, ybias.dtype if ybias is not None else None)
        return kept[0].view_as(kept[0]), h

    @staticmethod
    def backward(ctx, dres, dh):
        want_tok = ctx.has_token and ctx.needs_input_grad[6]
        # dres: the gradient of the stream handed through; the branch's own gradient (and its column sums) leaves it out
        dx, dy, dg, db, colsum = _ln_backward(dh, ctx.saved_tensors, dres, ctx.pdt[2] is not None or want_tok, ctx.mixed,
                                              split=dres is not None)
        dg, db, dyb = _param_grads(ctx.pdt, dg, db, colsum)
        return dx, dy, dyb, dg, db, None, (colsum if want_tok else None), None, None      # token rule: sum_rows(dy) itself


def add_layer_norm_pass(res, y, ybias, weight, bias, eps, ytoken=None, recipe=False):
    """Returns (res_again, h) with h = LayerNorm(res + y (+ ybias)); use res_again for the next consumer of res.
    ytoken: the column-sum token of y (see COLSUM_TOKENS)."""
    res = lowp(res)
    mixed = _mixed_ln(res, y)
    if y.dtype != res.dtype:       # the token stands for column sums of a y of the stream's dtype
        y, ytoken = (y if mixed else y.to(res.dtype)), None
    rec = LnRecipe() if recipe else None
    r, h = _AddLayerNormPassFn.apply(res, y, ybias, weight, bias, eps, ytoken, rec, mixed)
    return (r, _narrow(h), rec) if recipe else (r, _narrow(h))


def add_layer_norm(res, y, ybias, weight, bias, eps, keep_sum=True, recipe=False):
    """Returns (s, h) with s = res + y (+ ybias) and h = LayerNorm(s). With keep_sum=False s is None."""
    res = lowp(res)
    mixed = _mixed_ln(res, y)
    if y.dtype != res.dtype and not mixed:
        y = y.to(res.dtype)
    rec = LnRecipe() if recipe else None
    s, h = _AddLayerNormFn.apply(res, y, ybias, weight, bias, eps, keep_sum, rec, mixed)
    return ((s if keep_sum else None), _narrow(h)) + ((rec,) if recipe else ())


# --------------------------------------------------------------------------------------------------
# Stochastic depth: per-sample scaled residual add + LayerNorm
# --------------------------------------------------------------------------------------------------
def droppath_add_layernorm_fwd_raw(res, y, ybias, scale, rows_per_sample, gamma, beta, eps):
    """One lvl_droppath_add_layernorm_fwd call: (h, s, mean, rstd) with s = res + scale[sample] * (y + ybias)."""
    C.require_device(res, y, ybias, scale, gamma, beta)
    rows, cols = _rows_cols(res)
    s, h = torch.empty_like(res), torch.empty_like(res)
    mean = torch.empty(rows, dtype=torch.float32, device=res.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=res.device)
    C.check(C.lib().lvl_droppath_add_layernorm_fwd(C.ptr(res), C.ptr(y), C.ptr(ybias), C.ptr(scale), C.ptr(gamma),
                                                   C.ptr(beta), C.ptr(s), C.ptr(h), C.ptr(mean), C.ptr(rstd), rows,
                                                   int(rows_per_sample), cols, float(eps), C.dtype_code(res),
                                                   C.stream_ptr()), 'lvl_droppath_add_layernorm_fwd')
    return h, s, mean, rstd


def droppath_add_layernorm_bwd_raw(dh, s, gamma, mean, rstd, scale, dadd, rows_per_sample, want_dysum):
    """One lvl_droppath_add_layernorm_bwd call: (ds, dy, dgamma, dbeta, dysum)."""
    C.require_device(dh, s, gamma, mean, rstd, scale, dadd)
    rows, cols = _rows_cols(s)
    ds, dy = torch.empty_like(s), torch.empty_like(s)
    dgamma = torch.empty(cols, dtype=torch.float32, device=s.device)
    dbeta = torch.empty(cols, dtype=torch.float32, device=s.device)
    dysum = torch.empty(cols, dtype=torch.float32, device=s.device) if want_dysum else None
    ws = C.workspace('droppath_add_layernorm_bwd', rows, cols, s.device)
    C.check(C.lib().lvl_droppath_add_layernorm_bwd(C.ptr(dh), C.ptr(s), C.ptr(gamma), C.ptr(mean), C.ptr(rstd),
                                                   C.ptr(scale), C.ptr(dadd), C.ptr(ds), C.ptr(dy), C.ptr(dgamma),
                                                   C.ptr(dbeta), C.ptr(dysum), C.ptr(ws), rows, int(rows_per_sample),
                                                   cols, C.dtype_code(s), C.stream_ptr()),
            'lvl_droppath_add_layernorm_bwd')
    return ds, dy, dgamma, dbeta, dysum


class _ScaledAddLayerNormFn(torch.autograd.Function):
    """(s, h) = (res + c_b * (y + ybias), LN(s)) with one c_b per sample (stochastic depth: timesformer.py:192,196 and the
    LayerNorm that reads the sum). s is always kept: the backward runs on it. d scale is None (the mask is a constant)."""

    @staticmethod
    def forward(ctx, res, y, ybias, scale, rows_per_sample, weight, bias, eps, ytoken=None):
        res, y = res.contiguous(), y.contiguous()
        yb, g, b, c = _f32(ybias), _f32(weight), _f32(bias), _f32(scale)
        h, s, mean, rstd = droppath_add_layernorm_fwd_raw(res, y, yb, c, rows_per_sample, g, b, eps)
        ctx.save_for_backward(s, g, mean, rstd, c)
        ctx.rps = int(rows_per_sample)
        ctx.has_token = ytoken is not None
        ctx.pdt = (weight.dtype, bias.dtype, ybias.dtype if ybias is not None else None)
        ctx.set_materialize_grads(False)        # an unused s (the final norm) or h (a closing add) arrives as None
        return s, h

    @staticmethod
    def backward(ctx, ds, dh):
        s, g, mean, rstd, c = ctx.saved_tensors
        if ds is None and dh is None:
            return (None,) * 9
        want_tok = ctx.has_token and ctx.needs_input_grad[8]
        dh = torch.zeros_like(s) if dh is None else dh.contiguous()
        dres, dy, dg, db, dysum = droppath_add_layernorm_bwd_raw(dh, s, g, mean, rstd, c,
                                                                 None if ds is None else ds.contiguous(),
                                                                 ctx.rps, ctx.pdt[2] is not None or want_tok)
        dg, db, dyb = _param_grads(ctx.pdt, dg, db, dysum)
        return dres, dy, dyb, None, None, dg, db, None, (dysum if want_tok else None)


def scaled_add_layer_norm(res, y, ybias, scale, rows_per_sample, weight, bias, eps, ytoken=None):
    """Returns (s, h) with s = res + scale[sample] * (y (+ ybias)) and h = LayerNorm(s); rows r of the flattened res belong
    to sample r // rows_per_sample and scale is one float32 per sample (DropPath.sample_scale: 0 or 1 / keep).
    ytoken: the column-sum token of y (see COLSUM_TOKENS); without one the producer of y reduces its gradient itself."""
    res = lowp(res)
    if y.dtype != res.dtype:
        y, ytoken = y.to(res.dtype), None
    s, h = _ScaledAddLayerNormFn.apply(res, y, ybias, scale, rows_per_sample, weight, bias, eps, ytoken)
    return s, _narrow(h)


# --------------------------------------------------------------------------------------------------
# bias + QuickGELU
# --------------------------------------------------------------------------------------------------
class _BiasQuickGELUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, bias):
        u = u.contiguous()
        b = _f32(bias)
        C.require_device(u, b)
        rows, cols = _rows_cols(u)
        a = torch.empty_like(u)
        C.check(C.lib().lvl_bias_quickgelu_fwd(C.ptr(u), C.ptr(b), C.ptr(a), rows, cols, C.dtype_code(u),
                                               C.stream_ptr()), 'lvl_bias_quickgelu_fwd')
        ctx.save_for_backward(u, b)
        ctx.bdt = bias.dtype if bias is not None else None
        return a

    @staticmethod
    def backward(ctx, da):
        u, b = ctx.saved_tensors
        da = da.contiguous()
        rows, cols = _rows_cols(u)
        du = torch.empty_like(u)
        dbias = torch.empty(cols, dtype=torch.float32, device=u.device) if b is not None else None
        ws = C.workspace('bias_quickgelu_bwd', rows, cols, u.device) if b is not None else None
        C.check(C.lib().lvl_bias_quickgelu_bwd(C.ptr(da), C.ptr(u), C.ptr(b), C.ptr(du), C.ptr(dbias), C.ptr(ws),
                                               rows, cols, C.dtype_code(u), C.stream_ptr()),
                'lvl_bias_quickgelu_bwd')
        return du, (dbias.to(ctx.bdt) if b is not None else None)


def bias_quick_gelu(u, bias=None):
    """(u + bias) * sigmoid(1.702 (u + bias))"""
    return _BiasQuickGELUFn.apply(lowp(u), bias)


# --------------------------------------------------------------------------------------------------
# patch gather + token assembly
# --------------------------------------------------------------------------------------------------
def patchify(video, patch: int, dtype: torch.dtype, frame_major: bool = False, ld=None) -> torch.Tensor:
    """[B,C,F,H,W] f32 (or, frame_major, [B,F,C,H,W]) -> [B, F*N, C*P*P]; both layouts are read in place (no gradient
    w.r.t. pixels: the reference never needs one). An ingest.PendingClip (uint8 frames + crop blocks, channel-major) goes to
    the patch matrix in one kernel, with `ld` >= C*P*P columns per row, the ones behind C*P*P zero."""
    if isinstance(video, PendingClip):
        if frame_major:
            refuse_pending(video, 'a frame-major ([B,F,C,H,W]) entry point')
        return video.patches(patch, dtype, ld)
    video = video.detach()
    if video.dtype != torch.float32:
        video = video.float()          # fp16 clips of the --use-half eval recipes
    video = video.contiguous()
    C.require_device(video)
    if frame_major:
        B, Fr, Ch, H, W = video.shape
    else:
        B, Ch, Fr, H, W = video.shape
    N = (H // patch) * (W // patch)
    out = torch.empty(B, Fr * N, Ch * patch * patch, dtype=dtype, device=video.device)
    C.check(C.lib().lvl_patchify(C.ptr(video), C.ptr(out), B, Ch, Fr, H, W, patch, int(frame_major),
                                 C.dtype_code(out), C.stream_ptr()), 'lvl_patchify')
    return out


class _EmbedTokensFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pe, cls_token, pos_embed, temporal_embed, frames, n_per_frame):
        pe = pe.contiguous()
        B, FN, D = pe.shape
        cls, pos, tem = _f32(cls_token).reshape(-1), _f32(pos_embed).reshape(-1, D), _f32(temporal_embed).reshape(-1, D)
        C.require_device(pe, cls, pos, tem)
        x = torch.empty(B, 1 + FN, D, dtype=pe.dtype, device=pe.device)
        C.check(C.lib().lvl_embed_tokens_fwd(C.ptr(pe), C.ptr(cls), C.ptr(pos), C.ptr(tem), C.ptr(x), B, frames,
                                             n_per_frame, D, C.dtype_code(pe), C.stream_ptr()),
                'lvl_embed_tokens_fwd')
        ctx.dims = (B, frames, n_per_frame, D, temporal_embed.shape[1])
        ctx.pdt = (cls_token.dtype, pos_embed.dtype, temporal_embed.dtype)
        return x

    @staticmethod
    def backward(ctx, dx):
        B, Fr, N, D, num_frames = ctx.dims
        if dx.is_cuda and dx.dtype in (torch.bfloat16, torch.float32) and D % 8 == 0 and B > 0:
            # one pass over dx (lvl_embed_tokens_bwd) instead of a float32 copy of it and three framework reductions
            dx = dx.contiguous()
            dpos = torch.empty(1, N + 1, D, dtype=torch.float32, device=dx.device)
            dtem = torch.empty(1, num_frames, D, dtype=torch.float32, device=dx.device)
            ws = torch.empty(int(C.lib().lvl_embed_tokens_bwd_ws(Fr, N, D)), dtype=torch.float32, device=dx.device)
            C.check(C.lib().lvl_embed_tokens_bwd(C.ptr(dx), C.ptr(dpos), C.ptr(dtem), C.ptr(ws), B, Fr, N, D, num_frames,
                                                 C.dtype_code(dx), C.stream_ptr()), 'lvl_embed_tokens_bwd')
            # d cls_token is its own tensor, NOT a view of dpos: GradScaler.unscale_ / clip_grad_norm_ scale gradients in
            # place, and two parameters sharing gradient storage would be scaled twice (caught by test_grad_scaler_step_*)
            return (dx[:, 1:], dpos[:, 0].reshape(1, 1, D).to(ctx.pdt[0], copy=True), dpos.to(ctx.pdt[1]),
                    dtem.to(ctx.pdt[2]), None, None)
        body = dx[:, 1:].reshape(B, Fr, N, D).float()
        d0 = dx[:, 0].float().sum(0)                                    # cls row: d cls_token = d pos[0]
        dpos = torch.cat([d0[None], body.sum((0, 1))], 0)[None]         # [1, N+1, D]
        dtem = dx.new_zeros((1, num_frames, D), dtype=torch.float32)
        dtem[0, :Fr] = body.sum((0, 2))
        return (dx[:, 1:], d0.reshape(1, 1, D).to(ctx.pdt[0]), dpos.to(ctx.pdt[1]), dtem.to(ctx.pdt[2]),
                None, None)


def embed_tokens(pe, cls_token, pos_embed, temporal_embed, frames, n_per_frame):
    """temporal_embed None (the per-frame ViT of openai_model.VisionTransformer: frames == 1, no temporal embedding): a zero
    row stands in for it; the C entry is called as for every other caller."""
    if temporal_embed is None:
        temporal_embed = torch.zeros(1, max(1, frames), pe.shape[-1], dtype=torch.float32, device=pe.device)
    return _EmbedTokensFn.apply(lowp(pe), cls_token, pos_embed, temporal_embed, frames, n_per_frame)


class _TextEmbedFn(torch.autograd.Function):
    """x = token_embedding(text) + positional_embedding[:L] (models.py:152-153) as one gather kernel, and its backward as
    a sort-free deterministic segmented sum (csrc/text_embed.hip): torch's embedding_dense_backward takes a rocPRIM radix
    sort above 3072 token rows, whose histogram memsets turn into memset NODES of a replayed hipGraph."""

    @staticmethod
    def forward(ctx, text, table, pos, out_dtype):
        B, L = text.shape
        V, W = table.shape
        tab, p = _f32(table), _f32(pos)
        C.require_device(tab, p)
        x = torch.empty(B, L, W, dtype=out_dtype, device=table.device)
        C.check(C.lib().lvl_text_embed_fwd(C.ptr(text), _token_stride(text), C.ptr(tab), C.ptr(p), C.ptr(x), B, L, W, V,
                                           C.dtype_code(x), C.stream_ptr()), 'lvl_text_embed_fwd')
        ctx.save_for_backward(text)           # saved, not a plain attribute: an in-place write before backward then raises
        ctx.meta = (V, W, pos.shape[0], table.dtype, pos.dtype)
        return x

    @staticmethod
    def backward(ctx, dx):
        text, = ctx.saved_tensors
        B, L = text.shape
        V, W, ctx_len, tdt, pdt = ctx.meta
        want_table, want_pos = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if not (want_table or want_pos):
            return None, None, None, None
        dx = dx.contiguous()
        # a frozen table (or frozen positions) gets a null pointer: no dense [V, W] zero-fill and build for nothing
        dtable = torch.empty(V, W, dtype=torch.float32, device=dx.device) if want_table else None
        dpos = torch.empty(ctx_len, W, dtype=torch.float32, device=dx.device) if want_pos else None
        ws = (torch.empty(int(C.lib().lvl_text_embed_bwd_ws(B, L, V)), dtype=torch.int32, device=dx.device)
              if want_table else None)
        C.check(C.lib().lvl_text_embed_bwd(C.ptr(dx), C.ptr(text), _token_stride(text), C.ptr(dtable), C.ptr(dpos),
                                           C.ptr(ws), B, L, W, V, ctx_len, C.dtype_code(dx), C.stream_ptr()),
                'lvl_text_embed_bwd')
        return (None, dtable.to(tdt) if want_table else None, dpos.to(pdt) if want_pos else None, None)


def _token_stride(text):
    """Row stride of a [B, L] token view for the kernels. torch leaves the stride of a size-1 dimension arbitrary (`col.t()`
    of an [L, 1] tensor reports (1, 1)); with one row it is never used, so L is passed."""
    return text.shape[1] if text.shape[0] == 1 else text.stride(0)


def text_embed(text, table, pos, out_dtype):
    """CLIP.encode_text's first two lines on the own kernels when they apply (device int64 [B, L] tokens with unit inner
    stride on the table's device, float32 table / positions of a width that is a multiple of 8 and at most 2048); None
    otherwise (the caller keeps nn.Embedding). Never raises on tokens nn.Embedding accepts: a `text[:, :L]` view is read in
    place through its row stride, a single row is read with stride L whatever torch reports for it, and a batch whose rows
    overlap (row stride below L: `ids.expand(B, L)`) is read from a contiguous copy."""
    if not (text.is_cuda and text.dtype == torch.int64 and text.dim() == 2 and text.stride(1) == 1
            and text.shape[0] > 0 and text.shape[1] > 0 and text.device == table.device and pos.device == table.device
            and table.dtype == torch.float32 and pos.dtype == torch.float32 and table.is_contiguous()
            and pos.is_contiguous() and table.shape[1] % 8 == 0 and table.shape[1] <= 2048
            and pos.shape[0] >= text.shape[1] and out_dtype in (torch.float32, torch.bfloat16)):
        return None
    if text.shape[0] > 1 and text.stride(0) < text.shape[1]:
        text = text.contiguous()
    return _TextEmbedFn.apply(text, table, pos, out_dtype)


# --------------------------------------------------------------------------------------------------
# packed caption rows (csrc/pack_rows.hip): [B, L, D] <-> the len_b leading rows of every caption, [R, D]
# --------------------------------------------------------------------------------------------------
def _row_view(t, what):
    """A [B, L, D] bf16 / f32 device view the row kernels address in place: unit column stride, D and both row strides
    multiples of 8 elements, 16-byte aligned base."""
    if not t.is_cuda:
        C.require_device(t)                           # raises: there is no CPU fallback
    if t.dim() != 3 or t.stride(2) != 1 or t.shape[2] % 8 or t.stride(0) % 8 or t.stride(1) % 8 or t.stride(1) < t.shape[2]:
        raise C.HipExtensionError(f'{what}: a [B, L, D] view with unit column stride, D and the row strides multiples of 8 '
                                  f'is needed; got {tuple(t.shape)} with strides {tuple(t.stride())}')
    return t


def _row_offsets(cu, B):
    C.require_device(cu)
    if cu.dtype != torch.int32 or cu.numel() != B + 1:
        raise C.HipExtensionError(f'row offsets must be {B + 1} int32 values, got {tuple(cu.shape)} {cu.dtype}')
    return cu


def rows_pack_raw(src, cu, rows: int):
    """lvl_rows_pack: src [B, L, D] (a strided view is read in place), cu [B + 1] int32 on the device with cu[B] == rows (the
    caller holds the lengths) -> [rows, D]: caption b's first cu[b + 1] - cu[b] rows at cu[b]."""
    B, L, D = _row_view(src, 'rows_pack').shape
    out = torch.empty(int(rows), D, dtype=src.dtype, device=src.device)
    C.check(C.lib().lvl_rows_pack(C.ptr(src), src.stride(0), src.stride(1), C.ptr(_row_offsets(cu, B)), B, L, D, C.ptr(out),
                                  C.dtype_code(src), C.stream_ptr()), 'lvl_rows_pack')
    return out


def rows_unpack_raw(src, cu, B: int, L: int, out=None):
    """lvl_rows_unpack: src [R, D] contiguous -> out [B, L, D] (fresh, or a strided view written in place): caption b's
    rows followed by zeros; every element of out[:, :, :D] is written."""
    C.require_device(src)
    D = src.shape[1]
    if out is None:
        out = torch.empty(B, L, D, dtype=src.dtype, device=src.device)
    if tuple(_row_view(out, 'rows_unpack').shape) != (B, L, D) or out.dtype != src.dtype:
        raise C.HipExtensionError(f'rows_unpack: destination {tuple(out.shape)} {out.dtype} for [{B}, {L}, {D}] {src.dtype}')
    C.check(C.lib().lvl_rows_unpack(C.ptr(src), C.ptr(_row_offsets(cu, B)), B, L, D, C.ptr(out), out.stride(0), out.stride(1),
                                    C.dtype_code(src), C.stream_ptr()), 'lvl_rows_unpack')
    return out


class _PackRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cu, rows):
        ctx.cu, ctx.shape = cu, x.shape[:2]           # an index tensor (no gradient, not an output): a plain attribute
        return rows_pack_raw(x, cu, rows)

    @staticmethod
    def backward(ctx, dy):
        return rows_unpack_raw(dy.contiguous(), ctx.cu, *ctx.shape), None, None


class _UnpackRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, cu, B, L):
        ctx.cu, ctx.rows = cu, y.shape[0]
        return rows_unpack_raw(y.contiguous(), cu, B, L)

    @staticmethod
    def backward(ctx, dx):
        if dx.stride(2) != 1 or dx.stride(1) % 8 or dx.stride(0) % 8:
            dx = dx.contiguous()
        return rows_pack_raw(dx, ctx.cu, ctx.rows), None, None, None


def pack_rows(x, cu, rows: int):
    """[B, L, D] -> [rows, D]: the leading cu[b + 1] - cu[b] rows of every caption, in caption order; the backward is
    unpack_rows on the gradient (zeros for the rows left behind)."""
    return _PackRowsFn.apply(x, cu, rows)


def unpack_rows(y, cu, B: int, L: int):
    """[R, D] -> [B, L, D], zeros behind every caption's rows; the backward is pack_rows on the gradient."""
    return _UnpackRowsFn.apply(y, cu, B, L)


# --------------------------------------------------------------------------------------------------
# attention cores
# --------------------------------------------------------------------------------------------------
def set_fp8_qk(on: bool):
    """BASELINE configs[3]'s "fp8 MFMA QK^T path": the streaming space kernels (groups of more than 288 keys, bf16) compute
    their scores with the fp8 matrix instruction on e4m3-rounded q / k fragments, forward and backward consistently
    (include/lavila_hip.h: lvl_set_fp8_qk). Off by default; LAVILA_FP8_QK=1 in the environment is the same switch."""
    C.check(C.lib().lvl_set_fp8_qk(1 if on else 0), 'lvl_set_fp8_qk')


def _qkv_bias_grad(dqkv, dout, dtype):
    """d(bias) of the qkv Linear that feeds an attention core = column sums of dqkv, without reading the k and v
    thirds: every softmax row sums to 1, so sum_rows(dv) = sum_rows(dout) exactly, and the scores do not change when a
    constant vector is added to every key, so sum_rows(dk) = 0. Only the q third is reduced from dqkv itself
    (2/3 of the bytes of the plain reduction saved on q|k|v, 1/3 read back from dout)."""
    D = dout.shape[-1]
    rows = dout.numel() // D
    db = torch.empty(3 * D, dtype=torch.float32, device=dqkv.device)
    ws = C.workspace('qkv_bias_grad', rows, D, dqkv.device)
    C.check(C.lib().lvl_qkv_bias_grad(C.ptr(dqkv), C.ptr(dout), C.ptr(db), C.ptr(ws), rows, D, C.dtype_code(dqkv),
                                      C.stream_ptr()), 'lvl_qkv_bias_grad')
    return db.to(dtype)


class _DividedAttnFn(torch.autograd.Function):
    """`bias` (optional): the bias of the qkv Linear that produced `qkv` (already added there; the caller hands the
    Linear a detached copy). It takes no part in the forward; its gradient comes out of the backward call itself
    (lvl_divided_attn_bwd_bias: q third from the backward kernels' own column sums where they have the rider, k third 0,
    v third from the output's column-sum token when the consumer supplies it -- see COLSUM_TOKENS -- else from dout).
    want_token: also return the column-sum token of `out` (for a consumer that is an own token-aware Function)."""

    @staticmethod
    def forward(ctx, qkv, bias, frames, n_per_frame, heads, mode, want_token=False):
        qkv = qkv.contiguous()
        C.require_device(qkv)
        B, T, D3 = qkv.shape
        D = D3 // 3
        if D != heads * 64 or T != 1 + frames * n_per_frame:
            raise C.HipExtensionError(f'divided attention: qkv {tuple(qkv.shape)} inconsistent with heads={heads} '
                                      f'(head dim must be 64), frames={frames}, patches/frame={n_per_frame}')
        if qkv.dtype == torch.bfloat16 and not C.lib().lvl_attention_fast_path(mode, frames, n_per_frame, heads):
            warn_once(('attn', mode, frames, n_per_frame), f'divided attention ({"time" if mode else "space"}, {frames} '
                      f'frames x {n_per_frame} patches) has no MFMA kernel yet and runs on the generic (slow) kernels')
        out, lse = divided_attn_fwd_raw(qkv, frames, n_per_frame, heads, mode)
        ctx.save_for_backward(qkv, out, lse)
        ctx.cfg = (B, frames, n_per_frame, heads, mode, None if bias is None else bias.dtype)
        ctx.want_token = bool(want_token)
        # an unused token must arrive in backward as None (= "nobody computed the column sums"), not as zeros
        ctx.set_materialize_grads(False)
        if want_token:
            return out, out.new_zeros(D, dtype=torch.float32)      # the token's VALUE is never read; zeros, not uninitialised memory (hooks, anomaly mode)
        return out

    @staticmethod
    def backward(ctx, dout, dtoken=None):
        qkv, out, lse = ctx.saved_tensors
        B, Fr, N, H, mode, bdt = ctx.cfg
        if dout is None:                        # the output itself was not used: zero gradient, no token either
            dout, dtoken = torch.zeros_like(out), None
        dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        ws = C.workspace('divided_attn_bwd', B * H, 1 + Fr * N, qkv.device)
        if bdt is not None and ctx.needs_input_grad[1]:
            D = H * 64
            db = torch.empty(3 * D, dtype=torch.float32, device=qkv.device)
            n2 = int(C.lib().lvl_divided_attn_bwd_bias_ws(B, Fr, N, H, mode, C.dtype_code(qkv)))
            ws2 = torch.empty(max(n2, 4), dtype=torch.float32, device=qkv.device)
            tok = dtoken.float().contiguous() if dtoken is not None else None
            C.require_device(tok)
            C.check(C.lib().lvl_divided_attn_bwd_bias(C.ptr(qkv), C.ptr(out), C.ptr(dout), C.ptr(lse), C.ptr(dqkv),
                                                      C.ptr(ws), C.ptr(tok), C.ptr(db), C.ptr(ws2), B, Fr, N, H, mode,
                                                      C.dtype_code(qkv), C.stream_ptr()), 'lvl_divided_attn_bwd_bias')
            return dqkv, db.to(bdt), None, None, None, None, None
        C.check(C.lib().lvl_divided_attn_bwd(C.ptr(qkv), C.ptr(out), C.ptr(dout), C.ptr(lse), C.ptr(dqkv), C.ptr(ws),
                                             B, Fr, N, H, mode, C.dtype_code(qkv), C.stream_ptr()),
                'lvl_divided_attn_bwd')
        return dqkv, None, None, None, None, None, None


def divided_attn_fwd_raw(qkv, frames, n_per_frame, heads, mode):
    """One lvl_divided_attn_fwd call: (out [B,T,D], lse [B,H,T])."""
    B, T, D3 = qkv.shape
    out = torch.empty(B, T, D3 // 3, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B, heads, T, dtype=torch.float32, device=qkv.device)
    ws = C.workspace('divided_attn_fwd', B * heads, T, qkv.device)
    C.check(C.lib().lvl_divided_attn_fwd(C.ptr(qkv), C.ptr(out), C.ptr(lse), C.ptr(ws), B, frames, n_per_frame,
                                         heads, mode, C.dtype_code(qkv), C.stream_ptr()), 'lvl_divided_attn_fwd')
    return out, lse


def divided_attention(qkv, frames, n_per_frame, heads, mode, bias=None, want_token=False):
    """mode: 'space' | 'time'. qkv [B,T,3D] -> [B,T,D] (timesformer.py:110-140 between the two Linears).
    bias, want_token: see _DividedAttnFn; with want_token -> (out, token), token None when tokens are switched off."""
    m = {'space': C.ATTN_SPACE, 'time': C.ATTN_TIME}[mode]
    if want_token:
        if COLSUM_TOKENS and bias is not None and torch.is_grad_enabled():
            return _DividedAttnFn.apply(lowp(qkv), bias, frames, n_per_frame, heads, m, True)
        return _DividedAttnFn.apply(lowp(qkv), bias, frames, n_per_frame, heads, m), None
    return _DividedAttnFn.apply(lowp(qkv), bias, frames, n_per_frame, heads, m)


class _ClsAttnFn(torch.autograd.Function):
    """out[b] = attention of the cls query over all tokens (lvl_cls_attn_fwd / _bwd). `bias`: the qkv Linear's bias
    (its q third was added to `q`, its k | v thirds to `kv` by the caller's Linears on detached slices); its gradient
    follows from the softmax identities of _qkv_bias_grad: sum_j dk_j = 0, sum_j dv_j = dout, plus sum_b dq."""

    @staticmethod
    def forward(ctx, q, kv, bias, heads):
        q, kv = q.contiguous(), kv.contiguous()
        C.require_device(q, kv)
        B, T, D2 = kv.shape
        D = D2 // 2
        if D != heads * 64 or tuple(q.shape) != (B, D):
            raise C.HipExtensionError(f'cls attention: q {tuple(q.shape)} / kv {tuple(kv.shape)} inconsistent with '
                                      f'heads={heads} (head dim must be 64)')
        out = torch.empty(B, D, dtype=kv.dtype, device=kv.device)
        lse = torch.empty(B, heads, dtype=torch.float32, device=kv.device)
        C.check(C.lib().lvl_cls_attn_fwd(C.ptr(q), C.ptr(kv), C.ptr(out), C.ptr(lse), B, T, heads, C.dtype_code(kv),
                                         C.stream_ptr()), 'lvl_cls_attn_fwd')
        ctx.save_for_backward(q, kv, out, lse)
        ctx.cfg = (heads, q.dtype, None if bias is None else bias.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, kv, out, lse = ctx.saved_tensors
        heads, qdt, bdt = ctx.cfg
        B, T, D2 = kv.shape
        dout = dout.contiguous()
        dq = torch.empty(B, D2 // 2, dtype=torch.float32, device=kv.device)
        dkv = torch.empty_like(kv)
        C.check(C.lib().lvl_cls_attn_bwd(C.ptr(q), C.ptr(kv), C.ptr(out), C.ptr(dout), C.ptr(lse), C.ptr(dq), C.ptr(dkv),
                                         B, T, heads, C.dtype_code(kv), C.stream_ptr()), 'lvl_cls_attn_bwd')
        db = None
        if bdt is not None and ctx.needs_input_grad[2]:
            zero = dq.new_zeros(D2 // 2)
            db = torch.cat([dq.sum(0), zero, dout.sum(0, dtype=torch.float32)]).to(bdt)
        return dq.to(qdt), dkv, db, None


def cls_attention(q, kv, heads, bias=None):
    """q [B, D] (cls rows), kv [B, T, 2D] -> [B, D]; see _ClsAttnFn."""
    q, kv = lowp(q), lowp(kv)
    if q.dtype != kv.dtype:
        q = q.to(kv.dtype)
    return _ClsAttnFn.apply(q, kv, bias, heads)


class _CausalAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, bias, heads):
        qkv = qkv.contiguous()
        C.require_device(qkv)
        B, L, D3 = qkv.shape
        D = D3 // 3
        if D != heads * 64:
            raise C.HipExtensionError(f'causal attention: width {D} != heads*64 ({heads} heads)')
        if qkv.dtype == torch.bfloat16 and not C.lib().lvl_attention_fast_path(2, 1, L, heads):
            warn_once(('attn', 2, L), f'causal attention over {L} tokens runs on the generic (slow) kernels')
        out = torch.empty(B, L, D, dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty(B, heads, L, dtype=torch.float32, device=qkv.device)
        C.check(C.lib().lvl_causal_attn_fwd(C.ptr(qkv), C.ptr(out), C.ptr(lse), B, L, heads, C.dtype_code(qkv),
                                            C.stream_ptr()), 'lvl_causal_attn_fwd')
        ctx.save_for_backward(qkv, out, lse)
        ctx.cfg = (B, L, heads, None if bias is None else bias.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        B, L, H, bdt = ctx.cfg
        dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        ws = C.workspace('causal_attn_bwd', B * H, L, qkv.device)
        C.check(C.lib().lvl_causal_attn_bwd(C.ptr(qkv), C.ptr(out), C.ptr(dout), C.ptr(lse), C.ptr(dqkv), C.ptr(ws),
                                            B, L, H, C.dtype_code(qkv), C.stream_ptr()), 'lvl_causal_attn_bwd')
        db = _qkv_bias_grad(dqkv, dout, bdt) if (bdt is not None and ctx.needs_input_grad[1]) else None
        return dqkv, db, None


def causal_attention(qkv, heads, bias=None):
    """bias: the in_proj bias that produced qkv (see _DividedAttnFn)."""
    return _CausalAttnFn.apply(lowp(qkv), bias, heads)


class _KeymaskAttnFn(torch.autograd.Function):
    """lvl_keymask_attn_fwd / _bwd on three separate tensors: q [B, Lq, D] (Lq query rows per sample; Lq = 1 is the row-0
    form), k / v [B, Tk, D], keymask uint8 [B, Tk] (non-zero = visible) or None.
    drop = (idx_qrep, seed, site, p): dropout on the probabilities (lvl_keymask_attn_drop_fwd / _bwd). No mask is saved: the
    backward regenerates it from ctx.drop; idx_qrep = query rows per sample of the FULL call, so that the row-0 form (Lq = 1,
    idx_qrep = L) draws the mask elements of row 0 of the full call."""

    @staticmethod
    def forward(ctx, q, k, v, keymask, heads, drop=None):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        C.require_device(q, k, v, keymask)
        B, Tk, D = k.shape
        if D != heads * 64:
            raise C.HipExtensionError(f'key-masked attention: width {D} != heads*64 ({heads} heads)')
        if q.shape[0] != B or q.shape[-1] != D or v.shape != k.shape or q.dtype != k.dtype or v.dtype != k.dtype:
            raise C.HipExtensionError(f'key-masked attention: q {tuple(q.shape)} {q.dtype}, k {tuple(k.shape)} {k.dtype}, '
                                      f'v {tuple(v.shape)} {v.dtype} do not belong together')
        if keymask is not None and (keymask.dtype != torch.uint8 or tuple(keymask.shape) != (B, Tk)):
            raise C.HipExtensionError(f'key-masked attention: the mask must be uint8 [{B}, {Tk}]')
        qrep = q.numel() // (B * D) if B else 1
        out = torch.empty_like(q)
        ctx.fwd, ctx.bwd, ctx.drop = 'lvl_keymask_attn_fwd', 'lvl_keymask_attn_bwd', ()
        if drop is not None:
            idx_qrep, seed, site, p = drop
            ctx.fwd, ctx.bwd = 'lvl_keymask_attn_drop_fwd', 'lvl_keymask_attn_drop_bwd'
            ctx.drop = (int(idx_qrep), int(seed), int(site), float(p))
        C.check(getattr(C.lib(), ctx.fwd)(C.ptr(q), C.ptr(k), C.ptr(v), C.ptr(keymask), C.ptr(out), B, qrep, Tk, heads, D, D,
                                          Tk * D, Tk, *ctx.drop, C.dtype_code(q), C.stream_ptr()), ctx.fwd)
        ctx.save_for_backward(q, k, v)
        ctx.keymask = keymask                  # a byte mask (no gradient, not an output): kept as a plain attribute
        ctx.cfg = (B, qrep, Tk, heads, D)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v = ctx.saved_tensors
        B, qrep, Tk, H, D = ctx.cfg
        dout = dout.contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ws = C.workspace('keymask_attn_bwd', B * qrep * H, Tk, q.device)
        C.check(getattr(C.lib(), ctx.bwd)(C.ptr(q), C.ptr(k), C.ptr(v), C.ptr(ctx.keymask), C.ptr(dout), C.ptr(dq), C.ptr(dk),
                                          C.ptr(dv), C.ptr(ws), B, qrep, Tk, H, D, D, Tk * D, Tk, *ctx.drop, C.dtype_code(q),
                                          C.stream_ptr()), ctx.bwd)
        return dq, dk, dv, None, None, None


def keymask_attention(q, k, v, keymask, heads, drop=None):
    """Bidirectional attention whose keys are hidden per sample (DistilBERT under an attention_mask): softmax over the
    visible keys of each sample, exact zeros for hidden ones; keymask uint8 [B, Tk], non-zero = visible, None = all.
    drop = (idx_qrep, seed, site, p): dropout p on the probabilities, mask element ((((b * heads + h) * idx_qrep + i) << s) | j
    of (seed, site) -- include/lavila_hip.h, the text tower's mask contract."""
    return _KeymaskAttnFn.apply(lowp(q), lowp(k), lowp(v), keymask, heads, drop)


def add_ln_fwd_raw(res, y, gate, gamma, beta, eps, drop=None, row_index_stride=None):
    """One add + LayerNorm forward on contiguous rows: s = res + gate * y (gate: one f32 on the device, None = 1; y None =
    no add), h = LayerNorm(s) -> (s or None without y, h, mean, rstd). drop None: lvl_gated_add_layernorm_train.
    drop = (seed, site, p): dropout on y, lvl_gated_add_layernorm_train_drop, or with a row_index_stride (and no gate)
    lvl_dropout_add_layernorm_fwd."""
    C.require_device(res, y, gamma, beta)
    rows, D = _rows_cols(res)
    s = torch.empty_like(res) if y is not None else None
    h = torch.empty_like(res)
    mean = torch.empty(rows, dtype=torch.float32, device=res.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=res.device)
    mid = (C.ptr(gamma), C.ptr(beta), float(eps), C.ptr(s), C.ptr(h), C.ptr(mean), C.ptr(rstd), rows, D)
    end = (C.dtype_code(res), C.stream_ptr())
    if drop is None:
        name, args = 'lvl_gated_add_layernorm_train', (C.ptr(gate), *mid, *end)
    elif row_index_stride is None:
        name, args = 'lvl_gated_add_layernorm_train_drop', (C.ptr(gate), *mid, *drop, *end)
    else:
        name, args = 'lvl_dropout_add_layernorm_fwd', (*mid, row_index_stride, *drop, *end)
    C.check(getattr(C.lib(), name)(C.ptr(res), C.ptr(y), *args), name)
    return s, h, mean, rstd


def add_ln_bwd_raw(dh, s, y, gate, gamma, mean, rstd, dadd, drop=None, row_index_stride=None):
    """The backward of add_ln_fwd_raw from its kept sum and statistics -> (ds, dy, dgamma, dbeta, dgate): lvl_gated_add_
    layernorm_bwd, _bwd_drop or lvl_dropout_add_layernorm_bwd. dgate is None without a gate; dy is None for an ungated add
    without dropout (it is ds)."""
    rows, D = _rows_cols(s)
    ds = torch.empty_like(s)
    dy =torch.empty_like(s) if (gate is not None or drop is not None) else None
    dgamma = torch.empty(D, dtype=torch.float32, device=s.device)
    dbeta = torch.empty(D, dtype=torch.float32, device=s.device)
    dgate = torch.empty(1, dtype=torch.float32, device=s.device) if gate is not None else None
    ws = C.workspace('gated_add_layernorm_bwd', rows, D, s.device)
    stats = (C.ptr(gamma), C.ptr(mean), C.ptr(rstd), C.ptr(dadd), C.ptr(ds), C.ptr(dy), C.ptr(dgamma), C.ptr(dbeta))
    end = (C.dtype_code(s), C.stream_ptr())
    if row_index_stride is not None:
        name, args = 'lvl_dropout_add_layernorm_bwd', (*stats, C.ptr(ws), rows, D, row_index_stride, *drop, *end)
    else:
        name = 'lvl_gated_add_layernorm_bwd' if drop is None else 'lvl_gated_add_layernorm_bwd_drop'
        args = (C.ptr(y), C.ptr(gate), *stats, C.ptr(dgate), C.ptr(ws), rows, D, *(drop or ()), *end)
    C.check(getattr(C.lib(), name)(C.ptr(dh), C.ptr(s), *args), name)
    return ds, dy, dgamma, dbeta, dgate


class _DropoutAddLnFn(torch.autograd.Function):
    """h = LayerNorm(res + (keep ? scale : 0) * y) (lvl_dropout_add_layernorm_fwd / _bwd; DistilBERT's FFN site). The kept sum
    and the row statistics are saved, the mask is regenerated from ctx.drop = (row_index_stride, seed, site, p)."""

    @staticmethod
    def forward(ctx, res, y, gamma, beta, eps, row_index_stride, seed, site, p):
        res, y = res.contiguous(), y.contiguous()
        g = _f32(gamma)
        ctx.drop = (int(row_index_stride), int(seed), int(site), float(p))
        s, h, mean, rstd = add_ln_fwd_raw(res, y, None, g, _f32(beta), eps, ctx.drop[1:], ctx.drop[0])
        ctx.save_for_backward(s, g, mean, rstd)
        ctx.pdt = (gamma.dtype, beta.dtype)
        return h

    @staticmethod
    def backward(ctx, dh):
        s, g, mean, rstd = ctx.saved_tensors
        ds, dy, dgamma, dbeta, _ = add_ln_bwd_raw(dh.contiguous(), s, None, None, g, mean, rstd, None, ctx.drop[1:], ctx.drop[0])
        return (ds, dy, *_param_grads(ctx.pdt, dgamma, dbeta), None, None, None, None, None)


def dropout_add_layer_norm(res, y, weight, bias, eps, row_index_stride, seed, site, p):
    """LayerNorm(res + dropout(y)): mask element row * row_index_stride + col of (seed, site); row_index_stride is the width
    when the call holds all rows of the site, L * width when it holds row 0 of every sample."""
    res = lowp(res)
    if res.dtype not in (torch.float32, torch.bfloat16):
        raise C.HipExtensionError(f'dropout_add_layer_norm is built for float32 and bfloat16 rows, got {res.dtype}')
    return _narrow(_DropoutAddLnFn.apply(res, y.to(res.dtype), weight, bias, eps, row_index_stride, seed, site, p))


# --------------------------------------------------------------------------------------------------
# contrastive head (raw kernels; the autograd wrapper + collectives live in lavila_amd/loss.py)
# --------------------------------------------------------------------------------------------------
def clip_loss_fwd_raw(img_all, txt_all, scale, B: int, row0: int, want_logits=False):
    """scale: 0-dim/1-elem float32 DEVICE tensor (exp(logit_scale)); no host sync."""
    C.require_device(img_all, txt_all, scale)
    G, E = img_all.shape
    dev = img_all.device
    stats = torch.empty(2, B, 4, dtype=torch.float32, device=dev)
    argmax = torch.empty(2, B, dtype=torch.int32, device=dev)
    logits = torch.empty(2, B, G, dtype=torch.float32, device=dev) if want_logits else None
    C.check(C.lib().lvl_clip_loss_fwd(C.ptr(img_all), C.ptr(txt_all), C.ptr(scale), B, G, E, row0, C.ptr(stats),
                                      C.ptr(argmax), C.ptr(logits), C.dtype_code(img_all), C.stream_ptr()),
            'lvl_clip_loss_fwd')
    return stats, argmax, logits


def clip_loss_bwd_raw(img_all, txt_all, lse_all, scale, upstream, coef: float, B: int, row0: int,
                      rows_only: bool = False):
    C.require_device(img_all, txt_all, lse_all, scale, upstream)
    G, E = img_all.shape
    dimg = torch.empty(B, E, dtype=torch.float32, device=img_all.device)
    dtxt = torch.empty(B, E, dtype=torch.float32, device=img_all.device)
    C.check(C.lib().lvl_clip_loss_bwd(C.ptr(img_all), C.ptr(txt_all), C.ptr(lse_all), C.ptr(scale), C.ptr(upstream),
                                      float(coef), B, G, E, row0, int(rows_only), C.ptr(dimg), C.ptr(dtxt),
                                      C.dtype_code(img_all),
                                      C.stream_ptr()), 'lvl_clip_loss_bwd')
    return dimg, dtxt


def ssl_clip_loss_fwd_raw(img_all, txt_all, ind_all, scales3, B: int, row0: int, want_logits=False):
    """ind_all: [G] int32 device tensor; scales3: [3] float32 device tensor {pseudo, sqrt(pseudo*real), real}."""
    C.require_device(img_all, txt_all, ind_all, scales3)
    G, E = img_all.shape
    dev = img_all.device
    stats = torch.empty(2, B, 8, dtype=torch.float32, device=dev)
    argmax = torch.empty(2, B, dtype=torch.int32, device=dev)
    logits = torch.empty(2, B, G, dtype=torch.float32, device=dev) if want_logits else None
    C.check(C.lib().lvl_ssl_clip_loss_fwd(C.ptr(img_all), C.ptr(txt_all), C.ptr(ind_all), C.ptr(scales3), B, G, E, row0,
                                          C.ptr(stats), C.ptr(argmax), C.ptr(logits), C.dtype_code(img_all),
                                          C.stream_ptr()), 'lvl_ssl_clip_loss_fwd')
    return stats, argmax, logits


def ssl_clip_loss_bwd_raw(img_all, txt_all, ind_all, lse_all, scales3, upstream, coef: float, B: int, row0: int):
    C.require_device(img_all, txt_all, ind_all, lse_all, scales3, upstream)
    G, E = img_all.shape
    dimg = torch.empty(B, E, dtype=torch.float32, device=img_all.device)
    dtxt = torch.empty(B, E, dtype=torch.float32, device=img_all.device)
    C.check(C.lib().lvl_ssl_clip_loss_bwd(C.ptr(img_all), C.ptr(txt_all), C.ptr(ind_all), C.ptr(lse_all),
                                          C.ptr(scales3), C.ptr(upstream), float(coef), B, G, E, row0, C.ptr(dimg),
                                          C.ptr(dtxt), C.dtype_code(img_all), C.stream_ptr()), 'lvl_ssl_clip_loss_bwd')
    return dimg, dtxt


# --------------------------------------------------------------------------------------------------
# max-margin ranking losses of the retrieval fine-tune (raw kernels; autograd + collectives in lavila_amd/loss.py)
# --------------------------------------------------------------------------------------------------
def margin_loss_prepare_raw(img_all, txt_all, weight_all, margin: float):
    """weight_all: [G] float32 device tensor or None (every weight 1). Returns prep [7,G] f32 =
    {1/max(|img|,1e-8), 1/max(|txt|,1e-8), d, c, m, max(|img|,1e-8), max(|txt|,1e-8)}."""
    C.require_device(img_all, txt_all, weight_all)
    G, E = img_all.shape
    prep = torch.empty(7, G, dtype=torch.float32, device=img_all.device)
    C.check(C.lib().lvl_margin_loss_prepare(C.ptr(img_all), C.ptr(txt_all), C.ptr(weight_all), float(margin), G, E,
                                            C.ptr(prep), C.dtype_code(img_all), C.stream_ptr()),
            'lvl_margin_loss_prepare')
    return prep


def margin_loss_fwd_raw(img_all, txt_all, prep, B: int, row0: int, with_diag: bool):
    """hinge [2,B] f32 (per direction and local row: sum of its hinge terms), count [2,B] int32 (its active terms)."""
    C.require_device(img_all, txt_all, prep)
    G, E = img_all.shape
    hinge = torch.empty(2, B, dtype=torch.float32, device=img_all.device)
    count = torch.empty(2, B, dtype=torch.int32, device=img_all.device)
    C.check(C.lib().lvl_margin_loss_fwd(C.ptr(img_all), C.ptr(txt_all), C.ptr(prep), B, G, E, row0, int(with_diag),
                                        C.ptr(hinge), C.ptr(count), C.dtype_code(img_all), C.stream_ptr()),
            'lvl_margin_loss_fwd')
    return hinge, count


def margin_loss_bwd_raw(img_all, txt_all, prep, upstream, coef: float, B: int, row0: int):
    """coef * upstream * d(sum of all hinge terms)/d(raw local rows): dimg, dtxt [B,E] f32."""
    C.require_device(img_all, txt_all, prep, upstream)
    G, E = img_all.shape
    dimg = torch.empty(B, E, dtype=torch.float32, device=img_all.device)
    dtxt = torch.empty(B, E, dtype=torch.float32, device=img_all.device)
    C.check(C.lib().lvl_margin_loss_bwd(C.ptr(img_all), C.ptr(txt_all), C.ptr(prep), C.ptr(upstream), float(coef), B, G,
                                        E, row0, C.ptr(dimg), C.ptr(dtxt), C.dtype_code(img_all), C.stream_ptr()),
            'lvl_margin_loss_bwd')
    return dimg, dtxt


# --------------------------------------------------------------------------------------------------
# vocabulary cross-entropy of the narrator's criterion (raw kernels; autograd + layouts in lavila_amd/loss.py)
# --------------------------------------------------------------------------------------------------
def _token_rows(logits, labels, *more):
    """logits: a [rows, vocab] float32 / bfloat16 VIEW with class stride 1 and any row stride >= vocab (rows need not be
    contiguous or 16-byte aligned); labels: [rows] int64 with any stride. Returns (rows, vocab)."""
    for t in (logits, labels) + more:
        if t is not None and not t.is_cuda:
            raise C.HipExtensionError('lavila_amd: tensor on %s -- the HIP kernels need a ROCm device tensor; there is '
                                      'no CPU fallback' % t.device)
    C.require_device(*more)
    if logits.device.index != torch.cuda.current_device() or labels.device != logits.device:
        raise C.HipExtensionError(f'lavila_amd: logits on {logits.device}, labels on {labels.device}, current device '
                                  f'cuda:{torch.cuda.current_device()}')
    if logits.dim() != 2 or labels.dim() != 1 or labels.shape[0] != logits.shape[0] or labels.dtype != torch.int64:
        raise C.HipExtensionError(f'token_xent: logits {tuple(logits.shape)} / labels {tuple(labels.shape)} '
                                  f'{labels.dtype}: want [rows, vocab] and [rows] int64')
    rows, vocab = logits.shape
    if vocab < 1 or (rows > 0 and logits.stride(1) != 1) or (rows > 1 and logits.stride(0) < vocab):
        raise C.HipExtensionError(f'token_xent: logits strides {logits.stride()} for shape {tuple(logits.shape)}: the '
                                  'class stride must be 1 and the row stride at least vocab')
    return rows, vocab


def _out_buffer(out, shape, dtype, device):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device or not out.is_contiguous():
        raise C.HipExtensionError(f'out= buffer {tuple(out.shape)} {out.dtype}: want contiguous {tuple(shape)} {dtype}')
    return out


def token_xent_fwd_raw(logits, labels, pad_id: int, out=None):
    """One pass over each row. Returns (lse f32, nll f32, pred i32, correct i32, counted i32), each [rows]; `out`: an
    optional tuple of five such buffers to write into."""
    rows, vocab = _token_rows(logits, labels)
    dev = logits.device
    kinds = (torch.float32, torch.float32, torch.int32, torch.int32, torch.int32)
    bufs = tuple(_out_buffer(None if out is None else out[k], (rows,), kinds[k], dev) for k in range(5))
    C.check(C.lib().lvl_token_xent_fwd(C.ptr(logits), logits.stride(0) if rows > 1 else vocab, C.ptr(labels),
                                       labels.stride(0) if rows > 1 else 1, rows, vocab, int(pad_id),
                                       *(C.ptr(b) for b in bufs), C.dtype_code(logits), C.stream_ptr()),
            'lvl_token_xent_fwd')
    return bufs


def token_xent_reduce_raw(nll, correct, counted, B: int, T: int, out=None):
    """[3] f32 = {loss = sum(nll)/(B*T), caption_acc, ppl} from the per-row results, in a fixed summation order."""
    C.require_device(nll, correct, counted)
    if nll.numel() != B * T or correct.numel() != B * T or counted.numel() != B * T:
        raise C.HipExtensionError(f'token_xent_reduce: {nll.numel()} rows for B={B} T={T}')
    res = _out_buffer(out, (3,), torch.float32, nll.device)
    C.check(C.lib().lvl_token_xent_reduce(C.ptr(nll), C.ptr(correct), C.ptr(counted), B, T, C.ptr(res), C.stream_ptr()),
            'lvl_token_xent_reduce')
    return res


def token_xent_bwd_raw(logits, labels, lse, upstream, coef: float, pad_id: int, out=None):
    """coef * upstream * d(sum of nll)/d(logits) in the logits' dtype: [rows, Vp], Vp = vocab rounded up to 8; pad rows
    and the columns [vocab, Vp) are zeros, rows with an out-of-range label NaN. Every element is written."""
    rows, vocab = _token_rows(logits, labels, lse, upstream)
    grad = _out_buffer(out, (rows, (vocab + 7) // 8 * 8), logits.dtype, logits.device)
    C.check(C.lib().lvl_token_xent_bwd(C.ptr(logits), logits.stride(0) if rows > 1 else vocab, C.ptr(labels),
                                       labels.stride(0) if rows > 1 else 1, C.ptr(lse), C.ptr(upstream), float(coef),
                                       rows, vocab, int(pad_id), C.ptr(grad), C.dtype_code(logits), C.stream_ptr()),
            'lvl_token_xent_bwd')
    return grad
