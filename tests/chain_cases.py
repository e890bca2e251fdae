"""The case matrix of the fused residual chain: every route through SpaceTimeBlock / SpaceTimeTransformer, the OpenAI
image and text towers and the DistilBERT tower that closes a pending residual add, on towers as small as the kernels allow
while still taking the benched routes (width 256: lvl_linear_tn with the residual epilogue, the fused MLP).

CASES maps a name to its specification; run(name) builds (once) the tower, runs one forward and -- where the output carries a
graph -- one backward of `sum(out * cot)`, and returns the output, the loss, every gradient and (count_saved) the bytes kept
for backward. tests/test_gpu_chain_call_plans.py compares the C-ABI calls of every case with the recorded plans of
tests/golden/chain_call_plans.json (tools/gen_chain_call_plans.py); tools/ab_chain_outputs.py compares the numbers of two
trees bit for bit."""
import contextlib
import io

import torch
import torch.nn as nn

DEV = 'cuda'
BF = torch.bfloat16
FRAMES, IMG, PATCH, BATCH = 2, 32, 16, 2          # 2 frames of 2 x 2 patches + cls: 9 tokens per sample
CONTEXT, TEXT_BATCH, EOT_ROWS = 8, 3, (2, 5, 7)

CASES = {}


def _video(name, **spec):
    base = dict(kind='video', width=256, depth=3, act='quick', gating=False, rate=0.0, ckpt=False, cls=True, cls_only=True,
                f32_stream=False, amp=True, train=True)
    assert not set(spec) - set(base), spec
    CASES[name] = {**base, **spec}


MODES = {'plain': False, 'block': 'block', 'selective': 'selective'}
for _m, _ck in MODES.items():
    for _cls in (True, False):
        _t = 'cls' if _cls else 'all'
        _video(f'video {_m} {_t}', ckpt=_ck, cls=_cls)
        # stochastic depth: blocks 1 and 2 drop (rates 0, 0.25, 0.5)
        _video(f'video {_m} {_t} drop-path', ckpt=_ck, cls=_cls, rate=0.5)
        # depth 2: the last block is stochastic, in the selective mode behind a deferred MLP; depth 1: rate 0 after all
        _video(f'video {_m} {_t} drop-path depth 2', ckpt=_ck, cls=_cls, rate=0.5, depth=2)
    _video(f'video {_m} cls drop-path depth 1', ckpt=_ck, rate=0.5, depth=1)
    _video(f'video {_m} cls gelu', ckpt=_ck, act='gelu')
    _video(f'video {_m} all gelu', ckpt=_ck, act='gelu', cls=False)
    _video(f'video {_m} cls unclassified act', ckpt=_ck, act='tanh')
    _video(f'video {_m} all unclassified act drop-path', ckpt=_ck, act='tanh', cls=False, rate=0.5)
    _video(f'video {_m} cls tanh gating', ckpt=_ck, gating=True)
    _video(f'video {_m} cls tanh gating drop-path', ckpt=_ck, gating=True, rate=0.5)
    _video(f'video {_m} cls whole last block', ckpt=_ck, cls_only=False)
    _video(f'video {_m} cls float32', ckpt=_ck, amp=False)
    _video(f'video {_m} cls width 192', ckpt=_ck, width=192)
for _m in ('plain', 'block'):           # (the selective mode refuses the float32 stream)
    _video(f'video {_m} cls f32 stream', ckpt=MODES[_m], f32_stream=True)
    _video(f'video {_m} all f32 stream drop-path', ckpt=MODES[_m], f32_stream=True, cls=False, rate=0.5)
_video('video eval cls', train=False)
_video('video eval all', train=False, cls=False)
_video('video eval cls drop-path gelu', train=False, rate=0.5, act='gelu')

# the reference-signature forward of one block: blocks[0] never drops, blocks[2] does (rate 0.5)
for _m, _ck in MODES.items():
    CASES[f'video block forward {_m}'] = dict(kind='video_block', block=0, ckpt=_ck, rate=0.5, gating=False)
    CASES[f'video block forward {_m} drop-path'] = dict(kind='video_block', block=2, ckpt=_ck, rate=0.5, gating=False)
CASES['video block forward plain tanh gating'] = dict(kind='video_block', block=0, ckpt=False, rate=0.0, gating=True)

for _ck in (False, 'block'):
    _t = 'block' if _ck else 'plain'
    CASES[f'image {_t} cls'] = dict(kind='image', ckpt=_ck, cls=True)
    CASES[f'image {_t} all'] = dict(kind='image', ckpt=_ck, cls=False)                      # final_ln None
    CASES[f'image {_t} tokens ln'] = dict(kind='tower', mask=False, ckpt=_ck, rows=None, ln=True)
    CASES[f'text {_t} eot rows'] = dict(kind='tower', mask=True, ckpt=_ck, rows='eot', ln=True)
    CASES[f'text {_t} every row'] = dict(kind='tower', mask=True, ckpt=_ck, rows=None, ln=True)
    CASES[f'text {_t} no final ln'] = dict(kind='tower', mask=True, ckpt=_ck, rows=None, ln=False)
CASES['image plain cls whole last block'] = dict(kind='image', ckpt=False, cls=True, cls_only=False)
CASES['text plain eot rows whole last block'] = dict(kind='tower', mask=True, ckpt=False, rows='eot', ln=True, cls_only=False)
CASES['text plain eot rows float32'] = dict(kind='tower', mask=True, ckpt=False, rows='eot', ln=True, amp=False)
CASES['image plain cls f32 stream'] = dict(kind='image', ckpt=False, cls=True, f32_stream=True)
CASES['text reference forward'] = dict(kind='tower_forward', mask=True)
CASES['text block reference forward'] = dict(kind='tower_forward', mask=True, block=1)
CASES['image block reference forward'] = dict(kind='tower_forward', mask=False, block=1)

for _entry in ('forward', 'first_rows'):
    CASES[f'distilbert {_entry} eval'] = dict(kind='distilbert', entry=_entry, train=False, drop=False)
    CASES[f'distilbert {_entry} train dropout'] = dict(kind='distilbert', entry=_entry, train=True, drop=True)
    CASES[f'distilbert {_entry} train'] = dict(kind='distilbert', entry=_entry, train=True, drop=False)
CASES['distilbert first_rows eval float32'] = dict(kind='distilbert', entry='first_rows', train=False, drop=False, amp=False)
CASES['distilbert first_rows whole last layer'] = dict(kind='distilbert', entry='first_rows', train=True, drop=False,
                                                       cls_only=False)
CASES['distilbert layer forward'] = dict(kind='distilbert_layer')


def bf16_own_gemm_cases():
    """The cases whose Linears must be on lvl_linear_tn with the residual epilogue: bf16 at width 256."""
    def no_projection_epilogue(s):
        # a stochastic block adds its space branch in the scaled LayerNorm kernel, the cls-only block on B rows: the lone block
        # of the depth-1 tower and blocks[2] of the drop-path tower have no residual epilogue to show
        return (s['kind'] == 'video' and s['depth'] == 1 and s['cls']) or (s['kind'] == 'video_block' and s['block'] == 2)
    return [n for n, s in CASES.items() if s.get('amp', True) and s.get('width', 256) == 256
            and not s.get('f32_stream', False) and not no_projection_epilogue(s)]


def deferred_mlp_cases():
    """The cases in which a block's MLP waits for the next block's first LayerNorm (the fused MLP's residual call): the plain
    and the selective video step of more than one block in bf16, without stochastic depth in the plain one, with a classified
    activation."""
    out = []
    for n, s in CASES.items():
        if s['kind'] != 'video' or n not in bf16_own_gemm_cases() or s['depth'] < 2 or s['act'] == 'tanh':
            continue
        if (s['ckpt'] is False and (s['rate'] == 0.0 or not s['train'])) or s['ckpt'] == 'selective':
            out.append(n)
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
_models = {}


def _fill(module, seed):
    """Weights of a trained model's scale: matrices N(0, 0.02), LayerNorm weights around 1, biases around 0."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            if p.ndim > 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
            else:
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    return module.to(DEV)


def _cached(key, make):
    if key not in _models:
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            _models[key] = _fill(make(), 1)
    return _models[key]


def _randn(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV, dtype)


class _TanhGELU(nn.GELU):
    """An activation classify_act does not know: it runs as the module it is, between two Linear kernels."""

    def __init__(self):
        super().__init__(approximate='tanh')


def _video_tower(s):
    from lavila_amd.openai_model import QuickGELU
    from lavila_amd.timesformer import SpaceTimeTransformer
    width, depth = s.get('width', 256), s.get('depth', 3)
    act = {'quick': QuickGELU, 'gelu': nn.GELU, 'tanh': _TanhGELU}[s.get('act', 'quick')]
    return _cached(('video', width, depth, s.get('act', 'quick'), s['gating'], s['rate']),
                   lambda: SpaceTimeTransformer(img_size=IMG, patch_size=PATCH, embed_dim=width, depth=depth,
                                                num_heads=width // 64, num_frames=FRAMES, time_init='rand',
                                                attention_style='frozen-in-time', ln_pre=True, act_layer=act, num_classes=0,
                                                drop_path_rate=s['rate'], is_tanh_gating=s['gating']))


def _causal_mask():
    return torch.full((CONTEXT, CONTEXT), float('-inf')).triu_(1)


def _setup(s):
    """(module that owns the parameters, callable -> output, leaf inputs {name: tensor})."""
    from lavila_amd import distilbert as DB
    from lavila_amd import openai_model as OA
    from lavila_amd.timesformer import LayerNorm
    kind, leaves = s['kind'], {}
    if kind == 'video':
        vis = _video_tower(s)
        clip = _randn((BATCH, FRAMES, 3, IMG, IMG), 3)
        return vis, (lambda: vis.forward_features(clip, use_checkpoint=s['ckpt'], cls_at_last=s['cls'])), leaves
    if kind == 'video_block':
        vis = _video_tower(dict(s, width=256, depth=3, act='quick'))
        blk = vis.blocks[s['block']]
        x = leaves['x'] = _randn((BATCH, 1 + FRAMES * 4, 256), 5, BF).requires_grad_(True)
        return blk, (lambda: blk(x, 'b (f n) d', '(b f) n d', 'b (f n) d', '(b n) f d', 4, FRAMES, use_checkpoint=s['ckpt'])), \
            leaves
    if kind == 'image':
        vit = _cached(('image',), lambda: OA.VisionTransformer(IMG, PATCH, 256, 3, 4, 128))
        images = _randn((BATCH, 3, IMG, IMG), 7)
        return vit, (lambda: vit(images, use_checkpoint=s['ckpt'], cls_at_last=s['cls'])), leaves
    if kind in ('tower', 'tower_forward'):
        masked = s['mask']
        tower = _cached(('tower', masked), lambda: nn.ModuleDict(dict(
            t=OA.Transformer(256, 3, 4, _causal_mask() if masked else None), ln=LayerNorm(256))))
        dtype = BF if s.get('amp', True) else torch.float32
        if kind == 'tower_forward':         # [L, N, D], the reference's layout
            x = leaves['x'] = _randn((CONTEXT if masked else 5, TEXT_BATCH, 256), 9, dtype).requires_grad_(True)
            mod = tower['t'] if 'block' not in s else tower['t'].resblocks[s['block']]
            return mod, (lambda: mod(x)), leaves
        x = leaves['x'] = _randn((TEXT_BATCH, CONTEXT if masked else 5, 256), 9, dtype).requires_grad_(True)
        rows = torch.tensor(EOT_ROWS, device=DEV) if s['rows'] == 'eot' else s['rows']
        ln = tower['ln'] if s['ln'] else None
        return tower, (lambda: tower['t'].forward_batch_major(x, ln, use_checkpoint=s['ckpt'], rows=rows)), leaves
    p = 0.1 if s.get('drop') else 0.0
    bert = _cached(('distilbert', p), lambda: DB.DistilBertModel(DB.distilbert_config(
        vocab_size=512, max_position_embeddings=16, dim=256, n_heads=4, n_layers=2, hidden_dim=1024, dropout=p,
        attention_dropout=p)))
    keymask = (torch.arange(CONTEXT)[None, :] < torch.tensor([[8], [5], [3]])).to(DEV)
    if kind == 'distilbert_layer':
        layer = bert.transformer.layer[0]
        x = leaves['x'] = _randn((TEXT_BATCH, CONTEXT, 256), 11, BF).requires_grad_(True)
        return layer, (lambda: layer(x, keymask.to(torch.uint8).contiguous())), leaves
    ids = torch.randint(1, 512, (TEXT_BATCH, CONTEXT), generator=torch.Generator().manual_seed(13)).to(DEV)
    if s['entry'] == 'forward':
        return bert, (lambda: bert(ids, attention_mask=keymask).last_hidden_state), leaves
    return bert, (lambda: bert.first_rows(ids, attention_mask=keymask)), leaves


@contextlib.contextmanager
def _switches(s):
    """The module-level switches a case sets, put back afterwards."""
    from lavila_amd import distilbert, gpt2_gated, ops, timesformer
    old = (timesformer.CLS_ONLY_LAST_BLOCK, ops.RESIDUAL_F32, distilbert.TEXT_DROPOUT)
    timesformer.CLS_ONLY_LAST_BLOCK = s.get('cls_only', True)
    ops.RESIDUAL_F32 = s.get('f32_stream', False)
    distilbert.TEXT_DROPOUT = bool(s.get('drop', False))
    try:
        with gpt2_gated.fixed_dropout_seed(0x5EED) if s.get('drop') else contextlib.nullcontext():
            yield
    finally:
        timesformer.CLS_ONLY_LAST_BLOCK, ops.RESIDUAL_F32, distilbert.TEXT_DROPOUT = old


def run(name, recorder=None, count_saved=False):
    """One forward (+ backward) of the case: {'out', 'loss', 'grads': {name: tensor}, 'saved_bytes'}. recorder: a
    cabi_recorder.Recorder; its two lists then hold the calls of this forward and of this backward.
    count_saved: the bytes kept for backward, per distinct storage (saved_tensors_hooks)."""
    from lavila_amd import ops
    s = CASES[name]
    module, fn, leaves = _setup(s)
    train = s.get('train', True)
    module.train(train)
    for t in list(module.parameters()) + list(leaves.values()):
        t.grad = None
    seen, nbytes = set(), 0

    def pack(t):
        nonlocal nbytes
        st = t.untyped_storage()
        if t.is_cuda and st.data_ptr() not in seen:
            seen.add(st.data_ptr())
            nbytes += st.nbytes()
        return t
    hooks = torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t) if count_saved else contextlib.nullcontext()
    amp = torch.autocast('cuda', dtype=BF) if s.get('amp', True) else contextlib.nullcontext()
    grad = contextlib.nullcontext() if (train or s['kind'] != 'video') else torch.no_grad()
    ops.invalidate_weight_cache()
    torch.manual_seed(17)                   # the stochastic-depth masks come from the device generator
    with _switches(s):
        if recorder is not None:
            recorder.begin()
        with hooks:
            with amp, grad:
                out = fn()
            loss = None
            if out.requires_grad:
                cot = _randn(tuple(out.shape), 19) / out.numel() ** 0.5
                loss = (out.float() * cot).sum()
        if recorder is not None:
            recorder.phase_backward()
        if loss is not None:
            loss.backward()
        torch.cuda.synchronize()
        if recorder is not None:
            recorder.end()
    grads = {k: p.grad.clone() for k, p in module.named_parameters() if p.grad is not None}
    grads.update({'input.' + k: t.grad.clone() for k, t in leaves.items() if t.grad is not None})
    module.zero_grad(set_to_none=True)
    return {'out': out.detach().clone(), 'loss': None if loss is None else loss.detach().clone(), 'grads': grads,
            'saved_bytes': nbytes if count_saved else None}
