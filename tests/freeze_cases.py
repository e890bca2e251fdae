"""The `needs_input_grad` matrix of the own autograd Functions: one row per Function and path, as plain data.

Fourteen Functions of ops.py, gpt2_gated.py and models.py branch on ctx.needs_input_grad: the branches pick kernels (the `own`
decision of _LinearFn / _Conv1DFn reads needs_input_grad[0]), pick entry points (lvl_divided_attn_bwd with or without the
bias rider) and drop GEMMs, rebuilds and column-sum tokens. A row names

  * the Function, the module that defines it and the differentiable inputs of the call, in a fixed order;
  * the activation dtypes it runs in;
  * the GEMM shapes of the call with the predicate of ops.py that routes them and what it must answer (checked on the CPU);
  * the launches a run makes through the counted functions (COUNTED) as a list of conditions, one per launch:
    None -- always; 'x' -- only when input x wants a gradient; ('not', 'x') -- only when it does not;
  * `switch`: {input: kernel} -- freezing that input makes the run launch a DIFFERENT kernel for the listed results
    (`switch_results`), which are then held to the float64 bound of the Function's own test instead of bit equality.

test_gpu_freeze_ops.py builds every row (build(row, dtype) below, GPU only), runs it with every input trainable, then with
exactly one input frozen and with exactly one input trainable, and compares. test_freeze_cases_cpu.py checks the table.
"""
from dataclasses import dataclass, field

ROWS = 40                         # token rows of every GEMM case: one partial 256-row tile
COUNTED = ('_wgrad', '_wgrad_f32', 'linear_tn_raw', 'linear_tn_ragged_raw', 'layernorm_apply_raw', 'quickgelu_apply_raw',
           'vec_mat')
# where the Functions live (module file under lavila_amd/)
SOURCES = ('ops.py', 'gpt2_gated.py', 'models.py')


@dataclass
class Case:
    name: str
    function: str                 # class name of the torch.autograd.Function
    source: str                   # one of SOURCES
    inputs: tuple                 # differentiable inputs of the call
    dtypes: tuple = ('bf16',)
    gemms: tuple = ()             # (predicate of ops.py, rows, n_out, n_in, expected answer)
    launches: dict = field(default_factory=dict)
    switch: dict = field(default_factory=dict)
    switch_results: tuple = ()
    f32_launches: dict = None     # launches of the float32 run where they differ


def _own(n_out, n_in):
    return (('_tn_ok', ROWS, n_out, n_in, True), ('_tn_ok', ROWS, n_in, n_out, True))


def _own_f32(n_out, n_in):
    return (('_tn_ok_f32', ROWS, n_out, n_in, True), ('_tn_ok_f32', ROWS, n_in, n_out, True))


_MLP_BF16 = {'linear_tn_raw': [None, None, None, 'x'], '_wgrad': ['w2', 'w1']}
_MLP_F32 = {'linear_tn_raw': [None, None, None, 'x'], '_wgrad_f32': ['w2', 'w1']}
_MLP_SEL = dict(_MLP_BF16, quickgelu_apply_raw=['w2'], layernorm_apply_raw=['w1'])

CASES = [
    # ---- ops.py: Linear layers ----------------------------------------------------------------------------------------------
    Case('linear_own', '_LinearFn', 'ops.py', ('x', 'weight', 'bias'), ('bf16', 'f32'),
         gemms=_own(1024, 256) + _own_f32(1024, 256),
         launches={'linear_tn_raw': [None, 'x'], '_wgrad': ['weight']},
         f32_launches={'linear_tn_raw': [None, 'x'], '_wgrad_f32': ['weight']}),
    Case('linear_own_recipe', '_LinearFn', 'ops.py', ('x', 'weight', 'bias'), ('bf16', 'f32'),
         gemms=_own(1024, 256) + _own_f32(1024, 256),
         # x is the input of the LayerNorm whose output the Linear rebuilds: only the weight gradient reads the rebuilt rows
         launches={'linear_tn_raw': [None, 'x'], '_wgrad': ['weight'], 'layernorm_apply_raw': ['weight']},
         f32_launches={'linear_tn_raw': [None, 'x'], '_wgrad_f32': ['weight'], 'layernorm_apply_raw': ['weight']}),
    Case('linear_library_192', '_LinearFn', 'ops.py', ('x', 'weight', 'bias'), ('bf16', 'f32'),
         gemms=(('_tn_ok', ROWS, 192, 192, False), ('_tn_ok_f32', ROWS, 192, 192, False)),
         launches={'_wgrad': ['weight']}, f32_launches={'_wgrad_f32': ['weight']}),
    Case('linear_own_flip_192_to_256', '_LinearFn', 'ops.py', ('x', 'weight', 'bias'), ('bf16',),
         # the forward tiles (N = 256, K = 192), the input gradient (N = 192) does not: the layer is on the own kernels only
         # when x wants no gradient
         gemms=(('_tn_ok', ROWS, 256, 192, True), ('_tn_ok', ROWS, 192, 256, False)),
         launches={'linear_tn_raw': [('not', 'x')], '_wgrad': ['weight']},
         switch={'x': 'lvl_linear_tn (forward) where the all-trainable run uses the library GEMM'}, switch_results=('out0',)),
    Case('linear_token', '_LinearTokenFn', 'ops.py', ('x', 'weight', 'xtoken'), ('bf16',), gemms=_own(1024, 256),
         launches={'linear_tn_raw': [None, 'x'], '_wgrad': ['weight'], 'vec_mat': ['xtoken']}),
    Case('mlp', '_MlpFn', 'ops.py', ('x', 'w1', 'b1', 'w2'), ('bf16', 'f32'),
         gemms=_own(1024, 256) + _own_f32(1024, 256), launches=_MLP_BF16, f32_launches=_MLP_F32),
    Case('mlp_selective', '_MlpFn', 'ops.py', ('x', 'w1', 'b1', 'w2'), ('bf16',), gemms=_own(1024, 256), launches=_MLP_SEL),
    Case('linear_residual_ln', '_LinearResidualLayerNormFn', 'ops.py',
         ('x', 'weight', 'lbias', 'res', 'gamma', 'beta', 'xtoken'), ('bf16',), gemms=_own(256, 1024),
         launches={'linear_tn_raw': [None, 'x'], '_wgrad': ['weight'], 'vec_mat': ['xtoken']}),
    Case('linear_residual_ln_no_bias', '_LinearResidualLayerNormFn', 'ops.py', ('x', 'weight', 'res', 'gamma', 'beta', 'xtoken'),
         # without a Linear bias the token is the only reader of the LayerNorm backward's column sums
         ('bf16',), gemms=_own(256, 1024),
         launches={'linear_tn_raw': [None, 'x'], '_wgrad': ['weight'], 'vec_mat': ['xtoken']}),
    Case('mlp_residual_ln', '_MlpResidualLayerNormFn', 'ops.py', ('x', 'w1', 'b1', 'w2', 'b2', 'res', 'gamma', 'beta'),
         ('bf16',), gemms=_own(1024, 256), launches=_MLP_BF16),
    Case('mlp_residual_ln_selective', '_MlpResidualLayerNormFn', 'ops.py',
         ('x', 'w1', 'b1', 'w2', 'b2', 'res', 'gamma', 'beta'), ('bf16',), gemms=_own(1024, 256), launches=_MLP_SEL),
    # ---- ops.py: LayerNorm forms that carry a token, embedding, attention cores ---------------------------------------------------
    Case('add_ln_pass', '_AddLayerNormPassFn', 'ops.py', ('res', 'y', 'ybias', 'weight', 'bias', 'ytoken'), ('bf16', 'f32')),
    Case('scaled_add_ln', '_ScaledAddLayerNormFn', 'ops.py', ('res', 'y', 'ybias', 'weight', 'bias', 'ytoken'),
         ('bf16', 'f32')),
    Case('text_embed', '_TextEmbedFn', 'ops.py', ('table', 'pos'), ('bf16', 'f32')),
    Case('divided_space', '_DividedAttnFn', 'ops.py', ('qkv', 'bias'), ('bf16', 'f32')),
    Case('divided_time', '_DividedAttnFn', 'ops.py', ('qkv', 'bias'), ('bf16', 'f32')),
    Case('cls_attn', '_ClsAttnFn', 'ops.py', ('q', 'kv', 'bias'), ('bf16', 'f32')),
    Case('causal_attn', '_CausalAttnFn', 'ops.py', ('qkv', 'bias'), ('bf16', 'f32')),
    # ---- gpt2_gated.py: the narrator decoder -----------------------------------------------------------------------------------
    Case('conv1d_256', '_Conv1DFn', 'gpt2_gated.py', ('x', 'weight', 'bias'), ('bf16',),
         gemms=(('_tn_rows_ok', ROWS, 1024, 256, True), ('_tn_rows_ok', ROWS, 256, 1024, True)),
         launches={'linear_tn_raw': [None, 'x'], '_wgrad': ['weight']}),
    Case('conv1d_ragged_320', '_Conv1DFn', 'gpt2_gated.py', ('x', 'weight', 'bias'), ('bf16',),
         gemms=(('_tn_ok', ROWS, 320, 320, False), ('_tn_rows_ok', ROWS, 320, 320, True)),
         launches={'linear_tn_ragged_raw': [None, 'x'], '_wgrad': ['weight']}),
    Case('conv1d_flip_192_to_256', '_Conv1DFn', 'gpt2_gated.py', ('x', 'weight', 'bias'), ('bf16',),
         gemms=(('_tn_rows_ok', ROWS, 256, 192, True), ('_tn_rows_ok', ROWS, 192, 256, False)),
         launches={'linear_tn_raw': [('not', 'x')], '_wgrad': ['weight']},
         switch={'x': 'lvl_linear_tn (forward) where the all-trainable run uses the library GEMM'}, switch_results=('out0',)),
    Case('lm_head_256', '_LmHeadFn', 'gpt2_gated.py', ('h', 'weight'), ('bf16',),
         gemms=(('_tn_ok', ROWS, 512, 256, True), ('_tn_rows_ok', ROWS, 256, 512, True)),
         launches={'linear_tn_raw': [None, 'h'], '_wgrad': ['weight']}),
    Case('lm_head_ragged_320', '_LmHeadFn', 'gpt2_gated.py', ('h', 'weight'), ('bf16',),
         gemms=(('_tn_ok', ROWS, 512, 320, True), ('_tn_ok', ROWS, 320, 512, False), ('_tn_rows_ok', ROWS, 320, 512, True)),
         launches={'linear_tn_raw': [None], 'linear_tn_ragged_raw': ['h'], '_wgrad': ['weight']}),
    # ---- models.py: the classification fine-tune ---------------------------------------------------------------------------------
    Case('classifier_head', '_ClassifierHeadFn', 'models.py', ('x', 'weight', 'bias'), ('bf16',),
         gemms=(('_tn_ok', ROWS, 256, 256, True),),
         launches={'linear_tn_raw': [None, 'x'], '_wgrad': ['weight']}),
]
BY_NAME = {c.name: c for c in CASES}


def patterns(inputs):
    """The frozen sets a row is run with: none, each single input, and all but each single input (in that order, no repeats)."""
    out = [frozenset()]
    for group in ([frozenset([i]) for i in inputs], [frozenset(inputs) - {i} for i in inputs]):
        for f in group:
            if f not in out and len(f) < len(inputs):
                out.append(f)
    return out


def expected_launches(case, dtype, frozen):
    """{counted function: launches} of one run of `case` with the inputs in `frozen` wanting no gradient."""
    table = case.f32_launches if (dtype == 'f32' and case.f32_launches is not None) else case.launches

    def holds(cond):
        if cond is None:
            return True
        if isinstance(cond, tuple):
            assert cond[0] == 'not'
            return cond[1] in frozen
        return cond not in frozen
    return {fn: sum(holds(c) for c in table.get(fn, ())) for fn in COUNTED}


# ----------------------------------------------------------------------------------------------------------------------------------
# Builders (GPU): build(case, dtype, seed) -> (leaves {input: tensor}, run), run(leaves) -> tuple of outputs to differentiate.
# A leaf's requires_grad is set by the test; everything else a run needs is a constant made here.
# ----------------------------------------------------------------------------------------------------------------------------------
def build(case, dtype):
    import torch
    from lavila_amd import ops
    dev = 'cuda'
    dt = {'bf16': torch.bfloat16, 'f32': torch.float32}[dtype]
    g = torch.Generator().manual_seed(sum(map(ord, case.name)))

    def rnd(*shape, scale=1.0, shift=0.0, dtype=torch.float32):
        return (shift + scale * torch.randn(*shape, generator=g)).to(dev, dtype)

    def ln_consts(D):
        return rnd(D, scale=0.2, shift=1.0), rnd(D, scale=0.3)

    name = case.name
    if name.startswith('linear_') and case.function == '_LinearFn':
        n_out, n_in = {'linear_own': (1024, 256), 'linear_own_recipe': (1024, 256), 'linear_library_192': (192, 192),
                       'linear_own_flip_192_to_256': (256, 192)}[name]
        leaves = dict(x=rnd(ROWS, n_in, dtype=dt), weight=rnd(n_out, n_in, scale=n_in ** -0.5), bias=rnd(n_out, scale=0.1))
        if name == 'linear_own_recipe':
            gam, bet = ln_consts(n_in)

            def run(t):
                h, rec = ops.layer_norm(t['x'], gam, bet, 1e-6, recipe=True)
                return (ops.linear(h, t['weight'], t['bias'], ln=rec),)
        else:
            def run(t):
                return (ops.linear(t['x'], t['weight'], t['bias']),)
        return leaves, run
    if name == 'linear_token':
        leaves = dict(x=rnd(ROWS, 256, dtype=dt), weight=rnd(1024, 256, scale=1 / 16), xtoken=rnd(256))

        def run(t):
            y, tok = ops.linear_with_token(t['x'], t['weight'], t['xtoken'])
            assert tok is not None
            return y, tok
        return leaves, run
    if case.function in ('_MlpFn', '_MlpResidualLayerNormFn'):
        D, Hd = 256, 1024
        leaves = dict(x=rnd(ROWS, D, dtype=dt), w1=rnd(Hd, D, scale=D ** -0.5), b1=rnd(Hd, scale=0.5),
                      w2=rnd(D, Hd, scale=Hd ** -0.5))
        gam, bet = ln_consts(D)
        sel = name.endswith('selective')
        if case.function == '_MlpResidualLayerNormFn':
            leaves.update(b2=rnd(D, scale=0.5), res=rnd(ROWS, D, dtype=dt), gamma=rnd(D, scale=0.2, shift=1.0),
                          beta=rnd(D, scale=0.3))

        def run(t):
            h, rec = ops.layer_norm(t['x'], gam, bet, 1e-6, recipe=True) if sel else (t['x'], None)
            if case.function == '_MlpFn':
                return (ops.mlp_quickgelu(h, t['w1'], t['b1'], t['w2'], ln=rec),)
            out = ops.mlp_residual_layer_norm(h, t['w1'], t['b1'], t['w2'], t['b2'], t['res'], t['gamma'], t['beta'], 1e-6, ln=rec)
            assert out is not None
            return out
        return leaves, run
    if name in ('linear_residual_ln', 'linear_residual_ln_no_bias'):
        leaves = dict(x=rnd(ROWS, 1024, dtype=dt), weight=rnd(256, 1024, scale=1 / 32), lbias=rnd(256, scale=0.1),
                      res=rnd(ROWS, 256, dtype=dt), gamma=rnd(256, scale=0.2, shift=1.0), beta=rnd(256, scale=0.3),
                      xtoken=rnd(1024))
        if name.endswith('no_bias'):
            del leaves['lbias']

        def run(t):
            out = ops.linear_residual_layer_norm(t['x'], t['weight'], t.get('lbias'), t['res'], t['gamma'], t['beta'], 1e-6,
                                                 xtoken=t['xtoken'])
            assert out is not None
            return out
        return leaves, run
    if name in ('add_ln_pass', 'scaled_add_ln'):
        B, T, D = 4, 10, 256
        leaves = dict(res=rnd(B, T, D, dtype=dt), y=rnd(B, T, D, dtype=dt), ybias=rnd(D, scale=0.1),
                      weight=rnd(D, scale=0.2, shift=1.0), bias=rnd(D, scale=0.3), ytoken=rnd(D))
        scale = torch.tensor([0.0, 1.25, 1.25, 0.0], device=dev)

        def run(t):
            if name == 'add_ln_pass':
                return ops.add_layer_norm_pass(t['res'], t['y'], t['ybias'], t['weight'], t['bias'], 1e-6, ytoken=t['ytoken'])
            return ops.scaled_add_layer_norm(t['res'], t['y'], t['ybias'], scale, T, t['weight'], t['bias'], 1e-6,
                                             ytoken=t['ytoken'])
        return leaves, run
    if name == 'text_embed':
        V, W, ctx, B, L = 97, 256, 12, 5, 8
        text = torch.randint(0, V, (B, L), generator=g).to(dev)
        leaves = dict(table=rnd(V, W, scale=0.1), pos=rnd(ctx, W, scale=0.1))

        def run(t):
            x = ops.text_embed(text, t['table'], t['pos'], dt)
            assert x is not None
            return (x,)
        return leaves, run
    if name in ('divided_space', 'divided_time', 'causal_attn'):
        B, Fr, N, H = 2, 4, 9, 4
        D, T = 64 * H, 1 + Fr * N
        leaves = dict(qkv=rnd(B, T, 3 * D, scale=1.2, dtype=dt), bias=torch.zeros(3 * D, device=dev))

        def run(t):
            if name == 'causal_attn':
                return (ops.causal_attention(t['qkv'], H, bias=t['bias']),)
            return (ops.divided_attention(t['qkv'], Fr, N, H, name.split('_')[1], bias=t['bias']),)
        return leaves, run
    if name == 'cls_attn':
        B, T, H = 2, 37, 4
        D = 64 * H
        leaves = dict(q=rnd(B, D, dtype=dt), kv=rnd(B, T, 2 * D, dtype=dt), bias=torch.zeros(3 * D, device=dev))
        return leaves, lambda t: (ops.cls_attention(t['q'], t['kv'], H, bias=t['bias']),)
    if case.function == '_Conv1DFn':
        from lavila_amd import gpt2_gated
        n_in, n_out = {'conv1d_256': (256, 1024), 'conv1d_ragged_320': (320, 320), 'conv1d_flip_192_to_256': (192, 256)}[name]
        leaves = dict(x=rnd(ROWS, n_in, dtype=dt), weight=rnd(n_in, n_out, scale=n_in ** -0.5), bias=rnd(n_out, scale=0.1))
        return leaves, lambda t: (gpt2_gated._Conv1DFn.apply(t['x'], t['weight'], t['bias']),)
    if case.function == '_LmHeadFn':
        from lavila_amd import gpt2_gated
        D = 256 if name == 'lm_head_256' else 320
        leaves = dict(h=rnd(ROWS, D, dtype=dt), weight=rnd(300, D, scale=D ** -0.5))
        return leaves, lambda t: (gpt2_gated._LmHeadFn.apply(t['h'], t['weight']),)
    if name == 'classifier_head':
        from lavila_amd import models
        leaves = dict(x=rnd(ROWS, 256, dtype=dt), weight=rnd(97, 256, scale=1 / 16), bias=rnd(97, scale=0.1))
        return leaves, lambda t: (models._ClassifierHeadFn.apply(t['x'], t['weight'], t['bias']),)
    raise KeyError(name)
