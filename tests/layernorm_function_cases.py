"""The case matrix of the LayerNorm host layer (tests/test_gpu_layernorm_functions.py, tools/gen_layernorm_call_plans.py).

Every public form of lavila_amd.ops that ends in a LayerNorm Function -- layer_norm, add_layer_norm, add_layer_norm_pass,
linear_residual_layer_norm, mlp_residual_layer_norm -- crossed with what changes the kernels it launches or the operands it
hands them:

  dt        'bf16' (bf16 rows, bf16 parameters: the gradients are cast back), 'f32' (float32 without autocast), 'mixed' (float32
            stream, bf16 branch, bf16 autocast: the lvl_layernorm_*_mixed pair). The GEMM forms are bf16 only.
  keep_sum  add_layer_norm materialises the sum and runs its backward on it
  ybias     the pending bias of the branch (the Linear bias of linear_residual_layer_norm, fc2's of mlp_residual_layer_norm)
  dstream   the first output (the sum, or the stream handed through) has a consumer: its gradient arrives with dh
  token     the column-sum token of the branch (ops.COLSUM_TOKENS); the mixed forms drop it, so it is not crossed with them
  selective mlp_residual_layer_norm's input is a LayerNorm output rebuilt from its recipe (ln=)
  recipe    recipe=True: the form also returns the LnRecipe of its own output

Plain forms: 37 rows (no multiple of the rows per workgroup) x 768 (exact-width kernels) and 320 (general kernels only). GEMM
forms: the shapes of freeze_cases.py (40 rows, 256 x 1024). run() touches nothing but those five public functions."""
import contextlib
import itertools

ROWS, COLS, EPS = 37, (768, 320), 1e-6
GEMM_ROWS, D, HIDDEN = 40, 256, 1024
FLAGS = ('keep_sum', 'ybias', 'dstream', 'token', 'selective', 'recipe')
_B = (False, True)


def _matrix():
    cases = {}

    def add(form, dt, cols, **flags):
        on = [f for f in FLAGS if flags.get(f)]
        cases['-'.join([form, dt, str(cols)] + on)] = dict(form=form, dt=dt, cols=cols, **{f: f in on for f in FLAGS})
    for dt, cols in itertools.product(('bf16', 'f32', 'mixed'), COLS):
        for recipe in _B:
            add('layer_norm', dt, cols, recipe=recipe)
        for keep_sum, ybias, recipe in itertools.product(_B, _B, _B):
            for dstream in (_B if keep_sum else (False,)):           # without the sum there is no first output to consume
                add('add_layer_norm', dt, cols, keep_sum=keep_sum, ybias=ybias, dstream=dstream, recipe=recipe)
        for ybias, dstream, token, recipe in itertools.product(_B, _B, _B, _B):
            if not (token and dt == 'mixed'):
                add('add_layer_norm_pass', dt, cols, ybias=ybias, dstream=dstream, token=token, recipe=recipe)
    for ybias, dstream, token, recipe in itertools.product(_B, _B, _B, _B):
        add('linear_residual_layer_norm', 'bf16', D, ybias=ybias, dstream=dstream, token=token, recipe=recipe)
    for ybias, dstream, selective, recipe in itertools.product(_B, _B, _B, _B):
        add('mlp_residual_layer_norm', 'bf16', D, ybias=ybias, dstream=dstream, selective=selective, recipe=recipe)
    return cases


CASES = _matrix()


def inputs(name):
    """(leaves, consts, cotangents) of the case: leaves {argument: tensor that requires grad}, consts {name: tensor} and the
    cotangents (d first output, dh) in the dtypes the outputs have."""
    import torch
    c = CASES[name]
    bf16, f32 = torch.bfloat16, torch.float32
    g = torch.Generator().manual_seed(sum(map(ord, name)))

    def rnd(*shape, scale=1.0, shift=0.0, dtype=f32):
        return (shift + scale * torch.randn(*shape, generator=g)).to('cuda', dtype)
    stream = bf16 if c['dt'] == 'bf16' else f32
    branch = f32 if c['dt'] == 'f32' else bf16
    cols, consts = c['cols'], {}
    if c['form'] in ('layer_norm', 'add_layer_norm', 'add_layer_norm_pass'):
        rows, pdt = ROWS, (bf16 if c['dt'] == 'bf16' else f32)
        norm = dict(weight=rnd(cols, scale=0.2, shift=1.0, dtype=pdt), bias=rnd(cols, scale=0.3, dtype=pdt))
        if c['form'] == 'layer_norm':
            leaves = dict(x=rnd(rows, cols, scale=2.0, shift=0.5, dtype=stream), **norm)
        else:
            leaves = dict(res=rnd(rows, cols, scale=2.0, shift=0.5, dtype=stream), y=rnd(rows, cols, dtype=branch))
            if c['ybias']:
                leaves['ybias'] = rnd(cols, scale=0.1, dtype=pdt)
            leaves.update(norm)
            if c['token']:
                leaves['ytoken'] = rnd(cols)
    else:
        rows = GEMM_ROWS
        norm = dict(res=rnd(rows, D, dtype=bf16), gamma=rnd(D, scale=0.2, shift=1.0), beta=rnd(D, scale=0.3))
        if c['form'] == 'linear_residual_layer_norm':
            leaves = dict(x=rnd(rows, HIDDEN, dtype=bf16), weight=rnd(D, HIDDEN, scale=1 / 32))
            if c['ybias']:
                leaves['lbias'] = rnd(D, scale=0.1)
            leaves.update(norm)
            if c['token']:
                leaves['xtoken'] = rnd(HIDDEN)
        else:
            leaves = dict(x=rnd(rows, D, dtype=bf16), w1=rnd(HIDDEN, D, scale=D ** -0.5), b1=rnd(HIDDEN, scale=0.5),
                          w2=rnd(D, HIDDEN, scale=HIDDEN ** -0.5))
            if c['ybias']:
                leaves['b2'] = rnd(D, scale=0.5)
            leaves.update(norm)
            consts = dict(gam=rnd(D, scale=0.2, shift=1.0), bet=rnd(D, scale=0.3))
    hdt = bf16 if c['dt'] == 'mixed' else stream
    cot = (rnd(rows, cols, dtype=stream), rnd(rows, cols, dtype=hdt))
    return {k: v.requires_grad_(True) for k, v in leaves.items()}, consts, cot


def _call(ops, c, t, k):
    """The public form on the leaves t (consts k): (tuple of outputs without a None sum, recipe or None, wrt) -- wrt: the
    tensors the gradients are taken of, in the form's argument order."""
    form, recipe = c['form'], c['recipe']
    wrt = dict(t)
    if form == 'layer_norm':
        out = ops.layer_norm(t['x'], t['weight'], t['bias'], EPS, recipe=recipe)
        out = out if recipe else (out,)
    elif form == 'add_layer_norm':
        out = ops.add_layer_norm(t['res'], t['y'], t.get('ybias'), t['weight'], t['bias'], EPS, keep_sum=c['keep_sum'], recipe=recipe)
        assert (out[0] is None) == (not c['keep_sum'])
        out = out if c['keep_sum'] else out[1:]
    elif form == 'add_layer_norm_pass':
        out = ops.add_layer_norm_pass(t['res'], t['y'], t.get('ybias'), t['weight'], t['bias'], EPS, ytoken=t.get('ytoken'),
                                      recipe=recipe)
    elif form == 'linear_residual_layer_norm':
        out = ops.linear_residual_layer_norm(t['x'], t['weight'], t.get('lbias'), t['res'], t['gamma'], t['beta'], EPS,
                                             xtoken=t.get('xtoken'), recipe=recipe)
    else:
        h, ln = ops.layer_norm(t['x'], k['gam'], k['bet'], EPS, recipe=True) if c['selective'] else (t['x'], None)
        wrt['x'] = h                    # the gradient of the MLP's own input: the LayerNorm in front is not under test
        out = ops.mlp_residual_layer_norm(h, t['w1'], t['b1'], t['w2'], t.get('b2'), t['res'], t['gamma'], t['beta'], EPS, ln=ln,
                                          recipe=recipe)
    assert out is not None, 'the fused form refused the configuration'
    return (tuple(out[:-1]), out[-1], wrt) if recipe else (tuple(out), None, wrt)


def run(name, recorder=None):
    """One forward and one backward of the case through the public form. Returns {'case', 'leaves', 'consts', 'cot', 'outs'
    (detached), 'rec' (the LnRecipe or None), 'wrt' (the detached tensors the gradients were taken of), 'grads' {argument:
    gradient}}. recorder: a cabi_recorder.Recorder; its two lists then hold the calls of this forward and this backward."""
    import torch
    from lavila_amd import ops
    c = CASES[name]
    leaves, consts, cot = inputs(name)
    amp = torch.autocast('cuda', dtype=torch.bfloat16) if c['dt'] == 'mixed' else contextlib.nullcontext()
    if recorder is not None:
        recorder.begin()
    with amp:
        outs, rec, wrt = _call(ops, c, leaves, consts)
    if recorder is not None:
        recorder.phase_backward()
    both = c['dstream'] and len(outs) == 2
    grads = torch.autograd.grad(outs if both else outs[-1:], list(wrt.values()), cot if both else cot[-1:])
    torch.cuda.synchronize()
    if recorder is not None:
        recorder.end()
    return dict(case=c, leaves={k: v.detach() for k, v in leaves.items()}, consts=consts, cot=cot,
                outs=tuple(o.detach() for o in outs), rec=rec, wrt={k: v.detach() for k, v in wrt.items()},
                grads=dict(zip(wrt, grads)))
