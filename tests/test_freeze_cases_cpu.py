"""CPU: the case table of test_gpu_freeze_ops.py (freeze_cases.py) and the freeze-space helper (freeze_recipes.py).

  * every autograd Function of ops.py, gpt2_gated.py and models.py whose code mentions needs_input_grad has a row (source scan);
  * every GEMM shape of a row answers the routing predicate of ops.py as the row claims;
  * the launch conditions of a row speak of its own inputs and of functions ops.py has;
  * the freeze-space pattern derived from remap_keys equals the flags the reference's constructor left."""
import ast
import os

import pytest
import torch

import freeze_cases as FC
import freeze_recipes as FR
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# module-level helpers that read ctx.needs_input_grad on behalf of Functions: each of those Functions must have a row
SHARED_HELPERS = {'_mlp_backward': ('_MlpFn', '_MlpResidualLayerNormFn')}


def _mentions(source):
    """({class name}, {module-level function name}) whose code mentions needs_input_grad."""
    tree = ast.parse(source)
    classes, functions = set(), set()
    for node in tree.body:
        if not isinstance(node, (ast.ClassDef, ast.FunctionDef)):
            continue
        hit = any(isinstance(n, ast.Attribute) and n.attr == 'needs_input_grad' for n in ast.walk(node))
        if hit:
            (classes if isinstance(node, ast.ClassDef) else functions).add(node.name)
    return classes, functions


def test_every_function_that_reads_needs_input_grad_has_a_row():
    found = set()
    for src in FC.SOURCES:
        with open(os.path.join(ROOT, 'lavila_amd', src)) as f:
            classes, functions = _mentions(f.read())
        rows = {c.function for c in FC.CASES if c.source == src}
        assert classes <= rows, f'{src}: no row for {sorted(classes - rows)}'
        assert rows <= classes | {u for h in functions for u in SHARED_HELPERS.get(h, ())}, \
            f'{src}: rows for Functions that do not read needs_input_grad: {sorted(rows - classes)}'
        for helper in functions:
            assert helper in SHARED_HELPERS, f'{src}: {helper} reads needs_input_grad and is not known to the table'
            assert set(SHARED_HELPERS[helper]) <= rows, helper
        found |= classes | {u for h in functions for u in SHARED_HELPERS[h]}
    assert len(found) == 14, sorted(found)


def test_the_scan_sees_a_function_that_is_added():
    classes, functions = _mentions('class A:\n    def backward(ctx, d):\n        return d if ctx.needs_input_grad[0] else None\n'
                                   'class B:\n    pass\n'
                                   'def helper(ctx):\n    return ctx.needs_input_grad\n')
    assert classes == {'A'} and functions == {'helper'}


@pytest.mark.parametrize('case', FC.CASES, ids=[c.name for c in FC.CASES])
def test_row_is_consistent(case):
    from lavila_amd import ops
    assert case.source in FC.SOURCES and set(case.dtypes) <= {'bf16', 'f32'} and case.dtypes
    assert len(set(case.inputs)) == len(case.inputs) >= 2
    for pred, rows, n_out, n_in, expected in case.gemms:
        assert getattr(ops, pred)(rows, n_out, n_in) is expected, (case.name, pred, rows, n_out, n_in)
    for table in (case.launches, case.f32_launches or {}):
        for fn, conds in table.items():
            assert fn in FC.COUNTED and callable(getattr(ops, fn)), fn
            for c in conds:
                name = c[1] if isinstance(c, tuple) else c
                assert name is None or name in case.inputs, (case.name, fn, c)
    assert set(case.switch) <= set(case.inputs) and bool(case.switch) == bool(case.switch_results)
    # a frozen weight: no weight-gradient GEMM; a frozen activation: one forward / input-gradient GEMM less
    all_on = FC.expected_launches(case, case.dtypes[0], frozenset())
    for name in case.inputs:
        off = FC.expected_launches(case, case.dtypes[0], frozenset([name]))
        if name in case.switch:
            continue
        assert all(off[fn] <= all_on[fn] for fn in FC.COUNTED), (case.name, name)


def test_own_kernel_rows_sit_at_the_smallest_shapes():
    """40 rows (one partial tile), widths 256 / 1024 on lvl_linear_tn, 320 on the ragged entry, 192 on the library."""
    from lavila_amd import ops
    assert FC.ROWS == 40
    assert ops._tn_ok(40, 256, 1024) and ops._tn_ok(40, 1024, 256) and not ops._tn_ok(40, 320, 320)
    assert ops._tn_ragged_ok(40, 320, 320) and not ops._tn_rows_ok(40, 192, 192)
    names = {c.name for c in FC.CASES}
    assert {'conv1d_256', 'conv1d_ragged_320', 'lm_head_256', 'lm_head_ragged_320', 'linear_library_192'} <= names


def test_patterns():
    p = FC.patterns(('a', 'b', 'c'))
    assert p[0] == frozenset() and len(p) == 7 and len(set(p)) == 7
    assert sum(len(f) == 1 for f in p) == 3 and sum(len(f) == 2 for f in p) == 3
    assert FC.patterns(('a', 'b')) == [frozenset(), frozenset('a'), frozenset('b')]


def test_freeze_space_pattern_equals_the_reference_constructor():
    want = load_golden('reference_boundary.pt')['pretrained_clip']['512-True']['requires_grad']
    vis = {k[len('visual.'):]: v for k, v in want.items() if k.startswith('visual.')}
    assert len(vis) == 224
    got = FR.freeze_space_flags(list(vis), depth=12)
    assert got == vis
    assert got['cls_token'] and got['temporal_embed'] and not got['pos_embed'] and not got['norm.weight']
    assert got['blocks.11.norm3.bias'] and got['blocks.11.timeattn.proj.weight'] and not got['blocks.11.mlp.fc2.bias']
    # the unfrozen constructor trains everything
    assert all(load_golden('reference_boundary.pt')['pretrained_clip']['256-False']['requires_grad'].values())


def test_freeze_space_differs_from_freeze_spatial_weights_in_cls_token_only():
    import contextlib
    import io
    from lavila.models.timesformer import SpaceTimeTransformer
    with contextlib.redirect_stdout(io.StringIO()):
        vis = SpaceTimeTransformer(img_size=32, patch_size=16, embed_dim=64, depth=2, num_heads=1, num_frames=2, ln_pre=True,
                                   num_classes=0)
        a = FR.apply_recipe(vis, 'freeze_space')
        b = FR.apply_recipe(vis, 'spatial')
        c = FR.apply_recipe(vis, 'temporal')
    assert {k for k in a if a[k] != b[k]} == {'cls_token'}
    assert all(b[k] != c[k] for k in b)
    assert all(FR.apply_recipe(vis, 'none').values())
