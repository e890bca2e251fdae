"""The boundary of the mixed-dtype LayerNorm entry points (lvl_layernorm_fwd_mixed / lvl_layernorm_bwd_mixed), without a GPU:
declaration against ctypes signature, the flag values, the launcher's grid caps, and the dtype checks that stand in for the
dtype tag these entry points do not take."""
import os
import re

import pytest
import torch

import rowops_reference as R

HEADER = os.path.join(R.ROOT, 'include', 'lavila_hip.h')


def _decl(name):
    src = open(HEADER).read()
    m = re.search(r'\bint ' + name + r'\(([^;]*)\);', src)
    assert m, f'{name} is not declared in lavila_hip.h'
    return [a.strip() for a in m.group(1).replace('\n', ' ').split(',')]


@pytest.mark.parametrize('name', ('lvl_layernorm_fwd_mixed', 'lvl_layernorm_bwd_mixed'))
def test_signature_matches_the_declaration(name):
    import ctypes
    from lavila_amd import _cabi as C
    res, args = C.SIGNATURES[name]
    decl = _decl(name)
    assert res is ctypes.c_int and len(args) == len(decl)
    for a, d in zip(args, decl):
        want = ctypes.c_void_p if '*' in d else {'int64_t': ctypes.c_int64, 'int': ctypes.c_int, 'float': ctypes.c_float}[
            d.split()[0]]
        assert a is want, (name, d, a)
    # the same operands in the same order as the single-dtype entry point, `flags` where that one has `dtype`
    base = _decl(name[:-len('_mixed')])
    names = lambda decl: [d.split()[-1].lstrip('*') for d in decl]
    assert [n.replace('dx_plain', 'dx2').replace('dtype', 'flags') for n in names(base)] == names(decl)


def test_flag_values_match_the_header():
    from lavila_amd import _cabi as C
    src = open(HEADER).read()
    m = re.search(r'enum \{ LVL_LN_PLAIN = (\d+), LVL_LN_GENERAL = (\d+) \};', src)
    assert m and (C.LN_PLAIN, C.LN_GENERAL) == (int(m.group(1)), int(m.group(2)))
    assert C.LN_PLAIN & C.LN_GENERAL == 0


def test_mixed_forward_uses_the_float32_launchers_grid():
    """One function sizes the grid of both forward entry points; rowops_reference mirrors its caps."""
    src = open(os.path.join(R.CSRC, 'layernorm.hip')).read()
    for name in ('lvl_layernorm_fwd', 'lvl_layernorm_fwd_mixed'):
        body = src[src.index(f'extern "C" int {name}('):]
        assert 'blocks = ln_fwd_blocks(rows, x2);' in body[:body.index('extern "C"', 10)], name
    fn = src[src.index('static int64_t ln_fwd_blocks('):]
    m = re.search(r'const int64_t cap = x2 == nullptr \? (\d+) : (\d+);', fn[:fn.index('\n}\n')])
    assert (int(m.group(1)), int(m.group(2))) == (R.LN_FWD_BLOCKS, R.LN_FWD_X2_BLOCKS)


def test_raw_wrappers_check_the_dtypes_the_entry_points_assume():
    from lavila_amd import ops
    x, x2 = torch.zeros(4, 16), torch.zeros(4, 16, dtype=torch.bfloat16)
    ops._mixed_dtypes(x, x2, x2, x)
    ops._mixed_dtypes(x, None)
    for bad in ((x2, x2), (x, x), (x, x2, x), (x, x2, x2, x2), (x.t(), None)):
        with pytest.raises(TypeError):
            ops._mixed_dtypes(*bad)
    with pytest.raises(ValueError):
        ops._mixed_dtypes(x, x2[:2])


def test_mixed_path_needs_a_float32_stream_a_bf16_branch_and_a_bf16_consumer(monkeypatch):
    from lavila_amd import ops

    class Cuda:                      # what _mixed_ln reads of a tensor
        is_cuda = True

        def __init__(self, dtype):
            self.dtype = dtype
    f32, bf16 = Cuda(torch.float32), Cuda(torch.bfloat16)
    monkeypatch.setattr(ops, 'autocast_dtype', lambda: torch.bfloat16)
    assert ops._mixed_ln(f32) and ops._mixed_ln(f32, bf16)
    assert not ops._mixed_ln(bf16) and not ops._mixed_ln(f32, f32) and not ops._mixed_ln(bf16, bf16)
    assert not ops._mixed_ln(torch.zeros(2, 8))                  # a host tensor
    monkeypatch.setattr(ops, 'autocast_dtype', lambda: None)  # no autocast: a true float32 run
    assert not ops._mixed_ln(f32) and not ops._mixed_ln(f32, bf16)
