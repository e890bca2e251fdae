"""Records what the attention host layer ANSWERS, from the built library alone (no GPU, no torch): which shapes run on the
fast kernels (lvl_attention_fast_path[_f32]), the bias-gradient workspace (lvl_divided_attn_bwd_bias_ws) and the attention
workspaces of lvl_workspace_floats, each under every state of the three switches that change the answers.

    python tools/gen_attn_host_golden.py [--lib PATH] [--out tests/golden/attn_host_queries.json]

tests/test_attention_plan_cpu.py calls collect() on the library under test and compares with the committed table, which
was written from the library of the commit BEFORE the family table (csrc/attention.hip) replaced the four hand-kept copies
of the dispatch conditions. Regenerate only when an answer is meant to change.

Every query list is run-length encoded ([value, count] pairs, in the loop order documented in collect()).
"""
import argparse
import ctypes
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODES = (0, 1, 2)                     # LVL_ATTN_SPACE, LVL_ATTN_TIME, LVL_ATTN_CAUSAL
FS = (1, 3, 4, 5, 8, 16, 17, 64, 65)
NS = (1, 16, 196, 255, 256, 257, 271, 272, 273, 287, 288, 576, 591, 592)      # N, or the context length L in mode 2
HS = (1, 3, 4, 12, 16)
BS = (1, 64, 1024)
DTYPES = (0, 1)                       # LVL_F32, LVL_BF16
WS_OPS = ('divided_attn_fwd', 'divided_attn_bwd', 'causal_attn_bwd')
WS_SHAPES = ((1, 1), (12, 785), (768, 785), (576, 3137), (16384, 37889), (3, 77))        # (B*H, T)

# (name of the state, hook, argument); every hook is put back to its default afterwards
DEFAULTS = (('lvl_debug_space_stream', 0), ('lvl_debug_f32_generic', 0), ('lvl_debug_time_bwd_rider', -1))
STATES = (('default', None, None),
          ('space_stream=1', 'lvl_debug_space_stream', 1), ('space_stream=-1', 'lvl_debug_space_stream', -1),
          ('f32_generic=1', 'lvl_debug_f32_generic', 1),
          ('time_bwd_rider=0', 'lvl_debug_time_bwd_rider', 0), ('time_bwd_rider=1', 'lvl_debug_time_bwd_rider', 1),
          ('time_bwd_rider=2', 'lvl_debug_time_bwd_rider', 2))


def _bind(lib):
    i, l = ctypes.c_int, ctypes.c_int64
    for name, res, args in (('lvl_attention_fast_path', i, [i] * 4), ('lvl_attention_fast_path_f32', i, [i] * 4),
                            ('lvl_divided_attn_bwd_bias_ws', l, [i] * 6),
                            ('lvl_workspace_floats', l, [ctypes.c_char_p, l, l]),
                            ('lvl_debug_space_stream', i, [i]), ('lvl_debug_f32_generic', i, [i]),
                            ('lvl_debug_time_bwd_rider', i, [i])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args


def rle(values):
    runs = []
    for v in values:
        if runs and runs[-1][0] == v:
            runs[-1][1] += 1
        else:
            runs.append([v, 1])
    return runs


def unrle(runs):
    return [v for v, n in runs for _ in range(n)]


def fast_path_index(mode, F, N, H):
    return ((MODES.index(mode) * len(FS) + FS.index(F)) * len(NS) + NS.index(N)) * len(HS) + HS.index(H)


def bias_ws_index(dtype, mode, H, B, F, N):
    i = (DTYPES.index(dtype) * 2 + mode) * len(HS) + HS.index(H)
    return ((i * len(BS) + BS.index(B)) * len(FS) + FS.index(F)) * len(NS) + NS.index(N)


def _queries(lib):
    """Loop orders (the last index runs fastest): fast_path[_f32]: mode, F, N, H. bias_ws: dtype, mode (0, 1), H, B, F, N.
    workspace: op, shape."""
    q = {}
    for key, fn in (('fast_path', lib.lvl_attention_fast_path), ('fast_path_f32', lib.lvl_attention_fast_path_f32)):
        q[key] = [fn(m, F, N, H) for m in MODES for F in FS for N in NS for H in HS]
    q['bias_ws'] = [lib.lvl_divided_attn_bwd_bias_ws(B, F, N, H, m, dt)
                    for dt in DTYPES for m in (0, 1) for H in HS for B in BS for F in FS for N in NS]
    q['workspace'] = [lib.lvl_workspace_floats(op.encode(), r, c) for op in WS_OPS for r, c in WS_SHAPES]
    return q


def collect(lib):
    """{state: {query: run-length list}} of the library behind the ctypes handle `lib`."""
    _bind(lib)
    table = {}
    try:
        for state, hook, arg in STATES:
            for name, v in DEFAULTS:
                assert getattr(lib, name)(v) == 0
            if hook:
                assert getattr(lib, hook)(arg) == 0
            table[state] = {k: rle(v) for k, v in _queries(lib).items()}
    finally:
        for name, v in DEFAULTS:
            getattr(lib, name)(v)
    return table


def self_check(lib, table):
    """The table must be able to see what it is there for: the spot values of the issue, and a dq-rider term that decides
    the bias-gradient workspace for each family that has one (else the test is blind to the rider's row count)."""
    d = {k: unrle(v) for k, v in table['default'].items()}
    fp = lambda key, *a: d[key][fast_path_index(*a)]
    assert fp('fast_path', 0, 65, 196, 12) == 0 and fp('fast_path', 0, 64, 196, 12) == 1
    assert fp('fast_path', 1, 5, 196, 12) == 1 and fp('fast_path_f32', 1, 5, 196, 12) == 0
    assert fp('fast_path', 1, 5, 196, 3) == 0
    assert lib.lvl_attention_fast_path(2, 1, 256, 8) == 1 and lib.lvl_attention_fast_path(2, 1, 257, 8) == 0
    assert fp('fast_path', 2, 1, 256, 4) == 1 and fp('fast_path', 2, 1, 257, 4) == 0
    assert unrle(table['space_stream=1']['fast_path'])[fast_path_index(0, 65, 16, 4)] == 0
    assert lib.lvl_divided_attn_bwd_bias_ws(2, 4, 196, 12, 0, 1) == 1671168
    no_rider = unrle(table['time_bwd_rider=0']['bias_ws'])
    streamed = unrle(table['space_stream=1']['bias_ws'])
    for dt in DTYPES:
        won = {0: 0, 1: 0}
        for m in (0, 1):
            for H in HS:
                floor = lib.lvl_workspace_floats(b'qkv_bias_grad', 0, H * 64)       # the "pass" term
                for B in BS:
                    for F in FS:
                        for N in NS:
                            i = bias_ws_index(dt, m, H, B, F, N)
                            assert d['bias_ws'][i] >= floor
                            if d['bias_ws'][i] > floor:
                                won[m] += 1
                                # the rider's rows come from the family: without the family, no rider term
                                assert (streamed if m == 0 else no_rider)[i] == floor
        assert won[0] > 0, 'no space shape where the fused kernel\'s B*F rider rows size ws2'
        assert won[1] > 0, 'no time shape where the register-tiled kernels\' B*NC rider rows size ws2'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=os.path.join(ROOT, 'lavila_amd', 'lib', 'liblavila_hip.so'))
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'attn_host_queries.json'))
    a = ap.parse_args()
    lib = ctypes.CDLL(a.lib)
    table = collect(lib)
    self_check(lib, table)
    with open(a.out, 'w') as f:
        json.dump(table, f, separators=(',', ':'))
        f.write('\n')
    print(a.out, os.path.getsize(a.out), 'bytes')


if __name__ == '__main__':
    main()
