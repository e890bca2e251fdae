"""The attention host layer answers what it answered before the family table: every host-only query of the built library
(fast-path, bias-gradient workspace, attention workspaces; under each state of lvl_debug_space_stream / _f32_generic /
_time_bwd_rider) against tests/golden/attn_host_queries.json, which tools/gen_attn_host_golden.py recorded from the library
of the commit before csrc/attention.hip got its one table of kernel families. No GPU: none of these calls touches a device."""
import ctypes
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_generator():
    spec = importlib.util.spec_from_file_location('gen_attn_host_golden',
                                                  os.path.join(ROOT, 'tools', 'gen_attn_host_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _load_generator()


@pytest.fixture(scope='module')
def lib():
    from lavila_amd import _cabi
    _cabi.lib()                                   # raises if the library is not built
    return ctypes.CDLL(_cabi.LIB_PATH)            # own handle: the generator binds its own argument types


@pytest.fixture(scope='module')
def answers(lib):
    return GEN.collect(lib)


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(ROOT, 'tests', 'golden', 'attn_host_queries.json')) as f:
        return json.load(f)


def test_table_covers_every_switch_state(golden):
    assert sorted(golden) == sorted(s[0] for s in GEN.STATES)
    n_fp = len(GEN.MODES) * len(GEN.FS) * len(GEN.NS) * len(GEN.HS)
    for state in golden.values():
        assert len(GEN.unrle(state['fast_path'])) == len(GEN.unrle(state['fast_path_f32'])) == n_fp
        assert len(GEN.unrle(state['bias_ws'])) == len(GEN.DTYPES) * 2 * len(GEN.HS) * len(GEN.BS) * len(GEN.FS) * len(GEN.NS)
        assert len(GEN.unrle(state['workspace'])) == len(GEN.WS_OPS) * len(GEN.WS_SHAPES)


@pytest.mark.parametrize('state', [s[0] for s in GEN.STATES])
@pytest.mark.parametrize('query', ['fast_path', 'fast_path_f32', 'bias_ws', 'workspace'])
def test_host_answers_equal_the_recorded_ones(answers, golden, state, query):
    got, want = GEN.unrle(answers[state][query]), GEN.unrle(golden[state][query])
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert len(got) == len(want) and not bad, f'{state} / {query}: {len(bad)} answers differ, first at index {bad[:5]}'


def test_table_sees_the_riders_and_the_spot_values(lib, answers):
    GEN.self_check(lib, answers)


def test_switches_are_back_at_their_defaults(lib, answers):
    # after collect(): the default state's answers again, straight from the library
    assert lib.lvl_attention_fast_path(0, 64, 576, 12) == 1 and lib.lvl_attention_fast_path_f32(1, 4, 196, 12) == 1
    d = GEN.unrle(answers['default']['bias_ws'])
    assert lib.lvl_divided_attn_bwd_bias_ws(1024, 4, 196, 12, 1, 1) == d[GEN.bias_ws_index(1, 1, 12, 1024, 4, 196)]
