"""Writes tests/golden/layernorm_call_plans.json: the C-ABI calls (tests/cabi_recorder.py) of every case of
tests/layernorm_function_cases.py, forward and backward, as this tree makes them on an MI355X. It reaches the tree through the
public forms of lavila_amd.ops only (layer_norm, add_layer_norm, add_layer_norm_pass, linear_residual_layer_norm,
mlp_residual_layer_norm), so it runs unchanged on a tree from before a refactor of what lies below them;
tests/test_gpu_layernorm_functions.py holds every later tree to the file.

    python tools/gen_layernorm_call_plans.py [output path]
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def main():
    import layernorm_function_cases as LC
    from cabi_recorder import Recorder, dump_plans
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'layernorm_call_plans.json')
    plans = {}
    with pytest.MonkeyPatch.context() as mp:
        rec = Recorder(mp)
        for name in LC.CASES:
            LC.run(name, rec)
            plans[name] = {'forward': rec.forward, 'backward': rec.backward}
    dump_plans(plans, out)
    calls = sum(len(p['forward']) + len(p['backward']) for p in plans.values())
    print(f'{len(plans)} cases, {calls} calls -> {out} ({os.path.getsize(out)} bytes)')


if __name__ == '__main__':
    main()
