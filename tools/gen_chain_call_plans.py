"""Writes tests/golden/chain_call_plans.json: the C-ABI calls (tests/cabi_recorder.py) of every case of tests/chain_cases.py,
forward and backward, as this tree makes them on an MI355X. tests/test_gpu_chain_call_plans.py holds every later tree to them.

    python tools/gen_chain_call_plans.py [output path]
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def main():
    import chain_cases
    from cabi_recorder import Recorder, dump_plans
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'chain_call_plans.json')
    plans = {}
    with pytest.MonkeyPatch.context() as mp:
        rec = Recorder(mp)
        for name in chain_cases.CASES:
            chain_cases.run(name, rec)
            plans[name] = {'forward': rec.forward, 'backward': rec.backward}
            print(f'{name}: {len(rec.forward)} forward calls, {len(rec.backward)} backward calls')
    dump_plans(plans, out)
    print(f'{len(plans)} cases -> {out} ({os.path.getsize(out)} bytes)')


if __name__ == '__main__':
    main()
