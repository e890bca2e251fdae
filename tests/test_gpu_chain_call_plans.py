"""GPU (-m gpu): the fused residual chain makes the recorded C-ABI calls.

Every case of chain_cases.py -- the video tower under every checkpoint mode, activation, stochastic depth, the float32
stream; the OpenAI image and text towers; DistilBERT; the reference-signature forward of one block of each kind -- runs one
forward and one backward with every entry of the library wrapped (cabi_recorder.py). The two ordered lists of calls, with
their integer and float arguments and with which operands are there, must equal tests/golden/chain_call_plans.json
(tools/gen_chain_call_plans.py) exactly: a change of the Python layer above the kernels that enqueues another kernel, the same
kernels in another order or on other shapes, keeps another operand or drops a fused form shows here."""
import os

import pytest

import chain_cases
from cabi_recorder import Recorder, load_plans
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
_RESIDUAL = 3          # LVL_EPI_BIAS_RESIDUAL


@pytest.fixture(scope='module')
def plans():
    return load_plans(os.path.join(GOLDEN, 'chain_call_plans.json'))


def test_the_recorded_file_holds_exactly_the_matrix(plans):
    assert list(plans) == list(chain_cases.CASES)


def _residual_gemms(calls):
    """(M, N, K) of every lvl_linear_tn call with the residual epilogue (and its residual operand)."""
    from lavila_amd import _cabi as C
    assert C.EPI_BIAS_RESIDUAL == _RESIDUAL
    return [tuple(c[10:13]) for c in calls if c[0] == 'lvl_linear_tn' and c[13] == _RESIDUAL and c[6] == 'ptr']


@pytest.mark.parametrize('name', list(chain_cases.CASES))
def test_case_makes_the_recorded_calls(name, plans, monkeypatch):
    rec = Recorder(monkeypatch)
    chain_cases.run(name, rec)
    got, want = {'forward': rec.forward, 'backward': rec.backward}, plans[name]
    if name in chain_cases.bf16_own_gemm_cases():
        # the matrix is on the benched route: the projection's residual epilogue, and where an MLP waits, fc2's
        square = [mnk for mnk in _residual_gemms(got['forward']) if mnk[1] == mnk[2] == 256]
        assert square, f'{name}: no lvl_linear_tn call with the residual epilogue'
        if name in chain_cases.deferred_mlp_cases():
            assert [mnk for mnk in _residual_gemms(got['forward']) if mnk[1:] == (256, 1024)], \
                f'{name}: no fused MLP with the residual epilogue'
    for phase in ('forward', 'backward'):
        for i, (g, w) in enumerate(zip(got[phase], want[phase])):
            assert g == w, f'{name}: {phase} call {i} is {g}, recorded {w}'
        assert len(got[phase]) == len(want[phase]), \
            f'{name}: {len(got[phase])} {phase} calls, recorded {len(want[phase])}: {[c[0] for c in got[phase]]}'
