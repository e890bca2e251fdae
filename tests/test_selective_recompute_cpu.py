"""CPU: what a `use_checkpoint` argument means (ops.checkpoint_mode), without a device."""
import pytest

from lavila_amd import ops


def test_checkpoint_mode_values(monkeypatch):
    assert ops.checkpoint_mode(False) is None and ops.checkpoint_mode(None) is None
    assert ops.checkpoint_mode('block') == 'block'
    assert ops.checkpoint_mode('selective') == 'selective'
    assert ops.CHECKPOINT_MODES == ('block', 'selective')
    monkeypatch.setattr(ops, 'CHECKPOINT', 'block')
    assert ops.checkpoint_mode(True) == 'block'              # the default meaning of the reference drivers' bool
    monkeypatch.setattr(ops, 'CHECKPOINT', 'selective')       # LAVILA_CHECKPOINT=selective
    assert ops.checkpoint_mode(True) == 'selective'
    assert ops.checkpoint_mode(False) is None and ops.checkpoint_mode('block') == 'block'    # only True asks the variable


@pytest.mark.parametrize('bad', ['nonsense', 'Selective', '', 1, 0, 2.0, b'block', ('block',)])
def test_checkpoint_mode_rejects_everything_else(bad):
    with pytest.raises(ValueError):
        ops.checkpoint_mode(bad)


@pytest.mark.parametrize('bad', ['nonsense', '', 'true', '1'])
def test_checkpoint_variable_rejects_everything_else(bad, monkeypatch):
    monkeypatch.setattr(ops, 'CHECKPOINT', bad)
    with pytest.raises(ValueError, match='LAVILA_CHECKPOINT'):
        ops.checkpoint_mode(True)
    assert ops.checkpoint_mode(False) is None and ops.checkpoint_mode('selective') == 'selective'


def test_checkpoint_variable_is_read_from_the_environment():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = 'from lavila_amd import ops; print(ops.CHECKPOINT, ops.checkpoint_mode(True))'
    for env, want in (({}, 'block block'), ({'LAVILA_CHECKPOINT': 'selective'}, 'selective selective')):
        e = {k: v for k, v in os.environ.items() if k != 'LAVILA_CHECKPOINT'}
        e.update(env)
        out = subprocess.run([sys.executable, '-c', code], cwd=root, env=e, capture_output=True, text=True, check=True)
        assert out.stdout.strip().splitlines()[-1] == want
