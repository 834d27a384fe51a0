"""The shape and architecture matrix of the fused U-Net (tests/fused_shapes.py) on an MI355X: the checks of
tests/test_emu_fused_shapes.py on the device.  Every case is a single launch of at most 8 network evaluations on at most 81 pixels;
the per-sample errors are printed by the checks (run with -s).

Measured on an MI355X, largest max |s - ref64| / max(1, max |ref64|) of any program or switch run per shape (bound 2e-4):
F1 3.5e-5, F2 1.0e-5, F3 1.6e-5, F4 9.3e-6, F5 1.3e-5, F6 8.2e-6, F7 3.8e-5, shipped 9x9 1.3e-5; switch runs against the run without
the switch at most 5.4e-6; second launches bit-equal; F3 training forward 3.1e-6, worst parameter gradient 5.5e-6 of ||g64||."""
import pytest

from tests import fused_shapes as FS

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def _device_library():
    import torch
    import __graft_entry__ as ge
    from rdmi import _native
    if _native._lib is not None and _native.is_emulator():
        pytest.fail('the emulator build is bound: GPU tests need librdmi.so')
    ge.build()
    assert not _native.is_emulator()
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'


@pytest.mark.parametrize('name', list(FS.SHAPES))
def test_programs_built_and_refused(name):
    FS.check_plan(name, DEV)


@pytest.mark.parametrize('name,prog,B', FS.FORWARD_CASES, ids=[f'{n}-{p}-B{B}' for n, p, B in FS.FORWARD_CASES])
def test_guided_score_matches_oracle(name, prog, B):
    FS.check_forward(name, prog, B, DEV)


@pytest.mark.parametrize('name,switch', FS.SWITCH_CASES, ids=[f'{n}-{s}' for n, s in FS.SWITCH_CASES])
def test_planner_switch_matches_oracle_and_default(name, switch):
    FS.check_switch(name, switch, DEV)


@pytest.mark.parametrize('name,prog,B', FS.REPEAT_CASES, ids=[f'{n}-{p}-B{B}' for n, p, B in FS.REPEAT_CASES])
def test_second_launch_equals_fresh_context(name, prog, B):
    FS.check_repeat(name, prog, B, DEV)


def test_training_forward_f3():
    FS.check_training_forward('F3', DEV)
