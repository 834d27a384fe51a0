"""The fused programs of every configuration of tests/fused_programs.py, built by librdmi.so on an MI355X, against the recorded
tests/golden/fused_programs.json: the check of tests/test_emu_fused_programs.py on the device (contexts only, nothing is launched)."""
import pytest

from tests import fused_programs as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _device_library():
    from rdmi import _native
    if _native._lib is not None and _native.is_emulator():
        pytest.fail('the emulator build is bound: GPU tests need librdmi.so')


@pytest.mark.parametrize('name', list(F.CONFIGS))
def test_programs_match_the_recorded_plan(name):
    F.check(name, 'cuda:0')
