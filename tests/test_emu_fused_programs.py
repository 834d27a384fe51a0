"""The fused programs of every configuration of tests/fused_programs.py, built by the CPU emulator build of the library, against the
recorded tests/golden/fused_programs.json.  tests/test_gpu_fused_programs.py asks the same of librdmi.so on an MI355X."""
import pytest

from tests import fused_programs as F


@pytest.mark.parametrize('name', list(F.CONFIGS))
def test_programs_match_the_recorded_plan(emu, name):
    """rdmi_path_info, the programs that exist (S, coop, train), their op counts and the SHA-256 of their op descriptions equal the
    fixture; for the shipped configurations the op lists are compared one by one."""
    F.check(name, 'cpu')
