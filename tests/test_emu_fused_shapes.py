"""The shape and architecture matrix of the fused U-Net (tests/fused_shapes.py) on the CPU emulator: every inference program the planner
builds for each shape against the float64 oracle, the planner switches, a second launch on a used context, and the fused training
program at F3.

Measured, largest max |s - ref64| / max(1, max |ref64|) of any program or switch run per shape (bound 5e-5): F1 1.2e-5, F2 7.6e-6,
F3 7.1e-6, F4 4.2e-6, F5 5.5e-6, F6 4.0e-6, F7 1.7e-5, shipped 9x9 9.8e-6.  With the reader of the single-sample fused GroupNorm
adding all WM * 4 slots (before FusedBuilder::check_gn_slots) the same figures were 0.1 to 1.5 at F1 (S = 1, co-operative), F2 (every
program: level 0 is per sample in each), F3 (S = 1, co-operative, training program) and F6 (S = 1)."""
import pytest

from tests import fused_shapes as FS


@pytest.mark.parametrize('name', list(FS.SHAPES))
def test_programs_built_and_refused(emu, name):
    FS.check_plan(name, 'cpu')


@pytest.mark.parametrize('name,prog,B', FS.FORWARD_CASES, ids=[f'{n}-{p}-B{B}' for n, p, B in FS.FORWARD_CASES])
def test_guided_score_matches_oracle(emu, name, prog, B):
    FS.check_forward(name, prog, B, 'cpu')


@pytest.mark.parametrize('name,switch', FS.SWITCH_CASES, ids=[f'{n}-{s}' for n, s in FS.SWITCH_CASES])
def test_planner_switch_matches_oracle_and_default(emu, name, switch):
    FS.check_switch(name, switch, 'cpu')


@pytest.mark.parametrize('name,prog,B', FS.REPEAT_CASES, ids=[f'{n}-{p}-B{B}' for n, p, B in FS.REPEAT_CASES])
def test_second_launch_equals_fresh_context(emu, name, prog, B):
    FS.check_repeat(name, prog, B, 'cpu')


def test_training_forward_f3(emu):
    FS.check_training_forward('F3', 'cpu')
